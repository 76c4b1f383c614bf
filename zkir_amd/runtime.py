"""Host-side mirror of the reference's `zkir_runtime` API on top of the C ABI (include/zkir_amd.h).

    reference (Rust)                                   here
    -----------------------------------------------    ---------------------------------------------
    VMConfig {max_cycles, trace, enable_* ..}          VMConfig                      vm.rs:15-50
    VM::new(program, inputs, config)                   VM(program, inputs, config)   vm.rs:138
    VM::run(self) -> Result<ExecutionResult>           VM.run() -> ExecutionResult   vm.rs:208
    ExecutionResult.{cycles, outputs, halt_reason,     same attribute names          vm.rs:54-78
       range_check_witnesses, execution_trace,
       normalization_witnesses}
    ExecutionResult::get_memory_trace()                ExecutionResult.get_memory_trace()   vm.rs:85-94
    RuntimeError::{MisalignedAccess, ..}               RuntimeError(code, message)   error.rs:7-37
    zkir_runtime::run(program, inputs)                 run(program, inputs)          lib.rs:59-62

The wide execution trace stays resident in HBM (SoA columns); `execution_trace.column(...)` copies one
column to the host, `execution_trace.rows()` reassembles reference-shaped TraceRow records (for tests).
There is no CPU fallback: without the built HIP library or without a GPU, trace collection raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .spec import Program

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZKIR_AMD_LIB: another build of the same library (kernel experiments: scripts/build_variant.py); the default is the in-tree build
_SO = os.environ.get("ZKIR_AMD_LIB") or os.path.join(_HERE, "libzkir_amd.so")

(ZKIR_OK, ERR_MISALIGNED, ERR_INVALID_MEMORY, ERR_DIV_ZERO, ERR_INVALID_SYSCALL, ERR_DECODE, ERR_OTHER, ERR_BAD_PROGRAM,
 ERR_DEVICE, ERR_ARGUMENT) = range(10)
HALT_EBREAK, HALT_EXIT, HALT_CYCLE_LIMIT = 0, 1, 2

REG_EVENT_DTYPE = np.dtype([("value", "<u8"), ("payload", "<u8"), ("max_bits", "<u4"), ("vis", "<u4"), ("reg", "u1"),
                            ("state", "u1"), ("tag", "u1"), ("pad", "u1", (5,))])
MEM_EVENT_DTYPE = np.dtype([("address", "<u8"), ("value", "<u8"), ("row", "<u4"), ("is_write", "u1"), ("width", "u1"), ("pad", "<u2")])
RC_EVENT_DTYPE = np.dtype([("value", "<u8"), ("pc", "<u8")])
NORM_EVENT_DTYPE = np.dtype([("cycle", "<u8"), ("pc", "<u8"), ("raw_value", "<u8"), ("reg", "u1"), ("state", "u1"), ("opcode", "u1"),
                             ("pad", "u1", (5,))])
SHA_BLOCK_DTYPE = np.dtype([("message_block", "<u4", (16,)), ("timestamp", "<u8")])
HASH_OUT_DTYPE = np.dtype([("row", "<u4"), ("reserved", "<u4"), ("bytes", "u1", (32,))])      # zkir_hash_out
assert REG_EVENT_DTYPE.itemsize == 32 and MEM_EVENT_DTYPE.itemsize == 24 and NORM_EVENT_DTYPE.itemsize == 32 and SHA_BLOCK_DTYPE.itemsize == 72 and HASH_OUT_DTYPE.itemsize == 40

_MEMOP_DTYPE = np.dtype([("address", "<u8"), ("value", "<u8"), ("timestamp", "<u8"), ("is_write", "u1"), ("width", "u1"),
                         ("bound_bits", "<u4"), ("bound_tag", "u1"), ("bound_payload", "<u8")])
_NORM_DTYPE = np.dtype([("cycle", "<u8"), ("pc", "<u8"), ("reg", "u1"), ("accumulated", "<u8", (2,)), ("normalized", "<u4", (2,)),
                        ("carries", "<u4", (2,)), ("normalized_bits", "u1"), ("limb_bits", "u1"), ("cause", "u1"), ("opcode", "u1")])

FIELD_CYCLE, FIELD_PC, FIELD_INSTRUCTION, FIELD_REGISTERS, FIELD_BOUND_BITS, FIELD_BOUND_TAG, FIELD_BOUND_PAYLOAD, FIELD_REG_STATE = range(8)
_FIELD_DTYPE = {0: "<u8", 1: "<u8", 2: "<u4", 3: "<u8", 4: "<u4", 5: "u1", 6: "<u8", 7: "u1"}


class RuntimeError(Exception):  # noqa: A001 - mirrors zkir_runtime::RuntimeError
    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code, self.message = code, message


class VmConfigC(C.Structure):
    _fields_ = [("max_cycles", C.c_uint64), ("trace", C.c_uint8), ("enable_range_checking", C.c_uint8),
                ("enable_execution_trace", C.c_uint8), ("enable_deferred_model", C.c_uint8)]


class TraceColumnsC(C.Structure):
    _fields_ = [("cycle", C.c_void_p), ("pc", C.c_void_p), ("instruction", C.c_void_p), ("registers", C.c_void_p),
                ("bound_bits", C.c_void_p), ("bound_tag", C.c_void_p), ("bound_payload", C.c_void_p), ("reg_state", C.c_void_p),
                ("reg_stride", C.c_uint64)]


class TraceFillArgsC(C.Structure):
    _fields_ = [("events", C.c_void_p), ("tile_ev_off", C.c_void_p), ("tile_snap", C.c_void_p), ("n_rows", C.c_uint64),
                ("cycle_base", C.c_uint64), ("tile_rows", C.c_uint32), ("n_events", C.c_uint32), ("out", TraceColumnsC)]


class MemopColumnsC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("address", "value", "timestamp", "is_write", "width", "bound_bits", "bound_tag", "bound_payload")]


class NormColumnsC(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("cycle", "pc", "reg", "opcode", "accumulated0", "accumulated1", "normalized0", "normalized1",
                                         "carry0", "carry1")]


class ProverParamsC(C.Structure):             # zkir_prover_params
    _fields_ = [("mode", C.c_uint32), ("num_queries", C.c_uint32), ("pow_bits", C.c_uint32)]


class PublicInputsC(C.Structure):             # zkir_public_inputs
    _fields_ = [("n_real", C.c_uint64), ("entry_point", C.c_uint64), ("deferred", C.c_uint32), ("fri_params", C.c_uint32),
                ("program_digest", C.c_uint32 * 4), ("io_digest", C.c_uint32 * 4),
                ("program_blob", C.c_void_p), ("program_blob_len", C.c_uint64),      # borrowed pointer (prover side): see with_program()
                # mode 2 (`deferred` == 2: default VM mode + the I/O argument): the tapes and the halt reason in the clear (borrowed pointers: with_io()); for a SEGMENT
                # the WRITE / READ ecalls executed before its first row
                ("inputs", C.c_void_p), ("n_inputs", C.c_uint64), ("outputs", C.c_void_p), ("n_outputs", C.c_uint64), ("halt_kind", C.c_uint32), ("reserved2", C.c_uint32),
                ("halt_code", C.c_uint64), ("writes_before", C.c_uint64), ("reads_before", C.c_uint64),
                # mode 3 (`deferred` == 3: mode 2 + the memory argument): the memory witness of the run (borrowed pointers into a MemcheckWitness: with_memory())
                ("mem_old", C.c_void_p), ("mem_told", C.c_void_p), ("cell_addr", C.c_void_p), ("cell_bytes", C.c_void_p), ("cell_time", C.c_void_p), ("n_cells", C.c_uint64),
                # mode 4 (`deferred` == 4: mode 3 + the wide-arithmetic class + hash syscalls as a tape): the hash calls as the proof's hash section (borrowed from a MemcheckWitness)
                ("hash_section", C.c_void_p), ("hash_section_words", C.c_uint64),
                # (ABI 7) what the run's hash syscalls wrote, borrowed from the run's delta log (zkir_public_inputs_of): the device witness of mode 4 reads the digests from here
                ("hash_outs", C.c_void_p), ("n_hash_outs", C.c_uint64)]

    def with_params(self, num_queries: int = 0, pow_bits: int = 0) -> "PublicInputsC":
        """zkir_public_inputs_set_params: the prover's FRI parameters (0 = the defaults: 50 queries, 12 grinding bits; accepted 50..128 / 12..24).  A verifier given this
        struct as `expect` requires exactly them."""
        pr = ProverParamsC(int(self.deferred), int(num_queries), int(pow_bits))
        L = lib()
        L.zkir_public_inputs_set_params.restype = C.c_int
        L.zkir_public_inputs_set_params.argtypes = [C.c_void_p, C.c_void_p]
        rc = L.zkir_public_inputs_set_params(C.byref(self), C.byref(pr))
        if rc != ZKIR_OK:
            _raise(rc)
        return self

    def with_memory(self, witness: "MemcheckWitness") -> "PublicInputsC":
        """zkir_public_inputs_set_memory: mode 3 — point the struct at the run's memory witness (kept alive by the struct)."""
        self._mem_ref = witness
        lib().zkir_public_inputs_set_memory(C.byref(self), witness._h)
        return self

    def with_io(self, inputs, outputs, halt=None, writes_before=None, reads_before=None) -> "PublicInputsC":
        """Point the struct at its own copies of the I/O tapes (kept alive by the struct); halt = a HaltReason or (kind, code)."""
        self._in_ref = np.ascontiguousarray(np.asarray([int(x) & (2**64 - 1) for x in inputs], dtype=np.uint64))
        self._out_ref = np.ascontiguousarray(np.asarray([int(x) & (2**64 - 1) for x in outputs], dtype=np.uint64))
        self.inputs, self.n_inputs = (self._in_ref.ctypes.data if len(self._in_ref) else None), len(self._in_ref)
        self.outputs, self.n_outputs = (self._out_ref.ctypes.data if len(self._out_ref) else None), len(self._out_ref)
        if halt is not None:
            kind, code = (halt.kind, halt.code) if hasattr(halt, "kind") else halt
            self.halt_kind, self.halt_code = int(kind), int(code or 0) if int(kind) == 1 else 0
        if writes_before is not None:
            self.writes_before = int(writes_before)
        if reads_before is not None:
            self.reads_before = int(reads_before)
        return self

    def with_program(self, blob: bytes) -> "PublicInputsC":
        """Point the struct at `blob` (kept alive by the struct): needed after the struct has been copied byte-wise or sent to another
        process, where the borrowed pointer means nothing."""
        self._blob_ref = bytes(blob)
        self._blob_buf = C.create_string_buffer(self._blob_ref, len(self._blob_ref))
        self.program_blob = C.cast(self._blob_buf, C.c_void_p).value
        self.program_blob_len = len(self._blob_ref)
        return self

    def copy(self) -> "PublicInputsC":
        q = PublicInputsC.from_buffer_copy(bytes(self))
        q._log_ref = getattr(self, "_log_ref", None)          # (hash_outs points into the log's buffer)
        q.with_io(getattr(self, "_in_ref", []), getattr(self, "_out_ref", []))
        if hasattr(self, "_mem_ref"):
            q.with_memory(self._mem_ref)
        return q.with_program(getattr(self, "_blob_ref", b""))


class MemcheckWitness:
    """zkir_memcheck_witness_of: the memory witness of a whole run (mode 3) — per row the accessed 8-byte cell's bytes before the access and the time of its previous
    access, and the touched cells; a sequential host replay (memory is a chain).  Refused for shards / windows, addresses of 2^40 or more, executed hash syscalls."""

    def __init__(self, log: "DeltaLog", program, mode: int = 3):
        """mode 4 (zkir_memcheck_witness_of_mode): the run's hash syscalls are replayed too and recorded as the proof's hash section (n_hash_calls of them)."""
        blob = bytes(program) if isinstance(program, (bytes, bytearray)) else program.to_bytes()
        L = lib()
        L.zkir_memcheck_witness_of_mode.restype = C.c_int
        L.zkir_memcheck_witness_of_mode.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, C.c_void_p]
        L.zkir_memcheck_witness_n_hash_calls.restype = C.c_uint64; L.zkir_memcheck_witness_n_hash_calls.argtypes = [C.c_void_p]
        L.zkir_memcheck_witness_free.restype = None; L.zkir_memcheck_witness_free.argtypes = [C.c_void_p]
        L.zkir_memcheck_witness_n_cells.restype = C.c_uint64; L.zkir_memcheck_witness_n_cells.argtypes = [C.c_void_p]
        L.zkir_memcheck_witness_n_accesses.restype = C.c_uint64; L.zkir_memcheck_witness_n_accesses.argtypes = [C.c_void_p]
        L.zkir_public_inputs_set_memory.restype = None; L.zkir_public_inputs_set_memory.argtypes = [C.c_void_p, C.c_void_p]
        h = C.c_void_p()
        rc = L.zkir_memcheck_witness_of_mode(log._h, blob, len(blob), int(mode), C.byref(h))
        if rc != ZKIR_OK:
            _raise(rc)
        self._h = h
        self.n_hash_calls = int(L.zkir_memcheck_witness_n_hash_calls(h))
        self.n_cells = int(L.zkir_memcheck_witness_n_cells(h))
        self.n_accesses = int(L.zkir_memcheck_witness_n_accesses(h))

    def __del__(self):
        try:
            if self._h:
                lib().zkir_memcheck_witness_free(self._h)
                self._h = None
        except Exception:
            pass


def memcheck_witness_device(trace, log: "DeltaLog", program, mode: int = 4, hash_outs: Optional[np.ndarray] = None, stream=None) -> dict:
    """zkir_memcheck_witness_device_mode: the memory witness made ON THE DEVICE (memcheck.hip), as numpy arrays — mem_old / mem_told per row, the touched cells (cell_addr,
    cell_bytes, cell_time) and, in mode 4, the proof's hash section (hash_section; [0] for mode 3).  trace: the device columns of the whole run (a TraceColumnsC or an object
    with one as `.c` / `.columns`); hash_outs: the records to use instead of the log's."""
    blob = bytes(program) if isinstance(program, (bytes, bytearray)) else program.to_bytes()
    cols = trace if isinstance(trace, TraceColumnsC) else getattr(trace, "c", None) or trace.columns
    n = int(log.n_rows)
    outs = np.ascontiguousarray(log.hash_outs if hash_outs is None else hash_outs, dtype=HASH_OUT_DTYPE)
    cap, wcap = n + 4096, 1 + 48 * len(outs) + 4096           # a first guess; the call reports the counts when they exceed it, and is repeated with them
    while True:
        old, told = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        ca, cb, ct = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint32)
        hs = np.zeros(wcap, np.uint32)
        nc, nw = C.c_uint64(0), C.c_uint64(0)
        rc = lib().zkir_memcheck_witness_device_mode(C.byref(cols), n, blob, len(blob), int(mode), outs.ctypes.data if len(outs) else None, len(outs), old.ctypes.data, told.ctypes.data,
                                                     ca.ctypes.data, cb.ctypes.data, ct.ctypes.data, cap, C.byref(nc), hs.ctypes.data, wcap, C.byref(nw), stream)
        if rc == ERR_ARGUMENT and (nc.value > cap or nw.value > wcap):
            cap, wcap = max(cap, int(nc.value)), max(wcap, int(nw.value))
            continue
        if rc != ZKIR_OK:
            _raise(rc)
        break
    k = int(nc.value)
    return {"mem_old": old, "mem_told": told, "cell_addr": ca[:k], "cell_bytes": cb[:k], "cell_time": ct[:k], "hash_section": hs[:max(1, int(nw.value))]}


def tape_table_side(hash_section, new_bytes, wide_section, alpha, lam, device: bool = True, stream=None) -> dict:
    """zkir_tape_table_side_launch / _host: (mode 4) the hash tape's and the wide tape's share of the lookup table side.  hash_section: a hash section in the proof's layout;
    new_bytes: per touched cell, in the section's order, the cell's bytes after its call; wide_section: [n] + 8 words per record, any record order; alpha, lam: canonical E4
    (four words each).  Returns {"sum": [4], "hh": [n_calls, 4], "ww": [n_records, 4]}, canonical words.  device=False: the host form."""
    hs = np.ascontiguousarray(hash_section if hash_section is not None and len(hash_section) else [0], dtype=np.uint32)
    ws = np.ascontiguousarray(wide_section if wide_section is not None and len(wide_section) else [0], dtype=np.uint32)
    nb = np.ascontiguousarray(new_bytes if new_bytes is not None else [], dtype=np.uint64)
    a, l = np.ascontiguousarray(alpha, dtype=np.uint32), np.ascontiguousarray(lam, dtype=np.uint32)
    if a.shape != (4,) or l.shape != (4,):
        raise ValueError("alpha and lam are four words each")
    n_calls, q, cells = int(hs[0]), 1, 0                          # the arrays the call writes are sized by the sections' own counts: walked here, checked by the call
    for _ in range(n_calls):
        if q + 8 > len(hs):
            raise ValueError("the hash section is truncated")
        k = int(hs[q + 7]); cells += k; q += 8 + 5 * k
    if q != len(hs) or cells != len(nb):
        raise ValueError(f"the hash section has {len(hs)} words and states {cells} touched cells in {q} words; new_bytes has {len(nb)} entries")
    if len(ws) != 1 + 8 * int(ws[0]):
        raise ValueError("the wide section is [n] + 8 words per record")
    out = {"sum": np.zeros(4, np.uint32), "hh": np.zeros((n_calls, 4), np.uint32), "ww": np.zeros((int(ws[0]), 4), np.uint32)}
    args = [hs.ctypes.data, len(hs), nb.ctypes.data if len(nb) else None, ws.ctypes.data, len(ws), a.ctypes.data, l.ctypes.data, out["sum"].ctypes.data,
            out["hh"].ctypes.data if n_calls else None, out["ww"].ctypes.data if int(ws[0]) else None]
    rc = lib().zkir_tape_table_side_launch(*args, stream) if device else lib().zkir_tape_table_side_host(*args)
    if rc != ZKIR_OK:
        _raise(rc)
    return out


def hash_tape_new_bytes(hash_section, device: bool = True, stream=None) -> np.ndarray:
    """zkir_hash_tape_new_bytes_launch / _host: per touched cell of a hash section, in the section's order, the cell's bytes AFTER its call — the message rebuilt from the
    old bytes, hashed (SHA-256 / Keccak-256 / BLAKE3), the 32 output bytes laid over the old ones.  device=False: hashcall::new_bytes on the host."""
    hs = np.ascontiguousarray(hash_section if hash_section is not None and len(hash_section) else [0], dtype=np.uint32)
    n_calls, q, cells = int(hs[0]), 1, 0                          # the output is sized by the section's own counts: walked here, checked by the call
    for _ in range(n_calls):
        if q + 8 > len(hs):
            break
        k = int(hs[q + 7]); cells += k; q += 8 + 5 * k
    out = np.zeros(min(cells, len(hs)), np.uint64)
    args = [hs.ctypes.data, len(hs), out.ctypes.data if len(out) else None]
    rc = lib().zkir_hash_tape_new_bytes_launch(*args, stream) if device else lib().zkir_hash_tape_new_bytes_host(*args)
    if rc != ZKIR_OK:
        _raise(rc)
    return out


def hash_tape_check(hash_section, n_real: int, code_end: int, device: bool = True, stream=None) -> int:
    """zkir_hash_tape_check_launch / _host: hashcall::parse_section's checks of a hash section — 0 well-formed, 4 truncated, 55 a call's output on code bytes, 56 a malformed
    record; of the lowest failing record.  device=False: parse_section itself."""
    hs = np.ascontiguousarray(hash_section, dtype=np.uint32)
    code = C.c_int(-1)
    if device:
        rc = lib().zkir_hash_tape_check_launch(hs.ctypes.data if len(hs) else None, len(hs), int(n_real), int(code_end), C.byref(code), stream)
    else:
        rc = lib().zkir_hash_tape_check_host(hs.ctypes.data if len(hs) else None, len(hs), int(n_real), int(code_end), C.byref(code))
    if rc != ZKIR_OK:
        _raise(rc)
    return int(code.value)


class MemoryWitnessC(C.Structure):            # zkir_memory_witness
    _fields_ = [("n_ops", C.c_uint64), ("n_rows", C.c_uint64), ("row_order", MemopColumnsC), ("row_offsets", C.c_void_p), ("sorted", MemopColumnsC)]


class RangeCheckWitnessC(C.Structure):        # zkir_range_check_witness
    _fields_ = [("n_checks", C.c_uint64), ("n_witnesses", C.c_uint64), ("witness_offsets", C.c_void_p), ("witness_cycles", C.c_void_p),
                ("value", C.c_void_p), ("pc", C.c_void_p), ("chunks", C.c_void_p), ("chunk_stride", C.c_uint64), ("chunk_bits", C.c_uint32),
                ("multiplicity", C.c_void_p)]


class NormalizationWitnessC(C.Structure):     # zkir_normalization_witness
    _fields_ = [("n_events", C.c_uint64), ("columns", NormColumnsC)]


class Sha256WitnessC(C.Structure):            # zkir_sha256_witness
    _fields_ = [("n_blocks", C.c_uint64), ("columns", C.c_void_p), ("stride", C.c_uint64), ("timestamps", C.c_void_p)]


_lib = None


def lib() -> C.CDLL:
    """Load libzkir_amd.so; fails loudly if it has not been built (python -m zkir_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise ImportError(f"{_SO} is missing: build it with `python zkir_amd/build.py` (hipcc --offload-arch=gfx950). "
                          "zkir_amd has no pure-Python or CPU fallback.")
    # One HIP runtime per process: PyTorch ships its own libamdhip64.so (soname libamdhip64.so.7, same as
    # /opt/rocm's).  Importing torch first makes the loader resolve our DT_NEEDED to that already-loaded copy;
    # loading ours first would give the process two runtimes, and whichever touches the device second fails.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(_SO)
    L.zkir_last_error.restype = C.c_char_p
    L.zkir_version.restype = C.c_char_p
    L.zkir_interpret.restype = C.c_int
    L.zkir_interpret.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(VmConfigC), C.c_uint32,
                                 C.POINTER(C.c_void_p)]
    L.zkir_delta_log_free.argtypes = [C.c_void_p]
    L.zkir_delta_log_free.restype = None
    for name, res in [("cycles", C.c_uint64), ("halt_kind", C.c_int), ("halt_code", C.c_uint64), ("n_outputs", C.c_size_t),
                      ("outputs", C.c_void_p), ("n_rows", C.c_uint64), ("tile_rows", C.c_uint32), ("pc", C.c_void_p),
                      ("inst", C.c_void_p), ("n_reg_events", C.c_size_t), ("reg_events", C.c_void_p), ("n_tiles", C.c_size_t),
                      ("tile_ev_off", C.c_void_p), ("tile_snap", C.c_void_p), ("n_mem_events", C.c_size_t),
                      ("mem_events", C.c_void_p), ("n_rc_events", C.c_size_t), ("rc_events", C.c_void_p),
                      ("n_rc_witnesses", C.c_size_t), ("rc_offsets", C.c_void_p), ("rc_cycles", C.c_void_p), ("rc_chunk_bits", C.c_uint32),
                      ("n_norm_events", C.c_size_t), ("norm_events", C.c_void_p), ("n_sha_blocks", C.c_size_t),
                      ("sha_blocks", C.c_void_p), ("n_hash_outs", C.c_size_t), ("hash_outs", C.c_void_p)]:
        f = getattr(L, "zkir_delta_log_" + name)
        f.restype = res
        f.argtypes = [C.c_void_p]
    L.zkir_delta_log_shard.restype = C.c_int
    L.zkir_delta_log_shard.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]
    L.zkir_delta_log_cycle_base.restype = C.c_uint64
    L.zkir_delta_log_cycle_base.argtypes = [C.c_void_p]
    L.zkir_delta_log_window_open.restype = C.c_int
    L.zkir_delta_log_window_open.argtypes = [C.c_void_p]
    L.zkir_interpret_window.restype = C.c_int
    L.zkir_interpret_window.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(VmConfigC), C.c_uint32, C.c_uint64, C.c_uint64,
                                        C.POINTER(C.c_void_p)]
    L.zkir_exec_window.restype = C.c_int
    L.zkir_exec_window.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(VmConfigC), C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]
    L.zkir_exec_shard.restype = C.c_int
    L.zkir_exec_shard.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]
    L.zkir_trace_fill_launch.restype = C.c_int
    L.zkir_trace_fill_launch.argtypes = [C.POINTER(TraceFillArgsC), C.c_void_p]
    L.zkir_trace_fill_bytes.restype = C.c_uint64
    L.zkir_trace_fill_bytes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    V, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    for name, args in [("zkir_memops_expand_launch", [V, U64, U64, C.POINTER(MemopColumnsC), V]),
                       ("zkir_memops_row_offsets_launch", [V, U64, U64, V, V]),
                       ("zkir_memops_expand_csr_launch", [V, U64, U64, U64, C.POINTER(MemopColumnsC), V, V, V]),
                       ("zkir_memops_sort_prepared_launch", [V, U64, U64, V, V, C.POINTER(MemopColumnsC), V]),
                       ("zkir_memops_sort_launch", [V, U64, U64, U64, V, V, C.POINTER(MemopColumnsC), V]),
                       ("zkir_range_check_expand_launch", [V, U64, U32, V, V, V, U64, V, V]),
                       ("zkir_norm_expand_launch", [V, U64, C.POINTER(NormColumnsC), V]),
                       ("zkir_sha256_chip_launch", [V, U64, V, U64, V, V])]:
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = args
    L.zkir_stark_ctx_create.restype = C.c_int
    L.zkir_stark_ctx_create.argtypes = [U32, U32, C.POINTER(V)]
    if hasattr(L, "zkir_stark_ctx_log_blowup"):               # absent from older builds loaded through ZKIR_AMD_LIB (kernel experiments)
        L.zkir_stark_ctx_log_blowup.restype = U32; L.zkir_stark_ctx_log_blowup.argtypes = [V]
    L.zkir_stark_ctx_free.restype = None
    L.zkir_stark_ctx_free.argtypes = [V]
    L.zkir_main_trace_width.restype = U32
    if hasattr(L, "zkir_main_trace_width_for"):               # absent from older builds loaded through ZKIR_AMD_LIB (kernel experiments)
        L.zkir_main_trace_width_for.restype = U32; L.zkir_main_trace_width_for.argtypes = [U32]
    L.zkir_modmul_peak_per_s.restype = C.c_double
    L.zkir_modmul_peak_per_s.argtypes = [V]
    L.zkir_padded_log_n.restype = U32
    L.zkir_padded_log_n.argtypes = [U64]
    for name, args in [("zkir_main_trace_launch", [C.POINTER(TraceColumnsC), U64, U32, V, V]), ("zkir_lde_launch", [V, V, U32, V, V]),
                       ("zkir_merkle_commit_launch", [V, V, U32, U64, V, V]), ("zkir_merkle_leaves_launch", [V, V, U32, U64, V, V]),
                       ("zkir_merkle_cap_launch", [V, V, U64, V])]:
        f = getattr(L, name)
        f.restype = C.c_int
        f.argtypes = args
    L.zkir_prove.restype = C.c_int
    L.zkir_prove.argtypes = [V, C.POINTER(TraceColumnsC), C.POINTER(PublicInputsC), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(U64), C.POINTER(C.c_float), V]
    L.zkir_verify.restype = C.c_int
    L.zkir_verify.argtypes = [V, U64, C.POINTER(PublicInputsC)]
    L.zkir_verify_segment.restype = C.c_int
    L.zkir_verify_segment.argtypes = [V, U64, C.POINTER(PublicInputsC), V, V]
    L.zkir_verify_chain.restype = C.c_int
    L.zkir_verify_chain.argtypes = [V, V, C.c_uint32, C.POINTER(PublicInputsC)]
    L.zkir_proof_state_words.restype = C.c_uint32
    L.zkir_digest_bytes.restype = None
    L.zkir_digest_bytes.argtypes = [C.c_char_p, C.c_size_t, V]
    L.zkir_public_inputs_of.restype = C.c_int
    L.zkir_public_inputs_of.argtypes = [V, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t, U32, C.POINTER(PublicInputsC)]
    L.zkir_proof_version.restype = U32
    L.zkir_abi_version.restype = U32
    L.zkir_public_inputs_size.restype = U64
    L.zkir_hash_call_cells_host.restype = U64
    L.zkir_hash_call_cells_host.argtypes = [U64, U64, U64, U32, U64, C.POINTER(U64)]
    L.zkir_memcheck_witness_device_mode.restype = C.c_int
    L.zkir_memcheck_witness_device_mode.argtypes = [C.POINTER(TraceColumnsC), U64, C.c_char_p, C.c_size_t, U32, V, U64, V, V, V, V, V, U64, C.POINTER(U64), V, U64, C.POINTER(U64), V]
    if hasattr(L, "zkir_tape_table_side_launch"):             # absent from older builds loaded through ZKIR_AMD_LIB (kernel experiments)
        L.zkir_tape_table_side_launch.restype = C.c_int; L.zkir_tape_table_side_launch.argtypes = [V, U64, V, V, U64, V, V, V, V, V, V]
        L.zkir_tape_table_side_host.restype = C.c_int; L.zkir_tape_table_side_host.argtypes = [V, U64, V, V, U64, V, V, V, V, V]
        L.zkir_hash_tape_check_launch.restype = C.c_int; L.zkir_hash_tape_check_launch.argtypes = [V, U64, U64, U64, C.POINTER(C.c_int), V]
        L.zkir_hash_tape_check_host.restype = C.c_int; L.zkir_hash_tape_check_host.argtypes = [V, U64, U64, U64, C.POINTER(C.c_int)]
    if hasattr(L, "zkir_verify_device"):
        L.zkir_hash_tape_new_bytes_launch.restype = C.c_int; L.zkir_hash_tape_new_bytes_launch.argtypes = [V, U64, V, V]
        L.zkir_hash_tape_new_bytes_host.restype = C.c_int; L.zkir_hash_tape_new_bytes_host.argtypes = [V, U64, V]
        L.zkir_verify_device.restype = C.c_int; L.zkir_verify_device.argtypes = [V, U64, C.POINTER(PublicInputsC), V]
        L.zkir_verify_last_stages.restype = C.c_int; L.zkir_verify_last_stages.argtypes = [V, C.POINTER(C.c_uint32)]
    if hasattr(L, "zkir_verify_memory_device"):               # absent from older builds loaded through ZKIR_AMD_LIB (kernel experiments)
        L.zkir_verify_memory_device.restype = C.c_int; L.zkir_verify_memory_device.argtypes = [V, U64, C.POINTER(PublicInputsC), C.c_int, V]
        L.zkir_verify_rate_memory_device.restype = C.c_int; L.zkir_verify_rate_memory_device.argtypes = [V, U64, C.POINTER(PublicInputsC), U32, U32, V]
        L.zkir_verify_memory_last.restype = C.c_int; L.zkir_verify_memory_last.argtypes = [C.POINTER(U64), C.POINTER(U32), C.POINTER(U64)]
        L.zkir_mem_section_check_host.restype = C.c_int; L.zkir_mem_section_check_host.argtypes = [V, U64, U32, U64, C.POINTER(C.c_int32)]
        L.zkir_mem_section_check_launch.restype = C.c_int; L.zkir_mem_section_check_launch.argtypes = [V, U64, U32, U64, C.POINTER(C.c_int32), V]
        L.zkir_mem_table_side_host.restype = C.c_int; L.zkir_mem_table_side_host.argtypes = [V, U64, C.c_char_p, C.c_size_t, V, V, V]
        L.zkir_mem_table_side_launch.restype = C.c_int; L.zkir_mem_table_side_launch.argtypes = [V, U64, C.c_char_p, C.c_size_t, V, V, V, V]
    if hasattr(L, "zkir_verify_many_memory_device"):          # absent from older builds loaded through ZKIR_AMD_LIB (kernel experiments)
        L.zkir_verify_many_memory_device.restype = C.c_int; L.zkir_verify_many_memory_device.argtypes = [V, V, V, C.c_uint32, V, V]
        L.zkir_verify_many_memory_host.restype = C.c_int; L.zkir_verify_many_memory_host.argtypes = [V, V, V, C.c_uint32, V]
        L.zkir_verify_many_memory_probe.restype = C.c_int; L.zkir_verify_many_memory_probe.argtypes = [V, V, V, C.c_uint32, V, C.c_uint32, C.c_uint32, C.c_int, V]
        L.zkir_verify_rate_many_memory_device.restype = C.c_int; L.zkir_verify_rate_many_memory_device.argtypes = [V, V, V, V, V, U32, V, V]
        L.zkir_verify_rate_many_memory_host.restype = C.c_int; L.zkir_verify_rate_many_memory_host.argtypes = [V, V, V, V, V, U32, V]
        L.zkir_mem_sections_stage_host.restype = C.c_int; L.zkir_mem_sections_stage_host.argtypes = [V, V, V, V, V, V, V, V, U32, V, V, V]
        L.zkir_mem_sections_stage_launch.restype = C.c_int; L.zkir_mem_sections_stage_launch.argtypes = [V, V, V, V, V, V, V, V, U32, V, V, V, V]
    if hasattr(L, "zkir_verify_many_tapes_device"):           # likewise
        L.zkir_verify_many_tapes_device.restype = C.c_int; L.zkir_verify_many_tapes_device.argtypes = [V, V, V, C.c_uint32, V, V]
        L.zkir_verify_many_tapes_host.restype = C.c_int; L.zkir_verify_many_tapes_host.argtypes = [V, V, V, C.c_uint32, V]
        L.zkir_verify_many_tapes_probe.restype = C.c_int; L.zkir_verify_many_tapes_probe.argtypes = [V, V, V, C.c_uint32, V, C.c_uint32, C.c_uint32, C.c_int, V]
        L.zkir_verify_rate_many_tapes_device.restype = C.c_int; L.zkir_verify_rate_many_tapes_device.argtypes = [V, V, V, V, V, U32, V, V]
        L.zkir_verify_rate_many_tapes_host.restype = C.c_int; L.zkir_verify_rate_many_tapes_host.argtypes = [V, V, V, V, V, U32, V]
        L.zkir_tape_sections_stage_host.restype = C.c_int; L.zkir_tape_sections_stage_host.argtypes = [V, V, V, V, V, V, V, V, U32, V, V, V, V]
        L.zkir_tape_sections_stage_launch.restype = C.c_int; L.zkir_tape_sections_stage_launch.argtypes = [V, V, V, V, V, V, V, V, U32, V, V, V, V, V]
        L.zkir_verify_tapes_last.restype = C.c_int; L.zkir_verify_tapes_last.argtypes = [V, V, V]
    if hasattr(L, "zkir_verify_on_device"):                   # absent from older builds loaded through ZKIR_AMD_LIB (kernel experiments)
        L.zkir_verify_on_device.restype = C.c_int; L.zkir_verify_on_device.argtypes = [V, U64, C.POINTER(PublicInputsC), V]
        L.zkir_verify_many_on_device.restype = C.c_int; L.zkir_verify_many_on_device.argtypes = [V, V, V, C.c_uint32, V, V]
        L.zkir_verify_chain_on_device.restype = C.c_int; L.zkir_verify_chain_on_device.argtypes = [V, V, C.c_uint32, C.POINTER(PublicInputsC), V]
        L.zkir_verify_queries_last.restype = C.c_int; L.zkir_verify_queries_last.argtypes = [C.POINTER(U64), C.POINTER(U64), C.POINTER(C.c_uint32), C.POINTER(U64)]
        L.zkir_verify_queries_last_stage_ms.restype = C.c_int; L.zkir_verify_queries_last_stage_ms.argtypes = [V]
        L.zkir_stark_query_stage_probe.restype = C.c_int; L.zkir_stark_query_stage_probe.argtypes = [V, U64, C.c_uint32, C.c_uint32, C.c_int, V]
    if hasattr(L, "zkir_lowdeg_verify_device"):               # absent from older builds loaded through ZKIR_AMD_LIB (kernel experiments)
        L.zkir_lowdeg_verify_device.restype = C.c_int; L.zkir_lowdeg_verify_device.argtypes = [V, U64, V, V]
        L.zkir_eval_verify_device.restype = C.c_int; L.zkir_eval_verify_device.argtypes = [V, U64, V, V, V, V]
        L.zkir_batch_eval_verify_device.restype = C.c_int; L.zkir_batch_eval_verify_device.argtypes = [V, U64, V, V, V, V]
        L.zkir_mixed_eval_verify_device.restype = C.c_int; L.zkir_mixed_eval_verify_device.argtypes = [V, U64, V, V, V, V]
        L.zkir_pcs_verify_last_jobs.restype = C.c_int; L.zkir_pcs_verify_last_jobs.argtypes = [C.POINTER(U64), C.POINTER(U64)]
        L.zkir_pcs_verify_last_stage_ms.restype = C.c_int; L.zkir_pcs_verify_last_stage_ms.argtypes = [V]
    if hasattr(L, "zkir_merkle_open_launch"):                 # absent from older builds loaded through ZKIR_AMD_LIB (kernel experiments)
        L.zkir_merkle_opening_words.restype = U64; L.zkir_merkle_opening_words.argtypes = [U32, U64, U32]
        L.zkir_merkle_open_launch.restype = C.c_int; L.zkir_merkle_open_launch.argtypes = [V, V, U32, U64, V, V, U64, V, V]
        L.zkir_merkle_verify_launch.restype = C.c_int; L.zkir_merkle_verify_launch.argtypes = [V, V, U32, U64, V, U64, V, U32, V, V, V]
        L.zkir_merkle_verify_host.restype = C.c_int; L.zkir_merkle_verify_host.argtypes = [V, U32, U64, V, U64, V, U32, V, V]
    if hasattr(L, "zkir_lowdeg_prove"):                       # absent from older builds loaded through ZKIR_AMD_LIB (kernel experiments)
        L.zkir_lowdeg_proof_words.restype = U64; L.zkir_lowdeg_proof_words.argtypes = [U32, U32, U32, U32]
        L.zkir_lowdeg_prove.restype = C.c_int; L.zkir_lowdeg_prove.argtypes = [V, V, U32, V, U32, U32, V, U64, C.POINTER(U64), V]
        L.zkir_lowdeg_verify.restype = C.c_int; L.zkir_lowdeg_verify.argtypes = [V, U64, V]
        L.zkir_lowdeg_prove_stages.restype = C.c_int; L.zkir_lowdeg_prove_stages.argtypes = [V, V, U32, V, U32, U32, V, U64, C.POINTER(U64), V, V]
        L.zkir_lowdeg_combine_launch.restype = C.c_int; L.zkir_lowdeg_combine_launch.argtypes = [V, V, U32, V, V, V, V]
    if hasattr(L, "zkir_eval_prove"):                         # absent from older builds loaded through ZKIR_AMD_LIB (kernel experiments)
        L.zkir_eval_proof_words.restype = U64; L.zkir_eval_proof_words.argtypes = [U32, U32, U32, U32, U32]
        L.zkir_eval_prove.restype = C.c_int; L.zkir_eval_prove.argtypes = [V, V, U32, V, V, U32, U32, U32, V, U64, C.POINTER(U64), V]
        L.zkir_eval_verify.restype = C.c_int; L.zkir_eval_verify.argtypes = [V, U64, V, V, V]
        L.zkir_eval_prove_stages.restype = C.c_int; L.zkir_eval_prove_stages.argtypes = [V, V, U32, V, V, U32, U32, U32, V, U64, C.POINTER(U64), V, V]
        L.zkir_eval_at_scratch_words.restype = U64; L.zkir_eval_at_scratch_words.argtypes = [U32, U32, U32]
        L.zkir_eval_at_launch.restype = C.c_int; L.zkir_eval_at_launch.argtypes = [V, V, U32, V, U32, V, V, V]
        L.zkir_eval_quotient_scratch_words.restype = U64; L.zkir_eval_quotient_scratch_words.argtypes = [U32, U32, U32]
        L.zkir_eval_quotient_launch.restype = C.c_int; L.zkir_eval_quotient_launch.argtypes = [V, V, U32, V, V, U32, V, V, V, V]
    if hasattr(L, "zkir_batch_eval_prove"):                   # absent from older builds loaded through ZKIR_AMD_LIB (kernel experiments)
        L.zkir_batch_eval_proof_words.restype = U64; L.zkir_batch_eval_proof_words.argtypes = [U32, U32, U32, V, V, U32, U32]
        L.zkir_batch_eval_prove.restype = C.c_int; L.zkir_batch_eval_prove.argtypes = [V, U32, V, V, V, V, V, U32, U32, U32, V, U64, C.POINTER(U64), V]
        L.zkir_batch_eval_verify.restype = C.c_int; L.zkir_batch_eval_verify.argtypes = [V, U64, V, V, V]
        L.zkir_batch_eval_prove_stages.restype = C.c_int; L.zkir_batch_eval_prove_stages.argtypes = [V, U32, V, V, V, V, V, U32, U32, U32, V, U64, C.POINTER(U64), V, V]
        L.zkir_batch_eval_quotient_scratch_words.restype = U64; L.zkir_batch_eval_quotient_scratch_words.argtypes = [U32, U32, V, U32]
        L.zkir_batch_eval_quotient_launch.restype = C.c_int; L.zkir_batch_eval_quotient_launch.argtypes = [V, U32, V, V, V, V, V, U32, V, V, V, V]
    if hasattr(L, "zkir_mixed_eval_prove"):                   # absent from older builds loaded through ZKIR_AMD_LIB (kernel experiments)
        L.zkir_mixed_eval_proof_words.restype = U64; L.zkir_mixed_eval_proof_words.argtypes = [U32, U32, V, V, V, V, V, U32]
        L.zkir_mixed_eval_prove.restype = C.c_int; L.zkir_mixed_eval_prove.argtypes = [V, U32, V, V, V, V, V, V, V, U32, U32, V, U64, C.POINTER(U64), V]
        L.zkir_mixed_eval_verify.restype = C.c_int; L.zkir_mixed_eval_verify.argtypes = [V, U64, V, V, V]
        L.zkir_mixed_eval_prove_stages.restype = C.c_int; L.zkir_mixed_eval_prove_stages.argtypes = [V, U32, V, V, V, V, V, V, V, U32, U32, V, U64, C.POINTER(U64), V, V]
        L.zkir_fri_fold_launch.restype = C.c_int; L.zkir_fri_fold_launch.argtypes = [V, V, U32, U32, V, V, V, V]
    if hasattr(L, "zkir_prove_rate"):                         # absent from older builds loaded through ZKIR_AMD_LIB (kernel experiments)
        L.zkir_prove_rate.restype = C.c_int
        L.zkir_prove_rate.argtypes = [V, C.POINTER(TraceColumnsC), C.POINTER(PublicInputsC), U32, U32, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(U64), C.POINTER(C.c_float), V]
        L.zkir_verify_rate.restype = C.c_int; L.zkir_verify_rate.argtypes = [V, U64, C.POINTER(PublicInputsC), U32, U32]
        L.zkir_verify_rate_device.restype = C.c_int; L.zkir_verify_rate_device.argtypes = [V, U64, C.POINTER(PublicInputsC), U32, U32, V]
        L.zkir_prove_rate_last_matrices.restype = C.c_int; L.zkir_prove_rate_last_matrices.argtypes = [V, V, V, V, V, C.POINTER(U64)]
    if hasattr(L, "zkir_prove_rate_modes"):
        L.zkir_prove_rate_modes.restype = C.c_int; L.zkir_prove_rate_modes.argtypes = L.zkir_prove_rate.argtypes
        L.zkir_prove_result_rate.restype = C.c_int
        L.zkir_prove_result_rate.argtypes = [V, C.POINTER(ProverParamsC), U32, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
    if hasattr(L, "zkir_prove_rate_segment"):                 # absent from older builds loaded through ZKIR_AMD_LIB (kernel experiments)
        L.zkir_prove_rate_segment.restype = C.c_int; L.zkir_prove_rate_segment.argtypes = L.zkir_prove_rate.argtypes
        L.zkir_verify_rate_segment.restype = C.c_int; L.zkir_verify_rate_segment.argtypes = [V, U64, C.POINTER(PublicInputsC), U32, U32, V, V]
        L.zkir_verify_rate_chain.restype = C.c_int; L.zkir_verify_rate_chain.argtypes = [V, V, U32, C.POINTER(PublicInputsC), U32, U32]
        L.zkir_verify_rate_segment_device.restype = C.c_int; L.zkir_verify_rate_segment_device.argtypes = [V, U64, C.POINTER(PublicInputsC), U32, U32, V, V, V]
        L.zkir_verify_rate_chain_device.restype = C.c_int; L.zkir_verify_rate_chain_device.argtypes = [V, V, U32, C.POINTER(PublicInputsC), U32, U32, V]
        L.zkir_verify_rate_many_device.restype = C.c_int; L.zkir_verify_rate_many_device.argtypes = [V, V, V, V, V, U32, V, V]
        L.zkir_pcs_verify_many_device.restype = C.c_int; L.zkir_pcs_verify_many_device.argtypes = [V, V, V, V, V, V, U32, V, V]
    L.zkir_prove_result.restype = C.c_int
    L.zkir_prove_result.argtypes = [V, C.POINTER(ProverParamsC), C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
    L.zkir_proof_bytes_free.restype = None
    L.zkir_proof_bytes_free.argtypes = [C.POINTER(C.c_uint8)]
    L.zkir_proof_free.restype = None
    L.zkir_proof_free.argtypes = [C.POINTER(C.c_uint32)]
    L.zkir_proof_num_queries.restype = U32
    L.zkir_poseidon2_permute.restype = None; L.zkir_poseidon2_permute.argtypes = [C.c_void_p]
    L.zkir_poseidon2_permute_scaled.restype = None; L.zkir_poseidon2_permute_scaled.argtypes = [C.c_void_p, C.c_uint32]
    if hasattr(L, "zkir_poseidon2_scaled_quads"):               # (a library built from older sources, selected with ZKIR_AMD_LIB to time against, has neither)
        L.zkir_poseidon2_scaled_quads.restype = None; L.zkir_poseidon2_scaled_quads.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.zkir_poseidon2_sponge_full_blocks.restype = C.c_int; L.zkir_poseidon2_sponge_full_blocks.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.zkir_exec.restype = C.c_int
    L.zkir_exec.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(VmConfigC), C.POINTER(C.c_void_p)]
    L.zkir_result_free.argtypes = [C.c_void_p]
    L.zkir_result_free.restype = None
    L.zkir_result_delta_log.restype = C.c_void_p
    L.zkir_result_delta_log.argtypes = [C.c_void_p]
    L.zkir_result_trace.restype = C.POINTER(TraceColumnsC)
    L.zkir_result_trace.argtypes = [C.c_void_p]
    L.zkir_result_stage_ms.restype = None
    L.zkir_result_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.zkir_result_copy_column.restype = C.c_int
    L.zkir_result_copy_column.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    for name, st in [("memory_trace", MemoryWitnessC), ("range_check_witnesses", RangeCheckWitnessC),
                     ("normalization_witnesses", NormalizationWitnessC), ("sha256_witnesses", Sha256WitnessC)]:
        f = getattr(L, "zkir_result_" + name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(st)]
    L.zkir_host_to_device.restype = C.c_int
    L.zkir_host_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.zkir_device_to_host.restype = C.c_int
    L.zkir_device_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    _lib = L
    return L


def _raise(code: int):
    raise RuntimeError(code, lib().zkir_last_error().decode())


def _view(ptr, n, dtype) -> np.ndarray:
    dtype = np.dtype(dtype)
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_uint8 * (n * dtype.itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=n)


@dataclass
class VMConfig:
    """vm.rs:15-50 (same defaults)."""
    max_cycles: int = 1_000_000
    trace: bool = False
    enable_range_checking: bool = False
    enable_execution_trace: bool = False
    enable_deferred_model: bool = False

    def _c(self) -> VmConfigC:
        return VmConfigC(self.max_cycles, int(self.trace), int(self.enable_range_checking), int(self.enable_execution_trace),
                         int(self.enable_deferred_model))


@dataclass(frozen=True)
class HaltReason:
    """state.rs:8-15."""
    kind: int
    code: int = 0

    @staticmethod
    def Ebreak(): return HaltReason(HALT_EBREAK)
    @staticmethod
    def Exit(code: int): return HaltReason(HALT_EXIT, code)
    @staticmethod
    def CycleLimit(): return HaltReason(HALT_CYCLE_LIMIT)


class DeltaLog:
    """Owner of a zkir_delta_log handle with zero-copy numpy views (valid while this object lives)."""

    def __init__(self, handle: int, owned: bool = True):
        self._h, self._owned = handle, owned
        self._uploads = []                                    # events of asynchronous copies out of this log's (pinned) buffers: close() waits for them (pipeline.upload)
        L = lib()
        h = handle
        self.cycles = L.zkir_delta_log_cycles(h)
        self.halt_reason = HaltReason(L.zkir_delta_log_halt_kind(h), L.zkir_delta_log_halt_code(h) if L.zkir_delta_log_halt_kind(h) == HALT_EXIT else 0)
        self.outputs = _view(L.zkir_delta_log_outputs(h), L.zkir_delta_log_n_outputs(h), "<u8").tolist()
        self.n_rows = L.zkir_delta_log_n_rows(h)
        self.cycle_base = L.zkir_delta_log_cycle_base(h)
        self.window_open = bool(L.zkir_delta_log_window_open(h))      # a trace window that ended before the run did
        self.tile_rows = L.zkir_delta_log_tile_rows(h)
        self.pc = _view(L.zkir_delta_log_pc(h), self.n_rows, "<u8")
        self.inst = _view(L.zkir_delta_log_inst(h), self.n_rows, "<u4")
        self.reg_events = _view(L.zkir_delta_log_reg_events(h), L.zkir_delta_log_n_reg_events(h), REG_EVENT_DTYPE)
        self.n_tiles = L.zkir_delta_log_n_tiles(h)
        self.tile_ev_off = _view(L.zkir_delta_log_tile_ev_off(h), self.n_tiles + 1 if self.n_rows else 0, "<u4")
        self.tile_snap = _view(L.zkir_delta_log_tile_snap(h), self.n_tiles * 16, "<u4").reshape(-1, 16)
        self.mem_events = _view(L.zkir_delta_log_mem_events(h), L.zkir_delta_log_n_mem_events(h), MEM_EVENT_DTYPE)
        self.rc_events = _view(L.zkir_delta_log_rc_events(h), L.zkir_delta_log_n_rc_events(h), RC_EVENT_DTYPE)
        self.rc_offsets = _view(L.zkir_delta_log_rc_offsets(h), L.zkir_delta_log_n_rc_witnesses(h) + 1, "<u8")
        self.rc_cycles = _view(L.zkir_delta_log_rc_cycles(h), L.zkir_delta_log_n_rc_witnesses(h), "<u8")
        self.rc_chunk_bits = L.zkir_delta_log_rc_chunk_bits(h)
        self.norm_events = _view(L.zkir_delta_log_norm_events(h), L.zkir_delta_log_n_norm_events(h), NORM_EVENT_DTYPE)
        self.sha_blocks = _view(L.zkir_delta_log_sha_blocks(h), L.zkir_delta_log_n_sha_blocks(h), SHA_BLOCK_DTYPE)
        self.hash_outs = _view(L.zkir_delta_log_hash_outs(h), L.zkir_delta_log_n_hash_outs(h), HASH_OUT_DTYPE)     # what every executed hash syscall wrote (row, 32 bytes)

    def shard(self, row_begin: int, row_end: int) -> "DeltaLog":
        """zkir_delta_log_shard: self-contained delta log of rows [row_begin, row_end) (multi-GPU row sharding)."""
        out = C.c_void_p()
        rc = lib().zkir_delta_log_shard(self._h, row_begin, row_end, C.byref(out))
        if rc != ZKIR_OK:
            _raise(rc)
        return DeltaLog(out.value)

    def close(self):
        for ev in self._uploads:
            ev.synchronize()
        self._uploads = []
        if self._owned and self._h:
            lib().zkir_delta_log_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def public_inputs(log: DeltaLog, program: Program | bytes, inputs: Sequence[int] = (), deferred: bool = False, io_mode: bool = False, mem_mode: bool = False,
                  mem_witness: str = "device", num_queries: int = 0, pow_bits: int = 0, wide_mode: bool = False, hash_witness: str = "host") -> PublicInputsC:
    """zkir_public_inputs_of: what a proof of this run is bound to (row count, mode, entry pc, program digest, io digest).  io_mode = mode 2: the default VM mode
    with the I/O argument (WRITE / READ ecalls tied to the tapes, which the proof then carries).  mem_mode = mode 3: mode 2 with the memory argument (loads and stores
    constrained, every access tied to a consistent memory; the proof carries the touched cells).  mem_witness = "device": zkir_prove computes the run's memory witness on the
    GPU (memcheck.hip: address-major sort + segmented scan); "host": it is computed here by the host's sequential replay (zkir_memcheck_witness_of — the independent
    implementation; needs no device) and handed to zkir_prove.  num_queries / pow_bits: the prover's FRI parameters (zkir_prover_params; 0 = the defaults, 50 + 12).
    wide_mode = mode 4 (round 6): mode 3 with MULH / DIVU / REMU / DIV / REM constrained — by a chunk relation on operands below 2^40, through the wide tape (a record per row, the verifier
    recomputes the result on the raw 64-bit registers) above — hash syscalls as a tape, the code segment's boundary cell: every run of the VM that stays below 2^40 in its addresses and off
    its own code has a mode-4 proof.  hash_witness (mode 4, a run that makes hash syscalls): "host" = such a run is proven from the host replay, whatever mem_witness says (the
    hash tape comes with it); "device" = the struct is left without a witness and zkir_prove builds the memory witness and the tape on the GPU (memcheck.hip), taking what
    each call wrote from the log's hash_outs records."""
    assert hash_witness in ("host", "device")
    blob = bytes(program) if isinstance(program, (bytes, bytearray)) else program.to_bytes()
    arr = (C.c_uint64 * max(1, len(inputs)))(*[int(x) & (2**64 - 1) for x in inputs])
    out = PublicInputsC()
    assert not (deferred and (io_mode or mem_mode or wide_mode)), "the I/O and memory arguments are stated for the default VM mode"
    rc = lib().zkir_public_inputs_of(log._h, blob, len(blob), arr, len(inputs), 4 if wide_mode else 3 if mem_mode else 2 if io_mode else int(deferred), C.byref(out))
    if rc != ZKIR_OK:
        _raise(rc)
    out.with_io(list(inputs), list(log.outputs))      # the C call borrowed temporaries: re-point at arrays / bytes this struct owns
    out._log_ref = log                                # (hash_outs is borrowed from the log)
    if wide_mode and mem_witness == "device" and hash_witness != "device" and log.n_rows and int(np.count_nonzero((log.inst & 0x7F) == 0x50)) > (1 if log.halt_reason.kind == HALT_EXIT else 0):
        mem_witness = "host"                          # a run that may make hash syscalls (an ECALL beside the exit) is proven from the host witness: the hash tape comes with it
    if (mem_mode or wide_mode) and mem_witness == "host":
        out.with_memory(MemcheckWitness(log, blob, 4 if wide_mode else 3))
    if num_queries or pow_bits:
        out.with_params(num_queries, pow_bits)
    return out.with_program(blob)


def verify_segment(proof: np.ndarray, expect: Optional[PublicInputsC] = None):
    """zkir_verify_segment: a SEGMENT of a run -> (code, first_state u32[68], last_state u32[68])."""
    proof = np.ascontiguousarray(proof, dtype=np.uint32)
    first, last = np.zeros(68, np.uint32), np.zeros(68, np.uint32)
    rc = lib().zkir_verify_segment(proof.ctypes.data, len(proof), C.byref(expect) if expect is not None else None, first.ctypes.data, last.ctypes.data)
    return rc, first, last


def verify_chain(proofs, expect: Optional[PublicInputsC] = None, device: bool = False, stream=None) -> int:
    """zkir_verify_chain: the segments of one run, in order; expect.n_real = the run's total executed rows.  device=True: zkir_verify_chain_on_device — the same verdict, all
    the segments' queries as one batch on the GPU (two launches on `stream`); a negative result is a device failure, not a verdict (raised)."""
    ps = [np.ascontiguousarray(p, dtype=np.uint32) for p in proofs]
    ptrs = (C.c_void_p * len(ps))(*[p.ctypes.data for p in ps])
    lens = (C.c_uint64 * len(ps))(*[len(p) for p in ps])
    if device:
        return _pcs_verdict(lib().zkir_verify_chain_on_device(ptrs, lens, len(ps), C.byref(expect) if expect is not None else None, stream))
    return lib().zkir_verify_chain(ptrs, lens, len(ps), C.byref(expect) if expect is not None else None)


def verify_many(proofs, expects=None, stream=None, memory: bool = False, device: bool = True, probe=None, tapes: bool = False):
    """zkir_verify_many_on_device: n independent proofs (1 .. 1024) -> [zkir_verify(proofs[i], expects[i]) for i] with every proof's queries in ONE batch on the GPU.
    `expects`: None, or one entry (a PublicInputsC or None) per proof.  An empty list, more than 1024 proofs or a device failure raise.
    memory=True: zkir_verify_many_memory_device — the same verdicts with the memory sections of all mode-3 / mode-4 proofs as ONE device batch (three launches for the
    whole call; verify_memory_last() reports it).  memory=True, device=False: zkir_verify_many_memory_host, the same orchestration over the host stages (no HIP call).
    probe=(what, index): zkir_verify_many_memory_probe (test hook; what = 1 adds one to proof index's cell share before its deferred check 10), host or device.
    tapes=True (implies memory=True): zkir_verify_many_tapes_device — the hash and wide tapes of all mode-4 proofs as ONE device batch too (at most 8 launches for the
    whole call; verify_tapes_last() reports it); device=False: zkir_verify_many_tapes_host.  With probe=(what, index): zkir_verify_many_tapes_probe (what = 1 adds one to
    proof index's hash share, 2 to its wide share)."""
    ps = [np.ascontiguousarray(p, dtype=np.uint32) for p in proofs]
    n = len(ps)
    if expects is not None and len(expects) != n:
        raise ValueError(f"{n} proofs, {len(expects)} expectations")
    ptrs = (C.c_void_p * max(n, 1))(*[p.ctypes.data if len(p) else None for p in ps])
    lens = (C.c_uint64 * max(n, 1))(*[len(p) for p in ps])
    exps = (C.c_void_p * max(n, 1))(*[C.addressof(e) if e is not None else None for e in expects]) if expects is not None else None
    verdicts = (C.c_int32 * max(n, 1))()
    if tapes and probe is not None:
        rc = lib().zkir_verify_many_tapes_probe(ptrs, lens, exps, n, verdicts, int(probe[0]), int(probe[1]), 1 if device else 0, stream)
    elif tapes:
        rc = lib().zkir_verify_many_tapes_device(ptrs, lens, exps, n, verdicts, stream) if device else lib().zkir_verify_many_tapes_host(ptrs, lens, exps, n, verdicts)
    elif probe is not None:
        rc = lib().zkir_verify_many_memory_probe(ptrs, lens, exps, n, verdicts, int(probe[0]), int(probe[1]), 1 if device else 0, stream)
    elif memory:
        rc = lib().zkir_verify_many_memory_device(ptrs, lens, exps, n, verdicts, stream) if device else lib().zkir_verify_many_memory_host(ptrs, lens, exps, n, verdicts)
    else:
        rc = lib().zkir_verify_many_on_device(ptrs, lens, exps, n, verdicts, stream)
    if rc != 0:
        _raise(abs(rc))
    return [int(verdicts[i]) for i in range(n)]


def verify_queries_last() -> dict:
    """zkir_verify_queries_last: the device query stage of this thread's last verification (all zero after a host entry and after verify(device=True) without queries)."""
    h, v, l, u = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    lib().zkir_verify_queries_last(C.byref(h), C.byref(v), C.byref(l), C.byref(u))
    return {"hash_jobs": int(h.value), "value_jobs": int(v.value), "launches": int(l.value), "uploaded_words": int(u.value)}


def verify_memory_last() -> dict:
    """zkir_verify_memory_last: the device memory stages of this thread's last verification — the cells whose stages ran on the GPU, their launches and the words uploaded
    for them (all zero after any entry but verify(device=True, memory=True) / verify_rate(device=True, memory=True))."""
    c, l, u = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    lib().zkir_verify_memory_last(C.byref(c), C.byref(l), C.byref(u))
    return {"cells": int(c.value), "launches": int(l.value), "uploaded_words": int(u.value)}


def verify_tapes_last() -> dict:
    """zkir_verify_tapes_last: the tape list stage of this thread's last many-proof verification — the records (hash calls plus wide records) that went through it, its
    launches and the words uploaded for it (all zero after any entry but verify_many(tapes=True) / verify_rate_many(tapes=True) / tape_sections_stage)."""
    c, l, u = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    lib().zkir_verify_tapes_last(C.byref(c), C.byref(l), C.byref(u))
    return {"records": int(c.value), "launches": int(l.value), "uploaded_words": int(u.value)}


def tape_sections_stage(hash_secs, wide_secs, n_real, code_end, alphas, lams, device: bool = True, stream=None):
    """zkir_tape_sections_stage_launch / _host: a mode-4 proof's tape stages over n pairs of whole sections (hash_secs[i]: a hash section, [0] included; wide_secs[i]:
    [n_i] + 8 n_i words) as ONE list — at most 8 launches on the GPU, or the host stage functions.  n_real[i], code_end[i], alphas[i] / lams[i] canonical E4 ->
    (hash_verdicts [int], wide_verdicts [int], digests [(np.uint32[hash chunks_i, 4], np.uint32[wide chunks_i, 4]); zero where that verdict is not 0],
    sums np.uint32[n, 2, 4] canonical: hash share, wide share; zero unless both verdicts are 0)."""
    hs = [np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in hash_secs]
    ws = [np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in wide_secs]
    n = len(hs)
    if not (len(ws) == len(n_real) == len(code_end) == len(alphas) == len(lams) == n):
        raise ValueError("one wide section, n_real, code_end, alpha and lambda per hash section")
    hp = (C.c_void_p * max(n, 1))(*[x.ctypes.data if len(x) else None for x in hs])
    hl = (C.c_uint64 * max(n, 1))(*[len(x) for x in hs])
    wp = (C.c_void_p * max(n, 1))(*[x.ctypes.data if len(x) else None for x in ws])
    wl = (C.c_uint64 * max(n, 1))(*[len(x) for x in ws])
    nr = (C.c_uint64 * max(n, 1))(*[int(x) for x in n_real])
    ce = (C.c_uint64 * max(n, 1))(*[int(x) for x in code_end])
    a = np.ascontiguousarray(np.asarray(alphas, dtype=np.uint32).reshape(-1)) if n else np.zeros(4, np.uint32)
    l = np.ascontiguousarray(np.asarray(lams, dtype=np.uint32).reshape(-1)) if n else np.zeros(4, np.uint32)
    chunks = [((len(x) + 511) // 512, (len(y) + 511) // 512) for x, y in zip(hs, ws)]
    hv, wv = (C.c_int32 * max(n, 1))(), (C.c_int32 * max(n, 1))()
    dg = np.zeros(4 * max(sum(c0 + c1 for c0, c1 in chunks), 1), dtype=np.uint32)
    sums = np.zeros((max(n, 1), 2, 4), dtype=np.uint32)
    args = [hp, hl, wp, wl, nr, ce, a.ctypes.data, l.ctypes.data, n, hv, wv, dg.ctypes.data, sums.ctypes.data]
    rc = lib().zkir_tape_sections_stage_launch(*args, stream) if device else lib().zkir_tape_sections_stage_host(*args)
    if rc != ZKIR_OK:
        _raise(abs(rc))
    out, at = [], 0
    for c0, c1 in chunks:
        out.append((dg[4 * at:4 * (at + c0)].reshape(c0, 4).copy(), dg[4 * (at + c0):4 * (at + c0 + c1)].reshape(c1, 4).copy()))
        at += c0 + c1
    return [int(hv[i]) for i in range(n)], [int(wv[i]) for i in range(n)], out, sums[:n]


def mem_section_check(sec, mode: int, code_words: int, device: bool = True, stream=None) -> int:
    """zkir_mem_section_check_launch / _host: the verifier's checks of a touched-cell section ([n] + 7 n words) — 0 well-formed, 4 shorter than its count states, 54 a
    cell out of range or not above its predecessor, 55 a cell on the code_words code words at 0x1000 (mode 4 admits the boundary cell); of the lowest failing cell."""
    s = np.ascontiguousarray(sec, dtype=np.uint32).reshape(-1)
    verdict = C.c_int32(-1)
    args = [s.ctypes.data if len(s) else None, len(s), int(mode), int(code_words), C.byref(verdict)]
    rc = lib().zkir_mem_section_check_launch(*args, stream) if device else lib().zkir_mem_section_check_host(*args)
    if rc != ZKIR_OK:
        _raise(rc)
    return int(verdict.value)


def mem_table_side(sec, blob: bytes, alpha, lam, device: bool = True, stream=None) -> np.ndarray:
    """zkir_mem_table_side_launch / _host: the touched cells' share of the lookup table side, sum over the cells of 1 / (alpha - fp(cell, 0, image bytes)) -
    1 / (alpha - fp(cell, t_last, final bytes)) -> canonical E4 (np.uint32[4]).  alpha, lam: canonical E4; blob: the program (its image bytes)."""
    s = np.ascontiguousarray(sec, dtype=np.uint32).reshape(-1)
    a, l = np.ascontiguousarray(alpha, dtype=np.uint32), np.ascontiguousarray(lam, dtype=np.uint32)
    blob = bytes(blob)
    out = np.zeros(4, dtype=np.uint32)
    args = [s.ctypes.data if len(s) else None, len(s), blob, len(blob), a.ctypes.data, l.ctypes.data, out.ctypes.data]
    rc = lib().zkir_mem_table_side_launch(*args, stream) if device else lib().zkir_mem_table_side_host(*args)
    if rc != ZKIR_OK:
        _raise(rc)
    return out


def mem_sections_stage(secs, modes, code_words, blobs, alphas, lams, device: bool = True, stream=None):
    """zkir_mem_sections_stage_launch / _host: the memory stages of n whole sections ([n_i] + 7 n_i words each) as ONE list — three launches on the GPU, or the host stage
    functions.  modes[i] 3 / 4, code_words[i], blobs[i] the program, alphas[i] / lams[i] canonical E4 -> (verdicts [int], digests [np.uint32[chunks_i, 4]; zero where
    the verdict is not 0], sums np.uint32[n, 4] canonical; zero likewise)."""
    ss = [np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in secs]
    n = len(ss)
    bs = [bytes(b) for b in blobs]
    if not (len(modes) == len(code_words) == len(bs) == len(alphas) == len(lams) == n):
        raise ValueError("one mode, code size, blob, alpha and lambda per section")
    ptrs = (C.c_void_p * max(n, 1))(*[x.ctypes.data if len(x) else None for x in ss])
    lens = (C.c_uint64 * max(n, 1))(*[len(x) for x in ss])
    md = (C.c_uint32 * max(n, 1))(*[int(m) for m in modes])
    cw = (C.c_uint64 * max(n, 1))(*[int(c) for c in code_words])
    bp = (C.c_char_p * max(n, 1))(*bs)
    bl = (C.c_size_t * max(n, 1))(*[len(b) for b in bs])
    a = np.ascontiguousarray(np.asarray(alphas, dtype=np.uint32).reshape(-1)) if n else np.zeros(4, np.uint32)
    l = np.ascontiguousarray(np.asarray(lams, dtype=np.uint32).reshape(-1)) if n else np.zeros(4, np.uint32)
    chunks = [(len(x) + 511) // 512 for x in ss]
    verdicts = (C.c_int32 * max(n, 1))()
    dg = np.zeros(4 * max(sum(chunks), 1), dtype=np.uint32)
    sums = np.zeros((max(n, 1), 4), dtype=np.uint32)
    args = [ptrs, lens, md, cw, bp, bl, a.ctypes.data, l.ctypes.data, n, verdicts, dg.ctypes.data, sums.ctypes.data]
    rc = lib().zkir_mem_sections_stage_launch(*args, stream) if device else lib().zkir_mem_sections_stage_host(*args)
    if rc != ZKIR_OK:
        _raise(abs(rc))
    out, at = [], 0
    for c in chunks:
        out.append(dg[4 * at:4 * (at + c)].reshape(c, 4).copy())
        at += c
    return [int(verdicts[i]) for i in range(n)], out, sums[:n]


def verify_queries_last_stage_ms():
    """zkir_verify_queries_last_stage_ms: (upload, kernels, download) host clocks in ms of this thread's last device query stage, measured only with
    ZKIR_VERIFY_QUERIES_TIMES set."""
    ms = (C.c_double * 3)()
    lib().zkir_verify_queries_last_stage_ms(ms)
    return float(ms[0]), float(ms[1]), float(ms[2])


def stark_query_stage_probe(proof, what: int = 0, index: int = 0, device: bool = False, stream=None) -> int:
    """zkir_stark_query_stage_probe (test hook): the verifier's host part, then its query stage on perturbed draws — what: 0 nothing, 1 a0 + 1, 2 b0 + 1, 3 zeta + 1,
    4 betas[index] + 1, 5 qs[index] ^= 1 — on the host (device=False: no HIP call) or on the GPU.  Returns the verdict; a bad `what` / `index` or a device failure raise."""
    proof = np.ascontiguousarray(proof, dtype=np.uint32)
    return _pcs_verdict(lib().zkir_stark_query_stage_probe(proof.ctypes.data if len(proof) else None, len(proof), int(what), int(index), 1 if device else 0, stream))


def _u64s(a):
    return np.ascontiguousarray(np.asarray([int(x) & (2**64 - 1) for x in a], dtype=np.uint64))


def verify_io(proof: np.ndarray, expect: Optional[PublicInputsC], inputs, outputs, halt) -> int:
    """zkir_verify_io: zkir_verify + the run's claim in the clear — `inputs`, `outputs` and `halt` (a HaltReason or (kind, code)) must hash to the proof's io digest (50) and
    the halt row must be the instruction the halt reason names (52: not that instruction; 53: not that exit code)."""
    proof, i, o = np.ascontiguousarray(proof, dtype=np.uint32), _u64s(inputs), _u64s(outputs)
    kind, code = (halt.kind, halt.code) if hasattr(halt, "kind") else halt
    L = lib()
    L.zkir_verify_io.restype = C.c_int
    L.zkir_verify_io.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_uint64]
    return L.zkir_verify_io(proof.ctypes.data, len(proof), C.byref(expect) if expect is not None else None, i.ctypes.data, len(i), o.ctypes.data, len(o), int(kind), int(code or 0))


def verify_chain_io(proofs, expect: Optional[PublicInputsC], inputs, outputs, halt) -> int:
    """zkir_verify_chain_io: the same for a run proven in segments."""
    ps = [np.ascontiguousarray(p, dtype=np.uint32) for p in proofs]
    ptrs = (C.c_void_p * len(ps))(*[p.ctypes.data for p in ps])
    lens = (C.c_uint64 * len(ps))(*[len(p) for p in ps])
    i, o = _u64s(inputs), _u64s(outputs)
    kind, code = (halt.kind, halt.code) if hasattr(halt, "kind") else halt
    L = lib()
    L.zkir_verify_chain_io.restype = C.c_int
    L.zkir_verify_chain_io.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_uint64]
    return L.zkir_verify_chain_io(ptrs, lens, len(ps), C.byref(expect) if expect is not None else None, i.ctypes.data, len(i), o.ctypes.data, len(o), int(kind), int(code or 0))


def verify(proof: np.ndarray, expect: Optional[PublicInputsC] = None, device: bool = False, stream=None, queries: bool = False, memory: bool = False) -> int:
    """zkir_verify (host only): 0 = accepted, otherwise the number of the failed check.  device=True: zkir_verify_device — the same verdict, a mode-4 proof's tape stages
    (record checks, chunk digests, the table side with every hash call's digest) on the GPU; device=True, queries=True: zkir_verify_on_device — the same verdict, any mode,
    the query stage (Merkle paths, layer-0 values, folds) on the GPU as well; device=True, memory=True: zkir_verify_memory_device — the same verdict, a mode-3 / mode-4
    proof's touched-cell stages (cell checks, chunk digests, the cells' share of the table side) on the GPU too, with or without queries=True; a negative result is a
    device failure, not a verdict (raised)."""
    proof = np.ascontiguousarray(proof, dtype=np.uint32)
    if not device:
        if queries:
            raise ValueError("queries=True needs device=True")
        if memory:
            raise ValueError("memory=True needs device=True")
        return lib().zkir_verify(proof.ctypes.data, len(proof), C.byref(expect) if expect is not None else None)
    if memory:
        rc = lib().zkir_verify_memory_device(proof.ctypes.data, len(proof), C.byref(expect) if expect is not None else None, 1 if queries else 0, stream)
        if rc < 0:
            _raise(-rc)
        return rc
    entry = lib().zkir_verify_on_device if queries else lib().zkir_verify_device
    rc = entry(proof.ctypes.data, len(proof), C.byref(expect) if expect is not None else None, stream)
    if rc < 0:
        _raise(-rc)
    return rc


OPEN_LEAF_DIGEST, VERIFY_FORM_LANE, VERIFY_FORM_ROW16 = 1, 2, 4      # zkir_amd.h: ZKIR_OPEN_LEAF_DIGEST, ZKIR_VERIFY_FORM_*


def opening_words(width: int, n_leaves: int, flags: int = 0) -> int:
    """Words of one opening record (zkir_merkle_opening_words): width + 4 log2(n_leaves), 4 + 4 log2(n_leaves) in the digest form; 0 for a bad n_leaves."""
    return int(lib().zkir_merkle_opening_words(int(width), int(n_leaves) & (2**64 - 1), int(flags)))


def merkle_verify_host(root, width: int, n_leaves: int, indices, openings, flags: int = 0):
    """zkir_merkle_verify_host: the verdicts (0 ok, 1 wrong, 2 non-canonical word, 3 index out of range) of opening records against a root, on the host — no GPU.
    Returns (verdicts np.uint32[n_idx], summary np.uint32[2] = failures, smallest failing position or 0xFFFFFFFF)."""
    root = np.ascontiguousarray(root, dtype=np.uint32)
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint64).reshape(-1))
    rec = np.ascontiguousarray(openings, dtype=np.uint32).reshape(-1)
    words = opening_words(width, n_leaves, flags)
    if words == 0 and len(idx) and n_leaves and not (n_leaves & (n_leaves - 1)):
        rec = np.zeros(1, np.uint32)                            # (a record of no words: one leaf, no columns)
    elif words:
        assert len(rec) == len(idx) * words, f"{len(idx)} records of {words} words expected, got {len(rec)} words"
    verdicts, summary = np.zeros(max(len(idx), 1), np.uint32), np.zeros(2, np.uint32)
    rc = lib().zkir_merkle_verify_host(root.ctypes.data, int(width), int(n_leaves), idx.ctypes.data if len(idx) else None, len(idx), rec.ctypes.data if len(idx) else None, int(flags),
                                       verdicts.ctypes.data, summary.ctypes.data)
    if rc != ZKIR_OK:
        _raise(rc)
    return verdicts[:len(idx)], summary


def lowdeg_proof_words(log_n: int, log_blowup: int, width: int, num_queries: int) -> int:
    """Words of a low-degree proof of a commitment (zkir_lowdeg_proof_words); 0 for parameters no proof can state."""
    return int(lib().zkir_lowdeg_proof_words(int(log_n), int(log_blowup), int(width), int(num_queries)))


def _pcs_verdict(rc: int) -> int:
    """A *_verify_device result: a negative one is a device failure, not a verdict (raised)."""
    if rc < 0:
        _raise(-rc)
    return int(rc)


def pcs_verify_last_jobs():
    """zkir_pcs_verify_last_jobs: (hash_jobs, value_jobs) this thread's last *_verify(device=True) call launched; (0, 0) when it returned before its query stage."""
    h, v = C.c_uint64(0), C.c_uint64(0)
    lib().zkir_pcs_verify_last_jobs(C.byref(h), C.byref(v))
    return int(h.value), int(v.value)


def pcs_verify_last_stage_ms():
    """zkir_pcs_verify_last_stage_ms: (upload, kernels, download) host clocks in ms of this thread's last device query stage, measured only with ZKIR_PCS_VERIFY_TIMES set."""
    ms = (C.c_double * 3)()
    lib().zkir_pcs_verify_last_stage_ms(ms)
    return float(ms[0]), float(ms[1]), float(ms[2])


def lowdeg_verify(proof, root=None, device: bool = False, stream=None) -> int:
    """zkir_lowdeg_verify, on the host — no GPU: 0 = the proof convinces a holder of its root (or of `root`, four words, when given) that every committed column is close to a
    polynomial of degree < 2^log_n; else the code of the first failing check (include/zkir_amd.h lists them).  device=True: zkir_lowdeg_verify_device — the same verdict,
    checks 7 - 11 of all queries on the GPU."""
    w = np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1)
    r = None if root is None else np.ascontiguousarray(root, dtype=np.uint32).reshape(-1)
    assert r is None or len(r) == 4
    if device:
        return _pcs_verdict(lib().zkir_lowdeg_verify_device(w.ctypes.data if len(w) else None, len(w), r.ctypes.data if r is not None else None, stream))
    return int(lib().zkir_lowdeg_verify(w.ctypes.data if len(w) else None, len(w), r.ctypes.data if r is not None else None))


def eval_proof_words(log_n: int, log_blowup: int, width: int, n_points: int, num_queries: int) -> int:
    """Words of an evaluation proof of a commitment (zkir_eval_proof_words); 0 for parameters no proof can state."""
    return int(lib().zkir_eval_proof_words(int(log_n), int(log_blowup), int(width), int(n_points), int(num_queries)))


def eval_verify(proof, root=None, points=None, evals=None, device: bool = False, stream=None) -> int:
    """zkir_eval_verify, on the host — no GPU: 0 = the proof convinces a holder of its root that every committed column is close to a polynomial of degree < 2^log_n that takes
    the proof's evaluations at the proof's points; `root` (four words), `points` ([n_points][4]) and `evals` ([n_points][width][4]), when given, must be the proof's.  Else the
    code of the first failing check (include/zkir_amd.h lists them).  The library reads as many expected words as the proof's header states: where the header is one a proof
    can have, `points` / `evals` of another size raise ValueError.  device=True: zkir_eval_verify_device — the same verdict, checks 7 - 11 of all queries on the GPU."""
    w = np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1)
    r = None if root is None else np.ascontiguousarray(root, dtype=np.uint32).reshape(-1)
    assert r is None or len(r) == 4
    p = None if points is None else np.ascontiguousarray(points, dtype=np.uint32).reshape(-1)
    e = None if evals is None else np.ascontiguousarray(evals, dtype=np.uint32).reshape(-1)
    sane = len(w) >= 9 and 1 <= int(w[4]) <= 512 and 1 <= int(w[5]) <= 2
    if sane:
        if p is not None and len(p) != 4 * int(w[5]):
            raise ValueError(f"eval_verify: points must hold {4 * int(w[5])} words, the proof's n_points x 4")
        if e is not None and len(e) != 4 * int(w[5]) * int(w[4]):
            raise ValueError(f"eval_verify: evals must hold {4 * int(w[5]) * int(w[4])} words, the proof's n_points x width x 4")
    else:
        p = e = None                                             # the proof is malformed (1) whatever is expected of it
    ptr = lambda a: a.ctypes.data if a is not None else None
    if device:
        return _pcs_verdict(lib().zkir_eval_verify_device(w.ctypes.data if len(w) else None, len(w), ptr(r), ptr(p), ptr(e), stream))
    return int(lib().zkir_eval_verify(w.ctypes.data if len(w) else None, len(w), ptr(r), ptr(p), ptr(e)))


def batch_eval_proof_words(log_n: int, log_blowup: int, widths, masks, n_points: int, num_queries: int) -> int:
    """Words of a batched evaluation proof (zkir_batch_eval_proof_words) of len(widths) matrices; 0 for a shape no proof can state."""
    ws, ks = np.ascontiguousarray(widths, dtype=np.uint32).reshape(-1), np.ascontiguousarray(masks, dtype=np.uint32).reshape(-1)
    if len(ws) != len(ks) or not 1 <= len(ws) <= 4:
        return 0
    return int(lib().zkir_batch_eval_proof_words(int(log_n), int(log_blowup), len(ws), ws.ctypes.data, ks.ctypes.data, int(n_points), int(num_queries)))


RATE_DEFAULT_QUERIES = {1: 50, 2: 25, 3: 17}                  # by log_blowup: about 100 bits from the queries at rate 2^-b, plus the grinding bits


def verify_rate(proof, expect: Optional[PublicInputsC] = None, min_queries: int = 1, min_pow_bits: int = 0, device: bool = False, stream=None, memory: bool = False) -> int:
    """zkir_verify_rate, on the host — no GPU: 0 = the 'ZKSR' proof (stark.prove_rate: a ZKIR-STARK run at the rate its header states) is accepted and states at least
    `min_queries` queries and `min_pow_bits` grinding bits; otherwise the number of the failed check (include/zkir_amd.h: zkir_verify's codes for the front — 54 - 57 in modes 3 / 4 —, 2 also for too
    few queries or bits, 5 an embedded proof of another shape, 10 the constraints at zeta, 100 + c for the embedded evaluation proof's code c).  `expect.fri_params` is not
    consulted.  device=True: zkir_verify_rate_device — the same verdict, the embedded proof's query stage on the GPU; device=True, memory=True:
    zkir_verify_rate_memory_device — a mode-3 / mode-4 proof's touched-cell stages on the GPU too; a negative result is a device failure (raised)."""
    w = np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1)
    e = C.byref(expect) if expect is not None else None
    if not device:
        if memory:
            raise ValueError("memory=True needs device=True")
        return lib().zkir_verify_rate(w.ctypes.data, len(w), e, int(min_queries), int(min_pow_bits))
    entry = lib().zkir_verify_rate_memory_device if memory else lib().zkir_verify_rate_device
    rc = entry(w.ctypes.data, len(w), e, int(min_queries), int(min_pow_bits), stream)
    if rc < 0:
        _raise(-rc)
    return rc


def verify_rate_segment(proof, expect: Optional[PublicInputsC] = None, min_queries: int = 1, min_pow_bits: int = 0, device: bool = False, stream=None):
    """zkir_verify_rate_segment: a 'ZKSR' proof of a SEGMENT of a run (stark.prove_rate_segment) -> (code, first_state u32[68], last_state u32[68]): verify_rate's codes
    without check 7; the states are the header's on acceptance (zero otherwise).  device=True: zkir_verify_rate_segment_device — the same verdict, the embedded proof's
    queries on the GPU; a negative result is a device failure (raised)."""
    w = np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1)
    e = C.byref(expect) if expect is not None else None
    first, last = np.zeros(68, np.uint32), np.zeros(68, np.uint32)
    ptr = w.ctypes.data if len(w) else None
    if device:
        rc = _pcs_verdict(lib().zkir_verify_rate_segment_device(ptr, len(w), e, int(min_queries), int(min_pow_bits), first.ctypes.data, last.ctypes.data, stream))
    else:
        rc = lib().zkir_verify_rate_segment(ptr, len(w), e, int(min_queries), int(min_pow_bits), first.ctypes.data, last.ctypes.data)
    return rc, first, last


def verify_rate_chain(proofs, expect: Optional[PublicInputsC] = None, min_queries: int = 1, min_pow_bits: int = 0, device: bool = False, stream=None) -> int:
    """zkir_verify_rate_chain: the 'ZKSR' segments of one run, in order (verify_chain's codes: 40 empty, 1000 (i + 1) + c segment i's code c, 41 - 46, 50 - 53; 43 also for
    a segment of another rate, query count or grinding than segment 0); expect.n_real = the run's total executed rows, `min_queries` / `min_pow_bits` hold for every
    segment.  device=True: zkir_verify_rate_chain_device — the same verdict, all the segments' queries as one batch on the GPU (two launches on `stream`); a negative
    result is a device failure, not a verdict (raised)."""
    ps = [np.ascontiguousarray(p, dtype=np.uint32).reshape(-1) for p in proofs]
    n = len(ps)
    ptrs = (C.c_void_p * max(n, 1))(*[p.ctypes.data if len(p) else None for p in ps])
    lens = (C.c_uint64 * max(n, 1))(*[len(p) for p in ps])
    e = C.byref(expect) if expect is not None else None
    if device:
        return _pcs_verdict(lib().zkir_verify_rate_chain_device(ptrs, lens, n, e, int(min_queries), int(min_pow_bits), stream))
    return lib().zkir_verify_rate_chain(ptrs, lens, n, e, int(min_queries), int(min_pow_bits))


def _many_args(proofs):
    ps = [np.ascontiguousarray(p, dtype=np.uint32).reshape(-1) for p in proofs]
    n = len(ps)
    ptrs = (C.c_void_p * max(n, 1))(*[p.ctypes.data if len(p) else None for p in ps])
    lens = (C.c_uint64 * max(n, 1))(*[len(p) for p in ps])
    return ps, n, ptrs, lens


def verify_rate_many(proofs, expects=None, min_queries=None, min_pow_bits=None, stream=None, memory: bool = False, device: bool = True, tapes: bool = False):
    """zkir_verify_rate_many_device: n independent whole-run 'ZKSR' proofs (1 .. 1024) of any mode and rate -> [verify_rate(proofs[i], expects[i], min_queries[i],
    min_pow_bits[i]) for i] with every proof's queries in ONE batch on the GPU.  `expects`: None, or one entry (a PublicInputsC or None) per proof; `min_queries` /
    `min_pow_bits`: None (1 / 0) or one value per proof.  An empty list, more than 1024 proofs or a device failure raise, and no verdict is formed.
    memory=True: zkir_verify_rate_many_memory_device — the memory sections of all mode-3 / mode-4 proofs as ONE device batch, as verify_many(memory=True); with
    device=False zkir_verify_rate_many_memory_host (no HIP call).  tapes=True (implies memory=True): zkir_verify_rate_many_tapes_device / _host — the mode-4 proofs'
    hash and wide tapes as ONE batch too, as verify_many(tapes=True)."""
    ps, n, ptrs, lens = _many_args(proofs)
    for name, a in (("expectations", expects), ("min_queries", min_queries), ("min_pow_bits", min_pow_bits)):
        if a is not None and len(a) != n:
            raise ValueError(f"{n} proofs, {len(a)} {name}")
    exps = (C.c_void_p * max(n, 1))(*[C.addressof(e) if e is not None else None for e in expects]) if expects is not None else None
    mq = (C.c_uint32 * max(n, 1))(*[int(x) for x in min_queries]) if min_queries is not None else None
    mb = (C.c_uint32 * max(n, 1))(*[int(x) for x in min_pow_bits]) if min_pow_bits is not None else None
    verdicts = (C.c_int32 * max(n, 1))()
    if tapes:
        rc = lib().zkir_verify_rate_many_tapes_device(ptrs, lens, exps, mq, mb, n, verdicts, stream) if device else lib().zkir_verify_rate_many_tapes_host(ptrs, lens, exps, mq, mb, n, verdicts)
    elif memory and not device:
        rc = lib().zkir_verify_rate_many_memory_host(ptrs, lens, exps, mq, mb, n, verdicts)
    elif memory:
        rc = lib().zkir_verify_rate_many_memory_device(ptrs, lens, exps, mq, mb, n, verdicts, stream)
    else:
        rc = lib().zkir_verify_rate_many_device(ptrs, lens, exps, mq, mb, n, verdicts, stream)
    if rc != 0:
        _raise(abs(rc))
    return [int(verdicts[i]) for i in range(n)]


PCS_KINDS = {"lowdeg": 0, "eval": 1, "batch_eval": 2}         # zkir_pcs_verify_many_device's kinds: 'ZKLD', 'ZKEV', 'ZKBE'


def pcs_verify_many(kinds, proofs, roots=None, points=None, evals=None, stream=None):
    """zkir_pcs_verify_many_device: n stand-alone proofs of the commitment layer (1 .. 1024) in ONE stage run on the GPU -> [lowdeg_verify / eval_verify / batch_eval_verify
    of proof i].  kinds[i]: 0 / "lowdeg" ('ZKLD'), 1 / "eval" ('ZKEV'), 2 / "batch_eval" ('ZKBE').  `roots`, `points`, `evals`: None, or one entry (an array sized as the
    proof's header states, or None) per proof.  A bad kind, an empty list, more than 1024 proofs or a device failure raise, and no verdict is formed."""
    ps, n, ptrs, lens = _many_args(proofs)
    ks = [PCS_KINDS.get(k, k) if isinstance(k, str) else int(k) for k in kinds]
    if len(ks) != n:
        raise ValueError(f"{n} proofs, {len(ks)} kinds")
    keep = []

    def table(a, name):
        if a is None:
            return None
        if len(a) != n:
            raise ValueError(f"{n} proofs, {len(a)} {name}")
        arrs = [None if x is None else np.ascontiguousarray(x, dtype=np.uint32).reshape(-1) for x in a]
        keep.append(arrs)
        return (C.c_void_p * max(n, 1))(*[x.ctypes.data if x is not None else None for x in arrs])
    r, p, e = table(roots, "roots"), table(points, "points"), table(evals, "evals")
    kinds_c = (C.c_uint32 * max(n, 1))(*[k & 0xFFFFFFFF for k in ks])
    verdicts = (C.c_int32 * max(n, 1))()
    rc = lib().zkir_pcs_verify_many_device(kinds_c, ptrs, lens, r, p, e, n, verdicts, stream)
    if rc != 0:
        _raise(abs(rc))
    return [int(verdicts[i]) for i in range(n)]


def batch_eval_verify(proof, roots=None, points=None, evals=None, device: bool = False, stream=None) -> int:
    """zkir_batch_eval_verify, on the host — no GPU: 0 = the proof convinces a holder of its roots that every column of every committed matrix is close to a polynomial of
    degree < 2^log_n that takes the proof's evaluations at the points its matrix is opened at; `roots` ([n_mats][4]), `points` ([n_points][4]) and `evals` (the proof's
    evaluation words, in its exponent order), when given, must be the proof's.  Else the code of the first failing check (include/zkir_amd.h lists them).  The library reads
    as many expected words as the proof's header states: where the header is one a proof can have, expectations of another size raise ValueError.  device=True:
    zkir_batch_eval_verify_device — the same verdict, checks 7 - 11 of all queries on the GPU."""
    w = np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1)
    r = None if roots is None else np.ascontiguousarray(roots, dtype=np.uint32).reshape(-1)
    p = None if points is None else np.ascontiguousarray(points, dtype=np.uint32).reshape(-1)
    e = None if evals is None else np.ascontiguousarray(evals, dtype=np.uint32).reshape(-1)
    sane = len(w) >= 9 and 1 <= int(w[4]) <= 4 and 1 <= int(w[5]) <= 2 and len(w) >= 9 + 2 * int(w[4])
    if sane:
        n_mats, n_points = int(w[4]), int(w[5])
        shape = [(int(w[9 + 2 * m]), int(w[10 + 2 * m])) for m in range(n_mats)]
        sane = all(1 <= wd <= 512 and 1 <= k < (1 << n_points) for wd, k in shape)
    if sane:
        n_evals = sum(wd * bin(k).count("1") for wd, k in shape)
        for name, a, want in (("roots", r, 4 * n_mats), ("points", p, 4 * n_points), ("evals", e, 4 * n_evals)):
            if a is not None and len(a) != want:
                raise ValueError(f"batch_eval_verify: {name} must hold {want} words, what the proof's header states")
    else:
        r = p = e = None                                         # the proof is malformed (1) whatever is expected of it
    ptr = lambda a: a.ctypes.data if a is not None else None
    if device:
        return _pcs_verdict(lib().zkir_batch_eval_verify_device(w.ctypes.data if len(w) else None, len(w), ptr(r), ptr(p), ptr(e), stream))
    return int(lib().zkir_batch_eval_verify(w.ctypes.data if len(w) else None, len(w), ptr(r), ptr(p), ptr(e)))


def _mixed_shape(log_ns, shapes):
    """the flat arrays of the mixed-eval calls from shapes[h] = (widths, masks, n_points); None where the lists cannot be laid out (the library is then not called)"""
    log_ns, shapes = [int(x) for x in log_ns], [([int(x) for x in w], [int(x) for x in k], int(n)) for w, k, n in shapes]
    if len(shapes) != len(log_ns) or any(len(w) != len(k) for w, k, _ in shapes):
        return None
    if any(not 0 <= x < 2**32 for x in log_ns) or any(not 0 <= x < 2**32 for w, k, n in shapes for x in w + k + [n]):
        return None
    u = lambda xs: np.array(xs, np.uint32)
    return u(log_ns), u([len(w) for w, _, _ in shapes]), u([n for _, _, n in shapes]), u([x for w, _, _ in shapes for x in w]), u([x for _, k, _ in shapes for x in k])


def mixed_eval_proof_words(log_ns, log_blowup: int, shapes, num_queries: int) -> int:
    """Words of an evaluation proof over several heights (zkir_mixed_eval_proof_words): log_ns strictly decreasing, shapes[h] = (widths, masks, n_points) of group h;
    0 for a shape no proof can state."""
    flat = _mixed_shape(log_ns, shapes)
    if flat is None or not 0 <= int(log_blowup) < 2**32 or not 0 <= int(num_queries) < 2**32:
        return 0
    ln, nm, npt, ws, ks = flat
    return int(lib().zkir_mixed_eval_proof_words(int(log_blowup), len(ln), ln.ctypes.data, nm.ctypes.data, npt.ctypes.data, ws.ctypes.data, ks.ctypes.data, int(num_queries)))


def mixed_eval_groups(proof):
    """The group words of a 'ZKMH' proof's header, the one Python parse of them (mixed_eval_verify's sizes, stark.mixed_eval_layout): [{log_n, widths, masks, n_points}] and
    the word after them, or None where the header is one no proof can have (n_groups, a group's n_mats, n_points, a width, a mask; cut short)."""
    w = np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1)
    if len(w) < 7 or not 2 <= int(w[3]) <= 3:
        return None
    at, groups = 7, []
    for _ in range(int(w[3])):
        if len(w) < at + 3 or not 1 <= int(w[at + 1]) <= 4 or not 1 <= int(w[at + 2]) <= 2 or len(w) < at + 3 + 2 * int(w[at + 1]):
            return None
        nm, npt = int(w[at + 1]), int(w[at + 2])
        widths, masks = [int(x) for x in w[at + 3:at + 3 + 2 * nm:2]], [int(x) for x in w[at + 4:at + 3 + 2 * nm:2]]
        if not all(1 <= wd <= 512 and 1 <= k < (1 << npt) for wd, k in zip(widths, masks)):
            return None
        groups.append({"log_n": int(w[at]), "widths": widths, "masks": masks, "n_points": npt})
        at += 3 + 2 * nm
    return groups, at


def mixed_eval_sizes(proof):
    """(n_mats, n_points, n_evals) over all the groups as the header of a 'ZKMH' proof states them, or None where the header is one no proof can have"""
    parsed = mixed_eval_groups(proof)
    if parsed is None:
        return None
    groups = parsed[0]
    return (sum(len(g["widths"]) for g in groups), sum(g["n_points"] for g in groups),
            sum(wd * bin(k).count("1") for g in groups for wd, k in zip(g["widths"], g["masks"])))


def mixed_eval_verify(proof, roots=None, points=None, evals=None, device: bool = False, stream=None) -> int:
    """zkir_mixed_eval_verify, on the host — no GPU: 0 = the proof convinces a holder of its roots that every column of every committed matrix of
    every group is close to a polynomial of degree < 2^(its group's log_n) that takes the proof's evaluations at the points its matrix is opened at; `roots`, `points` and
    `evals` (all groups' words, in the proof's order), when given, must be the proof's.  Else the code of the first failing check (include/zkir_amd.h lists them).  The library
    reads as many expected words as the proof's header states: where the header is one a proof can have, expectations of another size raise ValueError.  device=True:
    zkir_mixed_eval_verify_device — the same verdict, checks 7 - 11 of all queries on the GPU (three launches on `stream`)."""
    w = np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1)
    r = None if roots is None else np.ascontiguousarray(roots, dtype=np.uint32).reshape(-1)
    p = None if points is None else np.ascontiguousarray(points, dtype=np.uint32).reshape(-1)
    e = None if evals is None else np.ascontiguousarray(evals, dtype=np.uint32).reshape(-1)
    sizes = mixed_eval_sizes(w)
    if sizes is not None:
        for name, a, want in (("roots", r, 4 * sizes[0]), ("points", p, 4 * sizes[1]), ("evals", e, 4 * sizes[2])):
            if a is not None and len(a) != want:
                raise ValueError(f"mixed_eval_verify: {name} must hold {want} words, what the proof's header states")
    else:
        r = p = e = None                                         # the proof is malformed (1) whatever is expected of it
    ptr = lambda a: a.ctypes.data if a is not None else None
    if device:
        return _pcs_verdict(lib().zkir_mixed_eval_verify_device(w.ctypes.data if len(w) else None, len(w), ptr(r), ptr(p), ptr(e), stream))
    return int(lib().zkir_mixed_eval_verify(w.ctypes.data if len(w) else None, len(w), ptr(r), ptr(p), ptr(e)))


def verify_last_stages() -> dict:
    """zkir_verify_last_stages: the host clocks (ms) of this thread's last verification and how many of its stages ran on the device."""
    ms, n = (C.c_double * 5)(), C.c_uint32(0)
    rc = lib().zkir_verify_last_stages(ms, C.byref(n))
    if rc != ZKIR_OK:
        raise RuntimeError(rc, "no verification has run on this thread")
    return {"parse": ms[0], "section_digests": ms[1], "hash_table_side": ms[2], "wide_table_side": ms[3], "rest": ms[4], "device_stages": int(n.value)}


def interpret(program: Program | bytes, inputs: Sequence[int] = (), config: Optional[VMConfig] = None, tile_rows: int = 0,
              window: Optional[Tuple[int, int]] = None) -> DeltaLog:
    """Host stage only (zkir_interpret): run the program, return the delta log.  Never touches a GPU.
    window = (row_begin, row_end): zkir_interpret_window — rows before row_begin are executed untraced, the log holds the window."""
    blob = program if isinstance(program, (bytes, bytearray)) else program.to_bytes()
    cfg = (config or VMConfig())._c()
    arr = (C.c_uint64 * max(1, len(inputs)))(*[int(x) & (2**64 - 1) for x in inputs])
    out = C.c_void_p()
    if window is None:
        rc = lib().zkir_interpret(bytes(blob), len(blob), arr, len(inputs), C.byref(cfg), tile_rows, C.byref(out))
    else:
        rc = lib().zkir_interpret_window(bytes(blob), len(blob), arr, len(inputs), C.byref(cfg), tile_rows, int(window[0]), int(window[1]), C.byref(out))
    if rc != ZKIR_OK:
        _raise(rc)
    return DeltaLog(out.value)


class ExecutionTrace:
    """Device-resident SoA execution trace (TraceRow schema, trace.rs:24-50)."""

    def __init__(self, result_handle: int, n_rows: int):
        self._r, self.n_rows = result_handle, n_rows
        self.columns = lib().zkir_result_trace(result_handle).contents if n_rows else None

    def __len__(self):
        return self.n_rows

    def column(self, field: int, reg: int = 0) -> np.ndarray:
        out = np.empty(self.n_rows, dtype=_FIELD_DTYPE[field])
        if self.n_rows:
            rc = lib().zkir_result_copy_column(self._r, field, reg, out.ctypes.data)
            if rc != ZKIR_OK:
                _raise(rc)
        return out

    _ROW_DTYPE = np.dtype([("cycle", "<u8"), ("pc", "<u8"), ("instruction", "<u4"), ("registers", "<u8", (16,)),
                           ("bound_bits", "<u4", (16,)), ("bound_tag", "u1", (16,)), ("bound_payload", "<u8", (16,)), ("reg_state", "u1", (16,))])

    def rows_window(self, lo: int, hi: int) -> np.ndarray:
        """Rows [lo, hi) as packed reference-shaped records, copied straight from the device columns (sampled parity checks at
        sizes where copying whole columns is wasteful)."""
        assert 0 <= lo <= hi <= self.n_rows
        n = hi - lo
        out = np.zeros(n, dtype=self._ROW_DTYPE)
        if n == 0:
            return out
        c, L = self.columns, lib()

        def grab(base, elt, dtype, reg=None):
            buf = np.empty(n, dtype=dtype)
            off = (lo if reg is None else reg * c.reg_stride + lo) * elt
            rc = L.zkir_device_to_host(buf.ctypes.data, base + off, n * elt)
            if rc != ZKIR_OK:
                _raise(rc)
            return buf
        out["cycle"] = grab(c.cycle, 8, "<u8"); out["pc"] = grab(c.pc, 8, "<u8"); out["instruction"] = grab(c.instruction, 4, "<u4")
        for r in range(16):
            out["registers"][:, r] = grab(c.registers, 8, "<u8", r)
            out["bound_bits"][:, r] = grab(c.bound_bits, 4, "<u4", r)
            out["bound_tag"][:, r] = grab(c.bound_tag, 1, "u1", r)
            out["bound_payload"][:, r] = grab(c.bound_payload, 8, "<u8", r)
            out["reg_state"][:, r] = grab(c.reg_state, 1, "u1", r)
        return out

    def rows(self) -> np.ndarray:
        """All rows as packed reference-shaped records (same dtype as the test oracle's rows)."""
        dt = self._ROW_DTYPE
        out = np.zeros(self.n_rows, dtype=dt)
        out["cycle"] = self.column(FIELD_CYCLE)
        out["pc"] = self.column(FIELD_PC)
        out["instruction"] = self.column(FIELD_INSTRUCTION)
        for r in range(16):
            out["registers"][:, r] = self.column(FIELD_REGISTERS, r)
            out["bound_bits"][:, r] = self.column(FIELD_BOUND_BITS, r)
            out["bound_tag"][:, r] = self.column(FIELD_BOUND_TAG, r)
            out["bound_payload"][:, r] = self.column(FIELD_BOUND_PAYLOAD, r)
            out["reg_state"][:, r] = self.column(FIELD_REG_STATE, r)
        return out


class ExecutionResult:
    """vm.rs:54-78."""

    def __init__(self, result_handle: Optional[int], log: DeltaLog, blob: bytes = b"", inputs: Sequence[int] = (), config: Optional[VMConfig] = None):
        self._r = result_handle
        self._log = log
        self._blob, self._inputs, self._config = blob, list(inputs), config or VMConfig()
        self.cycles: int = log.cycles
        self.outputs: List[int] = log.outputs
        self.halt_reason: HaltReason = log.halt_reason
        self.execution_trace = ExecutionTrace(result_handle, log.n_rows) if result_handle else ExecutionTrace.__new__(ExecutionTrace)
        if not result_handle:
            self.execution_trace._r, self.execution_trace.n_rows, self.execution_trace.columns = None, 0, None
        self.delta_log = log

    # -- the remaining ExecutionResult members (vm.rs:64-103): device columns behind the C handle (zkir_result_*), copied to the
    #    host here as reference-shaped records for the tests --
    def _d2h(self, ptr, n, dtype) -> np.ndarray:
        out = np.empty(n, dtype=dtype)
        if n:
            rc = lib().zkir_device_to_host(out.ctypes.data, ptr, out.nbytes)
            if rc != ZKIR_OK:
                _raise(rc)
        return out

    def _memops(self, cols: MemopColumnsC, n: int) -> np.ndarray:
        out = np.zeros(n, dtype=_MEMOP_DTYPE)
        for name in _MEMOP_DTYPE.names:
            out[name] = self._d2h(getattr(cols, name), n, _MEMOP_DTYPE[name])
        return out

    def memory_witness(self) -> MemoryWitnessC:
        """zkir_result_memory_trace: device columns (row order, CSR row offsets, sorted)."""
        w = MemoryWitnessC()
        rc = lib().zkir_result_memory_trace(self._r, C.byref(w))
        if rc != ZKIR_OK:
            _raise(rc)
        return w

    def get_memory_trace(self) -> np.ndarray:
        """ExecutionResult::get_memory_trace (vm.rs:85-94): every data-memory op, stably sorted by (timestamp, address, Read<Write).
        Returns packed MemoryOp records (address, value, timestamp, is_write, width, bound_*)."""
        if not self._r or self._log.n_rows == 0:
            return np.zeros(0, dtype=_MEMOP_DTYPE)
        w = self.memory_witness()
        return self._memops(w.sorted, w.n_ops)

    def row_memory_ops(self) -> Tuple[np.ndarray, np.ndarray]:
        """TraceRow.memory_ops of every row (trace.rs:49): (ops in row order, offsets[n_rows+1])."""
        if not self._r or self._log.n_rows == 0:
            return np.zeros(0, dtype=_MEMOP_DTYPE), np.zeros(1, dtype=np.uint64)
        w = self.memory_witness()
        return self._memops(w.row_order, w.n_ops), self._d2h(w.row_offsets, w.n_rows + 1, "<u8")

    def memory_op_count(self) -> int:
        """ExecutionResult::memory_op_count (vm.rs:97-102)."""
        return len(self._log.mem_events)

    def range_check_witness(self) -> Optional[RangeCheckWitnessC]:
        if not self._r:
            return None
        w = RangeCheckWitnessC()
        rc = lib().zkir_result_range_check_witnesses(self._r, C.byref(w))
        if rc != ZKIR_OK:
            _raise(rc)
        return w

    @property
    def range_check_witnesses(self) -> list:
        """Vec<RangeCheckWitness> (range_check.rs:209-238): one list of (value, chunks[4], pc) per non-empty checkpoint."""
        log = self._log
        if len(log.rc_events) == 0:
            return []
        if self._r:
            w = self.range_check_witness()
            n = w.n_checks
            v, p = self._d2h(w.value, n, "<u8"), self._d2h(w.pc, n, "<u8")
            c = self._d2h(w.chunks, 4 * w.chunk_stride, "<u2").reshape(4, -1)[:, :n].T
        else:                                   # run without an execution trace: no device handle; expand through the layer-2 launch
            from . import pipeline as pl
            value, pc, chunks, _ = pl.range_checks(log)
            v, p, c = value.cpu().numpy().view(np.uint64), pc.cpu().numpy().view(np.uint64), chunks.cpu().numpy().view(np.uint16).T
        offs = log.rc_offsets
        return [[(int(v[i]), [int(x) for x in c[i]], int(p[i])) for i in range(int(offs[k]), int(offs[k + 1]))] for k in range(len(offs) - 1)]

    @property
    def normalization_witnesses(self) -> np.ndarray:
        """Vec<NormalizationEvent> (normalization_witness.rs:129-138) as packed records."""
        if len(self._log.norm_events) == 0:
            return np.zeros(0, dtype=_NORM_DTYPE)
        if not self._r:
            from . import pipeline as pl
            return pl.normalization_events(self._log)
        w = NormalizationWitnessC()
        rc = lib().zkir_result_normalization_witnesses(self._r, C.byref(w))
        if rc != ZKIR_OK:
            _raise(rc)
        n, c = w.n_events, w.columns
        out = np.zeros(n, dtype=_NORM_DTYPE)
        out["cycle"] = self._d2h(c.cycle, n, "<u8"); out["pc"] = self._d2h(c.pc, n, "<u8")
        out["reg"] = self._d2h(c.reg, n, "u1"); out["opcode"] = self._d2h(c.opcode, n, "u1")
        out["accumulated"][:, 0] = self._d2h(c.accumulated0, n, "<u8"); out["accumulated"][:, 1] = self._d2h(c.accumulated1, n, "<u8")
        out["normalized"][:, 0] = self._d2h(c.normalized0, n, "<u4"); out["normalized"][:, 1] = self._d2h(c.normalized1, n, "<u4")
        out["carries"][:, 0] = self._d2h(c.carry0, n, "<u4"); out["carries"][:, 1] = self._d2h(c.carry1, n, "<u4")
        out["normalized_bits"] = 20; out["limb_bits"] = 30; out["cause"] = 0
        return out

    def sha256_witnesses(self) -> Tuple[np.ndarray, np.ndarray]:
        """Sha256Witness columns of every single-block SHA-256 syscall: (uint32[608][n_blocks], timestamps[n_blocks])."""
        if not self._r:
            return np.zeros((608, 0), dtype=np.uint32), np.zeros(0, dtype=np.uint64)
        w = Sha256WitnessC()
        rc = lib().zkir_result_sha256_witnesses(self._r, C.byref(w))
        if rc != ZKIR_OK:
            _raise(rc)
        cols = self._d2h(w.columns, 608 * w.stride, "<u4").reshape(608, -1)[:, :w.n_blocks]
        return cols, self._d2h(w.timestamps, w.n_blocks, "<u8")

    def exec_stage_ms(self) -> dict:
        """Wall-clock breakdown of the zkir_exec call behind this result (zkir_result_stage_ms)."""
        ms = (C.c_float * 4)()
        if self._r:
            lib().zkir_result_stage_ms(self._r, ms)
        return dict(zip(("interpret", "device_alloc", "h2d", "k1_and_sync"), [float(x) for x in ms]))

    def prove(self, mode: int = 0, num_queries: int = 0, pow_bits: int = 0) -> np.ndarray:
        """zkir_prove_result: the proof of this whole traced run (VM.run with enable_execution_trace) as u32 words — the context, the public inputs and, in modes 3 / 4, the
        memory witness (mode 4: the hash tape too) are made inside the call, on the device."""
        if not self._r:
            raise ValueError("prove() needs the device handle of a traced run (VMConfig.enable_execution_trace)")
        pr = ProverParamsC(int(mode), int(num_queries), int(pow_bits))
        p, n = C.POINTER(C.c_uint8)(), C.c_size_t(0)
        L = lib()
        rc = L.zkir_prove_result(self._r, C.byref(pr), C.byref(p), C.byref(n))
        if rc != ZKIR_OK:
            _raise(rc)
        try:
            return np.frombuffer(C.string_at(p, n.value), dtype="<u4").copy()
        finally:
            L.zkir_proof_bytes_free(p)

    def prove_rate(self, mode: int, log_blowup: int, num_queries: int = 0, pow_bits: int = 0) -> np.ndarray:
        """zkir_prove_result_rate: prove() at log_blowup 1, 2 or 3 — a 'ZKSR' proof of this whole traced run in any mode (verify_rate checks it).  num_queries 0: 50 / 25 / 17
        by rate; pow_bits 0: 12; otherwise 1 .. 128 queries and 0 .. 24 bits."""
        if not self._r:
            raise ValueError("prove_rate() needs the device handle of a traced run (VMConfig.enable_execution_trace)")
        pr = ProverParamsC(int(mode), int(num_queries), int(pow_bits))
        p, n = C.POINTER(C.c_uint8)(), C.c_size_t(0)
        L = lib()
        rc = L.zkir_prove_result_rate(self._r, C.byref(pr), int(log_blowup), C.byref(p), C.byref(n))
        if rc != ZKIR_OK:
            _raise(rc)
        try:
            return np.frombuffer(C.string_at(p, n.value), dtype="<u4").copy()
        finally:
            L.zkir_proof_bytes_free(p)

    def public_inputs(self) -> PublicInputsC:
        """Public inputs of a proof of this run (zkir_public_inputs_of)."""
        return public_inputs(self._log, self._blob, self._inputs, self._config.enable_deferred_model)

    def close(self):
        if self._r:
            lib().zkir_result_free(self._r)    # also frees the delta log it owns
            self._r = None
            self._log._h = None
        else:
            self._log.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VM:
    """VM::new + VM::run (vm.rs:138-358).  `run()` consumes the VM, as in the reference."""

    def __init__(self, program: Program | bytes, inputs: Sequence[int] = (), config: Optional[VMConfig] = None):
        self._blob = bytes(program) if isinstance(program, (bytes, bytearray)) else program.to_bytes()
        self._inputs = [int(x) & (2**64 - 1) for x in inputs]
        self._config = config or VMConfig()
        self._consumed = False

    def run_window(self, row_begin: int, row_end: int) -> ExecutionResult:
        """zkir_exec_window: one GPU's share of the run — rows before row_begin executed untraced on this thread, rows [row_begin,
        row_end) traced, uploaded and filled on the current device (multi-GPU: every rank calls it with its own range)."""
        if self._consumed:
            raise ValueError("VM::run consumes the VM (vm.rs:208)")
        self._consumed = True
        L = lib()
        cfg = self._config._c()
        arr = (C.c_uint64 * max(1, len(self._inputs)))(*self._inputs)
        out = C.c_void_p()
        rc = L.zkir_exec_window(self._blob, len(self._blob), arr, len(self._inputs), C.byref(cfg), int(row_begin), int(row_end), C.byref(out))
        if rc != ZKIR_OK:
            _raise(rc)
        log = DeltaLog(L.zkir_result_delta_log(out.value), owned=False)
        return ExecutionResult(out.value, log, self._blob, self._inputs, self._config)

    def run(self) -> ExecutionResult:
        if self._consumed:
            raise ValueError("VM::run consumes the VM (vm.rs:208)")
        self._consumed = True
        L = lib()
        cfg = self._config._c()
        arr = (C.c_uint64 * max(1, len(self._inputs)))(*self._inputs)
        if not self._config.enable_execution_trace:
            # nothing to materialise on the device: host stage only
            return ExecutionResult(None, interpret(self._blob, self._inputs, self._config), self._blob, self._inputs, self._config)
        out = C.c_void_p()
        rc = L.zkir_exec(self._blob, len(self._blob), arr, len(self._inputs), C.byref(cfg), C.byref(out))
        if rc != ZKIR_OK:
            _raise(rc)
        log = DeltaLog(L.zkir_result_delta_log(out.value), owned=False)
        return ExecutionResult(out.value, log, self._blob, self._inputs, self._config)


def exec_shard(log: "DeltaLog", row_begin: int, row_end: int, blob: bytes = b"", inputs: Sequence[int] = (), config: Optional[VMConfig] = None) -> ExecutionResult:
    """zkir_exec_shard: the drop-in handle for rows [row_begin, row_end) of a finished interpretation, cut out, uploaded to the current
    device and filled there (multi-GPU: one call per device; segment proofs: ranges that share one row)."""
    L = lib()
    out = C.c_void_p()
    rc = L.zkir_exec_shard(log._h, int(row_begin), int(row_end), C.byref(out))
    if rc != ZKIR_OK:
        _raise(rc)
    return ExecutionResult(out.value, DeltaLog(L.zkir_result_delta_log(out.value), owned=False), blob, inputs, config)


def run(program: Program | bytes, inputs: Sequence[int] = ()) -> List[int]:
    """zkir_runtime::run (lib.rs:59-62): default config, outputs only."""
    res = VM(program, inputs, VMConfig()).run()
    try:
        return list(res.outputs)
    finally:
        res.close()
