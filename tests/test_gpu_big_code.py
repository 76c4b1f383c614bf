"""GPU parity on programs larger than the prover's LDS window over the instruction ROM (ROM_LDS = 4096 code words) and on pcs past 2^20, against oracle/stark_oracle.cpp.

What the rest of the suite never runs (its largest program has 410 code words, its largest pc is below 0x1668): lookup_index_kernel's global-atomic path for ROM rows
>= 4096 and the split next to it; pc limb 1 in trace_fill_kernel, main_trace_kernel<0 / 2 / 3 / 4>, the quotient kernel's next-pc constraints and the ROM tuple of
lookup_tables_kernel / lookup_index_kernel (the pc + 4 carry, branch / jump deltas that borrow across the limb, links of 2^20 and above); everything sized by n_code at
261 184 words — the tables grid, the arena's n_code * 24 bytes, the pinned staging of the inverses, n_code > N, the boundary cell above 2^20 (LK_B1 = 1), the code-segment
bound of the mode-3 refusal and of the hash-tape check.  The programs are tests/programs.py BIG_CODE; the expected values come from tests/big_code_ref.py, once per process;
tests/test_big_code.py asserts that the programs reach these edges.

COVERED: pc limbs 0 and 1.  NOT COVERED: pc limb 2 — a pc of 2^40 needs a 1 TiB code section, which no program blob can carry (see tests/test_big_code.py)."""
import ctypes as C

import numpy as np
import pytest

import big_code_ref as ref
import helpers
import programs as pg
from oracle import stark_api as so
from zkir_amd import runtime as rt, spec

pytestmark = pytest.mark.gpu
P = so.P


def _device(name, mode, witness=None):
    """(blob, inputs, oracle run, host log, device trace, oracle public inputs, product public inputs) of a big-code program in a proof mode.  `witness` (modes 3 / 4):
    "device" = memcheck.hip builds the memory witness (and, mode 4, the hash tape); "host" = the host's sequential replay."""
    from zkir_amd import pipeline as pl
    blob, ins, cfg = ref.program(name)
    ores = ref.run(name)
    log = rt.interpret(blob, list(ins), rt.VMConfig(enable_execution_trace=True, **cfg))
    assert log.n_rows == len(ores.rows)
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    opub = ref.public(name, mode)
    pub = rt.public_inputs(log, blob, list(ins), io_mode=mode == 2, mem_mode=mode == 3, wide_mode=mode == 4, mem_witness=witness or "device", hash_witness=witness or "host")
    assert pub.deferred == mode and (mode < 2 or list(pub.io_digest) == list(opub.io))
    return blob, list(ins), ores, log, tr, opub, pub


def _assert_words_equal(proof, want, what):
    assert len(proof) == len(want), (what, len(proof), len(want))
    if not np.array_equal(proof, want):
        bad = np.nonzero(proof != want)[0]
        raise AssertionError(f"{what}: proof differs at word {bad[0]} of {len(want)} ({len(bad)} words differ)")


@pytest.mark.parametrize("name", sorted(ref.MODES))
def test_trace_fill_rows_equal_the_oracles(name):
    """trace_fill_kernel: every field of every row, the 64-bit pc column among them."""
    blob, ins, cfg = ref.program(name)
    want = ref.run(name)
    res = rt.VM(blob, list(ins), rt.VMConfig(enable_execution_trace=True, **cfg)).run()
    assert res.cycles == want.cycles and list(res.outputs) == list(want.outputs)
    helpers.assert_rows_equal(res.execution_trace.rows(), want.rows)
    res.close()


@pytest.mark.parametrize("name", sorted(ref.MODES))
def test_main_trace_and_commit_match_oracle(name):
    """main_trace_kernel<0>: all committed columns of the padded main trace — the pc limbs are columns 1 .. 3 — the LDE and the commitment root."""
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = _device(name, 0)
    rows = ores.rows
    wm = stark.main_width(False)
    want_m = so.to_committed(so.main_trace(rows, opub), False)
    got_m = stark.from_b8(stark.main_trace(tr), wm).cpu().numpy().view(np.uint32)
    assert got_m.shape == want_m.shape
    for k in range(wm):
        assert np.array_equal(got_m[k], want_m[k]), f"main-trace column {k}: first difference at row {int(np.nonzero(got_m[k] != want_m[k])[0][0])}"
    ctx = stark.StarkContext(stark.padded_log_n(len(rows)))
    root, L, tree = stark.commit_trace(ctx, tr)
    want_root, want_L = so.commit_trace(rows, 1, want_lde=True, pub=opub)
    assert np.array_equal(stark.from_b8(L, wm).cpu().numpy().view(np.uint32), want_L)
    assert np.array_equal(root, want_root)
    ctx.close(); log.close()


class _IoArgs(C.Structure):
    _fields_ = [("inputs", C.c_void_p), ("n_inputs", C.c_uint64), ("writes_before", C.c_uint64), ("reads_before", C.c_uint64)]


@pytest.mark.parametrize("name,mode", [("pc_carry", 3), ("pc_carry_mem", 3), ("pc_carry_mem_wide", 4), ("rom_straddle", 3)])
def test_device_main_trace_of_modes_3_and_4_equals_the_oracles(name, mode):
    """main_trace_kernel<3> / <4> (+ wide_tape_fix_kernel), host witness: every committed column of every row — the pc limbs, the address limbs and the old bytes of cells
    above 2^20, the boundary cell's window in mode 4.  The failure names the column and the first row."""
    import torch
    blob, ins, ores, log, tr, opub, pub = _device(name, mode, "host")
    nr = len(ores.rows)
    N, wm = 1 << so.padded_log_n(nr), so.committed_width(mode)
    out = torch.zeros((wm // 8, N, 8), dtype=torch.int32, device="cuda")
    scratch = torch.zeros(2 * N + 2 * (N // 1024 + 2) + 64, dtype=torch.int32, device="cuda")
    tape = torch.zeros(1, dtype=torch.int64, device="cuda")
    io = _IoArgs(tape.data_ptr(), 0, 0, 0)
    mo = torch.from_numpy(np.ctypeslib.as_array(C.cast(pub.mem_old, C.POINTER(C.c_uint64)), (nr,)).astype(np.int64)).cuda()
    mt = torch.from_numpy(np.ctypeslib.as_array(C.cast(pub.mem_told, C.POINTER(C.c_uint32)), (nr,)).astype(np.int32)).cuda()
    L = rt.lib()
    V, U64 = C.c_void_p, C.c_uint64
    if mode == 4:
        L.zkir_main_trace_wide_launch.restype = C.c_int
        L.zkir_main_trace_wide_launch.argtypes = [V, U64, V, V, V, U64, V, V, V]
        rc = L.zkir_main_trace_wide_launch(C.byref(tr.c), nr, C.byref(io), mo.data_ptr(), mt.data_ptr(), int.from_bytes(blob[16:20], "little"), scratch.data_ptr(), out.data_ptr(), None)
    else:
        L.zkir_main_trace_mem_launch.restype = C.c_int
        L.zkir_main_trace_mem_launch.argtypes = [V, U64, V, V, V, V, V, V]
        rc = L.zkir_main_trace_mem_launch(C.byref(tr.c), nr, C.byref(io), mo.data_ptr(), mt.data_ptr(), scratch.data_ptr(), out.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32).transpose(0, 2, 1).reshape(wm, N)
    want = so.to_committed(so.main_trace(ores.rows, opub), mode)
    for k in range(wm):
        assert np.array_equal(got[k], want[k]), f"committed column {k}: first difference at row {int(np.nonzero(got[k] != want[k])[0][0])}"
    log.close()


_PROOFS = [(name, mode, w) for name, mode in ref.PROOF_CASES for w in (("device", "host") if mode >= 3 else (None,))]


@pytest.mark.parametrize("name,mode,witness", _PROOFS)
def test_proof_bytes_match_oracle_and_verify(name, mode, witness):
    """The whole proof — the ROM multiplicities from both sides of lookup_index_kernel's split, the aux trace's running sum over them, the quotient over the next-pc
    constraints, the openings — equals the oracle's word for word; both verifiers accept it, with and without expected public inputs, and with the claim in the clear."""
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = _device(name, mode, witness)
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)))
    proof = stark.prove(ctx, tr, pub)
    assert int(proof[9]) == mode
    _assert_words_equal(proof, ref.proof(name, mode), f"{name}, mode {mode}, witness {witness}")
    assert so.verify(proof, opub) == 0 and rt.verify(proof, pub) == 0 and rt.verify(proof) == 0
    if mode >= 2:
        assert rt.verify_io(proof, pub, ins, list(ores.outputs), (ores.halt_kind, ores.halt_code)) == 0
    ctx.close(); log.close()


def test_mode4_device_verifier_gives_the_hosts_verdict(monkeypatch):
    """zkir_verify_device on pc_carry_mem's mode-4 proof: its tape stages hash the one call's record next to a code-segment bound above 2^20.  The host's verdict on the
    honest proof and on three tampered copies: a word of the hash tape, a halfword of the carried program, the last word."""
    from zkir_amd import stark
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_RECORDS", "0")                   # (whatever the default routing of short tapes is: this is about the device stages)
    blob, ins, ores, log, tr, opub, pub = _device("pc_carry_mem_wide", 4, "device")
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)))
    proof = stark.prove(ctx, tr, pub)
    ctx.close(); log.close()
    lay = stark.proof_layout(proof)
    assert lay["mode"] == 4 and int(proof[lay["hash_section"]]) == 1
    assert rt.verify(proof, pub) == 0 and rt.verify(proof, pub, device=True) == 0 and rt.verify(proof, device=True) == 0
    assert rt.verify_last_stages()["device_stages"] >= 1
    for what, pos in (("hash tape", lay["hash_section"] + 4), ("code word", ref.blob_at(4) + 16 + 2 * (pg.W20 - 1)), ("last", len(proof) - 1)):
        t = proof.copy()
        t[pos] = (int(t[pos]) ^ 0x80) if what == "code word" else (int(t[pos]) + 1) % P
        host = rt.verify(t)
        assert host != 0 and so.verify(t) == host and rt.verify(t, device=True) == host, what


def test_memory_witness_device_equals_host_replay():
    """memcheck.hip on pc_carry_mem — every cell above 2^20, the program image (1 MiB of code, then the data the loads read) behind it — against the host's replay: old
    bytes and old time of every row, the touched cells with their final bytes and times."""
    import torch
    blob, ins, ores, log, tr, opub, pub0 = _device("pc_carry_mem", 0)
    torch.cuda.synchronize()
    n = log.n_rows
    hw = rt.MemcheckWitness(log, blob)
    pub = rt.PublicInputsC(); pub.with_memory(hw)
    nc = hw.n_cells
    host = [np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), (m,)).copy() for p, t, m in
            ((pub.mem_old, C.c_uint64, n), (pub.mem_told, C.c_uint32, n), (pub.cell_addr, C.c_uint64, nc), (pub.cell_bytes, C.c_uint64, nc), (pub.cell_time, C.c_uint32, nc))]
    d_old, d_told = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    d_ca, d_cb, d_ct, dn = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint32), C.c_uint64(0)
    L = rt.lib()
    L.zkir_memcheck_witness_device.restype = C.c_int
    L.zkir_memcheck_witness_device.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t] + [C.c_void_p] * 5 + [C.c_uint64, C.c_void_p, C.c_void_p]
    assert L.zkir_memcheck_witness_device(C.byref(tr.c), n, blob, len(blob), d_old.ctypes.data, d_told.ctypes.data, d_ca.ctypes.data, d_cb.ctypes.data, d_ct.ctypes.data, n, C.byref(dn), None) == 0
    assert dn.value == nc and nc >= 3 and (host[2] >= 1 << 20).all()
    for got, want, name in zip((d_old, d_told, d_ca[:nc], d_cb[:nc], d_ct[:nc]), host, ("old bytes", "old time", "cell address", "cell bytes", "cell time")):
        assert np.array_equal(got, want), f"{name}: first difference at {int(np.nonzero(got != want)[0][0])}"
    assert host[0].any()                                                          # some load found initial data or an earlier store
    log.close()


@pytest.mark.parametrize("witness", ["device", "host"])
@pytest.mark.parametrize("name", ref.REFUSED)
def test_mode3_refuses_accesses_to_the_last_code_word(name, witness):
    """A store to / a load from the last word of a 1 MiB code segment: the GPU prover refuses the run with the code-segment message (the bound it compares with is above
    2^20), from either witness; both verifiers reject the oracle's proof of it with check 55 (tests/test_big_code.py)."""
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = _device(name, 3, witness)
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)))
    with pytest.raises(rt.RuntimeError) as e:
        stark.prove(ctx, tr, pub)
    assert e.value.code == rt.ERR_ARGUMENT and "overlaps the code segment" in e.value.message, e.value.message
    ctx.close(); log.close()


def test_pc_carry_proven_in_segments():
    """pc_carry in three segments whose shared rows are the two rows at pc 0xFFFFC (rows 5 and 10): the boundary states carry pc limbs (0xFFFFC, 0) out of one segment and
    into the next, whose first step crosses 2^20.  Each segment proof is the oracle's word for word; the chain verifies as one run in both verifiers."""
    from zkir_amd import pipeline as pl, stark
    blob, ins, cfg = ref.program("pc_carry")
    ores = ref.run("pc_carry")
    log = rt.interpret(blob, [], rt.VMConfig(enable_execution_trace=True, **cfg))
    run_pub, run_opub = rt.public_inputs(log, blob, []), ref.public("pc_carry", 0)
    cuts = [(0, 6), (5, 11), (10, log.n_rows)]
    assert all(int(ores.rows["pc"][b - 1]) == 0xFFFFC for a, b in cuts[:2])
    proofs = []
    for a, b in cuts:
        sh = log.shard(a, b)
        ddl = pl.upload(sh); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
        pub = rt.PublicInputsC.from_buffer_copy(run_pub); pub.n_real = b - a
        ctx = stark.StarkContext(stark.padded_log_n(b - a))
        proof = stark.prove(ctx, tr, pub)
        ctx.close(); sh.close()
        opub = so.PublicC.from_buffer_copy(run_opub); opub.n_real = b - a
        _assert_words_equal(proof, so.prove(ores.rows[a:b], opub), f"segment rows [{a}, {b})")
        proofs.append(proof)
    assert rt.verify_chain(proofs, run_pub) == 0 and so.verify_chain(proofs, run_opub) == 0
    assert rt.verify_chain(proofs[1:]) == 41 and rt.verify_chain([proofs[0]] + proofs[2:]) == 42
    log.close()


def test_one_context_proves_a_small_a_big_and_a_small_program():
    """One StarkContext proves fib (9 code words), then pc_carry (261 184), then fib again: the arena grows by n_code * 24 bytes, the pinned staging by 1 MiB of code and
    261 k inverses.  The big proof is the oracle's; the two fib proofs are the oracle's and byte-identical."""
    from zkir_amd import pipeline as pl, stark
    from oracle import api as oracle
    blob, ins, ores, log, tr, opub, pub = _device("pc_carry", 0)
    n = 1 << stark.padded_log_n(len(ores.rows))
    fblob = spec.fib_endless_program().to_bytes()
    flog = rt.interpret(fblob, [], rt.VMConfig(max_cycles=n, enable_execution_trace=True))
    fddl = pl.upload(flog); ftr = pl.DeviceTrace(fddl); pl.trace_fill(pl.trace_fill_args(fddl, ftr))
    fpub = rt.public_inputs(flog, fblob)
    fres = oracle.run(fblob, max_cycles=n, enable_execution_trace=True)
    want = so.prove(fres.rows, so.public_inputs(n, fblob, [], [], (fres.halt_kind, fres.halt_code)))
    ctx = stark.StarkContext(stark.padded_log_n(n))
    first = stark.prove(ctx, ftr, fpub)
    big = stark.prove(ctx, tr, pub)
    again = stark.prove(ctx, ftr, fpub)
    _assert_words_equal(first, want, "fib before")
    _assert_words_equal(big, ref.proof("pc_carry", 0), "pc_carry")
    assert first.tobytes() == again.tobytes()
    assert rt.verify(big, pub) == 0 and rt.verify(again, fpub) == 0
    ctx.close(); log.close(); flog.close()
