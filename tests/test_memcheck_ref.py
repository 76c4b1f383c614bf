"""tests/memcheck_ref.py (the plain replay the GPU tests of memcheck.hip compare with) is held to the host's sequential replay rt.MemcheckWitness — itself held to the oracle
by tests/test_abi.py and tests/test_memory_edges.py — on the rows of real runs: mem_old and mem_told of every row, the touched cells and, in mode 4, the hash section word for
word; and the refusals fall into the same classes.  The rows are the oracle's, the written digests the interpreter's records.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import memcheck_ref as mr
import programs as pg
from oracle import api as oracle
from test_hash_outs import NAMED, hash_case
from zkir_amd import runtime as rt, spec

MODE3_NAMED = ["mem_sw_lw", "timestamps", "loads_stores", "alu_all", "q9_access_at_own_pc", "echo5"]          # tests/test_abi.py's mode-3 list, with random 1 / 3 / 5 below
REFUSAL_MESSAGE = {"address": "is not below 2^40", "hash": "its memory effect is not stated", "hash_range": "is outside what a proof states"}


def _case(which):
    """(blob, inputs, config): a builder of tests/programs.py by name, ("ring", log2_cells, cycles), ("random", seed) without hash calls, ("random_hashes", seed) with them."""
    if isinstance(which, tuple) and which[0] == "ring":
        return spec.memory_ring_program(which[1]).to_bytes(), [], {"max_cycles": which[2]}
    if isinstance(which, tuple) and which[0] == "random":
        blob, ins = pg.random_program(which[1], hashes=False)
        return blob, list(ins), {}
    if isinstance(which, tuple):
        return hash_case(which[1])
    blob, ins, cfg = getattr(pg, which)()
    return blob, list(ins), {k: v for k, v in cfg.items() if k == "max_cycles"}


def _run(which):
    blob, ins, cfg = _case(which)
    rows = oracle.run(blob, ins, enable_execution_trace=True, **cfg).rows
    log = rt.interpret(blob, ins, rt.VMConfig(enable_execution_trace=True, **cfg))
    assert int(log.n_rows) == len(rows)
    return blob, rows, log


def _reference(rows, blob, mode, log):
    return mr.replay(np.ascontiguousarray(rows["instruction"]), np.ascontiguousarray(rows["registers"].T), blob, mode, log.hash_outs if mode == 4 else None)


def _host(log, blob, mode):
    hw = rt.MemcheckWitness(log, blob, mode)
    pub = rt.PublicInputsC(); pub.with_memory(hw)
    n, nc = int(log.n_rows), hw.n_cells
    assert pub.n_cells == nc
    arr = lambda p, t, m: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), (m,)).copy() if m and p else np.zeros(0, np.dtype(t))  # noqa: E731
    w = {"mem_old": arr(pub.mem_old, C.c_uint64, n), "mem_told": arr(pub.mem_told, C.c_uint32, n), "cell_addr": arr(pub.cell_addr, C.c_uint64, nc),
         "cell_bytes": arr(pub.cell_bytes, C.c_uint64, nc), "cell_time": arr(pub.cell_time, C.c_uint32, nc)}
    if mode == 4:
        w["hash_section"] = arr(pub.hash_section, C.c_uint32, int(pub.hash_section_words))
    return w, hw


def _assert_equal(which, mode, min_calls=0):
    blob, rows, log = _run(which)
    want, hw = _host(log, blob, mode)
    got = _reference(rows, blob, mode, log)
    assert got.refusal is None
    for name, w in want.items():
        g = getattr(got, name)
        assert g.dtype == w.dtype and len(g) == len(w), (name, len(g), len(w))
        if not np.array_equal(g, w):
            raise AssertionError(f"{name}: first difference at {int(np.nonzero(g != w)[0][0])} of {len(w)}")
    hash_cells = 0
    if mode == 4:
        assert int(got.hash_section[0]) == hw.n_hash_calls >= min_calls
        hash_cells = (len(got.hash_section) - 1 - 8 * hw.n_hash_calls) // 5
    assert got.n_accesses == hw.n_accesses + hash_cells                    # (the host counts the load / store rows only)
    log.close()
    return got


RANDOM_SEEDS = [20, 21, 25, 26, 27, 28, 29, 30, 32, 33]       # (seeds whose program runs to its EBREAK without hash calls: others stop on a VM error, which has no witness)
MEM_PROGRAMS = MODE3_NAMED + sorted(pg.MEM_EDGES) + [("random", s) for s in (1, 3, 5)] + [("ring", 3, 700), ("ring", 6, 3000)] + [("random", s) for s in RANDOM_SEEDS]
HASH_PROGRAMS = sorted(pg.HASH_EDGES) + NAMED + [("random_hashes", s) for s in RANDOM_SEEDS]
_id = lambda w: w if isinstance(w, str) else "_".join(str(x) for x in w)  # noqa: E731


@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("which", MEM_PROGRAMS, ids=_id)
def test_reference_equals_host_replay_on_runs_of_loads_and_stores(which, mode):
    got = _assert_equal(which, mode)
    assert got.n_accesses >= 1 or which in ("alu_all", "echo5")            # (those two run no load or store: the empty witness)


@pytest.mark.parametrize("which", HASH_PROGRAMS, ids=_id)
def test_reference_equals_host_replay_on_runs_with_hash_calls(which):
    _assert_equal(which, 4, min_calls=0 if isinstance(which, tuple) else 1)


def test_the_ring_revisits_its_cells():
    """The ring runs above are long enough to come round: a cell's second visit reads what the first one stored."""
    blob, rows, log = _run(("ring", 3, 700))
    got = _reference(rows, blob, 3, log)
    assert len(got.cell_addr) == 8 and got.n_accesses > 5 * 8 * 4 and int(got.mem_told.max()) > 128
    log.close()


@pytest.mark.parametrize("which,mode,want", [("edge_at_2p40", 3, "address"), ("edge_at_2p40", 4, "address"), ("edge_above_2p40", 3, "address"), ("edge_above_2p40", 4, "address"),
                                             ("hash_edge_len_over", 4, "hash_range"), ("hash_edge_out_over_2p40", 4, "hash_range"),
                                             ("hash_edge_len_over", 3, "hash"), ("hash_edge_out_over_2p40", 3, "hash"), ("sha256_hello", 3, "hash")])
def test_refusal_classes_agree(which, mode, want):
    blob, rows, log = _run(which)
    got = _reference(rows, blob, mode, log)
    assert got.refusal == want and got.mem_old is None
    with pytest.raises(rt.RuntimeError) as e:
        rt.MemcheckWitness(log, blob, mode)
    assert e.value.code == rt.ERR_ARGUMENT and REFUSAL_MESSAGE[want] in e.value.message
    log.close()


def test_records_that_are_not_the_runs_are_refused():
    """The records are an input of the reference (as of the device): one too few, one too many, one on another row — refused; a trailing record of the last row is ignored."""
    blob, rows, log = _run("hashes_all")
    ins, regs, outs = np.ascontiguousarray(rows["instruction"]), np.ascontiguousarray(rows["registers"].T), log.hash_outs.copy()
    want = mr.replay(ins, regs, blob, 4, outs)
    assert want.refusal is None and len(outs) >= 3
    assert mr.replay(ins, regs, blob, 4, outs[:-1]).refusal == "records"
    assert mr.replay(ins, regs, blob, 4, outs[1:]).refusal == "records"
    assert mr.replay(ins, regs, blob, 4, None).refusal == "records"
    moved = outs.copy(); moved["row"][1] += 1
    assert mr.replay(ins, regs, blob, 4, moved).refusal == "records"
    extra = np.concatenate([outs, outs[-1:]]); extra["row"][-1] = len(ins) - 2
    assert mr.replay(ins, regs, blob, 4, extra).refusal == "records"
    extra["row"][-1] = len(ins) - 1                               # on the last row: ignored
    got = mr.replay(ins, regs, blob, 4, extra)
    assert got.refusal is None and np.array_equal(got.hash_section, want.hash_section) and np.array_equal(got.cell_bytes, want.cell_bytes)
    flipped = outs.copy(); flipped["bytes"][0][5] ^= 1            # what a call wrote is an input: other bytes, other cells
    assert not np.array_equal(mr.replay(ins, regs, blob, 4, flipped).cell_bytes, want.cell_bytes)
    log.close()


def test_the_image_counts_as_empty_when_the_blob_is_short():
    blob = spec.Program.from_code([pg.A(5, 0, 0x1000), spec.encode(spec.Opcode.LD, 1, 5, imm=0), pg.EB], data=b"abc").to_bytes()
    ins = np.array([int.from_bytes(blob[32 + 4 * k:36 + 4 * k], "little") for k in range(3)], np.uint32)
    regs = np.zeros((16, 3), np.uint64); regs[5, 1:] = 0x1000
    assert int(mr.replay(ins, regs, blob, 3).mem_old[1]) == int.from_bytes(blob[32:40], "little")
    assert int(mr.replay(ins, regs, blob[:-1], 3).mem_old[1]) == 0
