"""What the device witness of proof mode 4 needs from the host (CPU tests): the interpreter's record of what every hash syscall WROTE (zkir_hash_out in the delta log: a digest
depends on what earlier calls wrote, and no trace column holds it), the closed forms of hashcall::cells_of that give every touched cell of a call a thread of its own
(csrc/hashcall.h: n_cells_of / rank_of), and the ABI revision that carries the records in zkir_public_inputs."""
import ctypes as C

import numpy as np
import pytest

import programs as pg
from oracle import api as oracle
from zkir_amd import runtime as rt

NAMED = ["sha256_hello", "hashes_all", "blake3_multi_chunk", "sha_chain_small"]
SEEDS = [0, 3, 7, 11]


def hash_case(which):
    """(blob, inputs, config) of the programs the hash-witness tests share: the reference's hash tests, the chain, seeded random programs with hash calls."""
    if isinstance(which, int):
        blob, ins = pg.random_program(which, n_instr=200, hashes=True, wide_safe=True)
        return blob, list(ins), {"max_cycles": 600}
    blob, ins, cfg = getattr(pg, which)()
    return blob, list(ins), {k: v for k, v in cfg.items() if k == "max_cycles"}


def _written_bytes(ores, row):
    """The oracle run's write events of `row` laid out as bytes: (first address, bytes)."""
    lo, hi = int(ores.row_memop_offsets[row]), int(ores.row_memop_offsets[row + 1])
    mem = {}
    for op in ores.memops[lo:hi]:
        if op["is_write"]:
            for k in range(int(op["width"])):
                mem[int(op["address"]) + k] = (int(op["value"]) >> (8 * k)) & 0xFF
    first = min(mem)
    assert sorted(mem) == list(range(first, first + len(mem)))
    return first, bytes(mem[a] for a in sorted(mem))


@pytest.mark.parametrize("which", NAMED + SEEDS)
def test_the_log_records_what_every_hash_call_wrote(which):
    """One record per executed hash syscall, in row order: the row and the 32 bytes as they lie at out .. out + 32 after the call — call for call the oracle run's write events
    of that row.  Their number (the halt row's aside: it executes nothing a proof states) is the host replay's number of hash calls."""
    blob, ins, cfg = hash_case(which)
    ores = oracle.run(blob, ins, enable_execution_trace=True, **cfg)
    log = rt.interpret(blob, ins, rt.VMConfig(enable_execution_trace=True, **cfg))
    rows = ores.rows
    regs = rows["registers"]
    hash_rows = [i for i in range(len(rows)) if (int(rows["instruction"][i]) & 0x7F) == 0x50 and int(regs[i][10]) in (3, 5, 6)]
    if log.halt_reason.kind != rt.HALT_CYCLE_LIMIT and hash_rows and hash_rows[-1] == len(rows) - 1:
        hash_rows.pop()                                           # (a halt row that is an ECALL is the exit, never a hash call; a cycle limit can fall on an executed call)
    outs = log.hash_outs
    assert [int(r) for r in outs["row"]] == hash_rows and len(hash_rows) >= 1
    for rec in outs:
        first, data = _written_bytes(ores, int(rec["row"]))
        assert first == int(regs[int(rec["row"])][13]) and data == bytes(rec["bytes"]), int(rec["row"])
    n = int(log.n_rows)
    assert int(np.count_nonzero(outs["row"] + 1 < n)) == rt.MemcheckWitness(log, blob, 4).n_hash_calls
    pub = rt.public_inputs(log, blob, ins, wide_mode=True, hash_witness="device")
    assert pub.n_hash_outs == len(outs) and pub.hash_outs == outs.ctypes.data and not pub.mem_old and not pub.hash_section       # no witness: zkir_prove builds it on the device
    assert rt.public_inputs(log, blob, ins, wide_mode=True).mem_old                                                              # the default is unchanged: the host replay
    log.close()


def test_untraced_runs_record_nothing():
    blob, ins, cfg = hash_case("hashes_all")
    log = rt.interpret(blob, ins, rt.VMConfig(**cfg))
    assert len(log.hash_outs) == 0
    log.close()


@pytest.mark.parametrize("which", ["hashes_all", "sha_chain_small", 3])
def test_a_shard_or_window_carries_the_records_of_its_rows_rebased(which):
    blob, ins, cfg = hash_case(which)
    log = rt.interpret(blob, ins, rt.VMConfig(enable_execution_trace=True, **cfg))
    outs, n = log.hash_outs, int(log.n_rows)
    mid = int(outs["row"][len(outs) // 2])
    for a, b in ((0, n), (0, mid), (mid, n), (mid + 1, n), (mid // 2, mid + 1), (7, 7)):
        want = outs[(outs["row"] >= a) & (outs["row"] < b)]
        sh = log.shard(a, b)
        assert [int(r) for r in sh.hash_outs["row"]] == [int(r) - a for r in want["row"]]
        assert np.array_equal(sh.hash_outs["bytes"], want["bytes"])
        sh.close()
        if a < b:
            win = rt.interpret(blob, ins, rt.VMConfig(enable_execution_trace=True, **cfg), window=(a, b))
            assert win.cycle_base == a and [int(r) for r in win.hash_outs["row"]] == [int(r) - a for r in want["row"]]
            assert np.array_equal(win.hash_outs["bytes"], want["bytes"])
            win.close()
    log.close()


# ---- the closed forms of hashcall::cells_of --------------------------------------------------------------------------------------------------------------------------
def _cells_of(in_ptr, length, out_ptr):
    """hashcall::cells_of restated: the aligned 8-byte cells under [in, in + len) and [out, out + 32), ascending, each once."""
    cells = set()
    if length:
        cells.update(range(in_ptr & ~7, in_ptr + length, 8))
    cells.update(range(out_ptr & ~7, out_ptr + 32, 8))
    return sorted(cells)


def _closed(in_ptr, length, out_ptr, kind, cell):
    rank = C.c_uint64(0)
    n = rt.lib().zkir_hash_call_cells_host(in_ptr, length, out_ptr, kind, cell, C.byref(rank))
    return n, rank.value


NONE = (1 << 64) - 1


def _check(in_ptr, length, out_ptr, kind, probe_all=True):
    want = _cells_of(in_ptr, length, out_ptr)
    n, _ = _closed(in_ptr, length, out_ptr, kind, 0)
    assert n == len(want), (hex(in_ptr), length, hex(out_ptr), n, len(want))
    probes = want if probe_all else want[:6] + want[-6:] + want[len(want) // 2 - 3:len(want) // 2 + 3]
    for c in probes:
        assert _closed(in_ptr, length, out_ptr, kind, c)[1] == _bisect(want, c), (hex(in_ptr), length, hex(out_ptr), hex(c))
    for c in (want[0] - 8, want[-1] + 8, want[0] + 1, want[0] + 4):
        if c >= 0 and c not in want:
            assert _closed(in_ptr, length, out_ptr, kind, c)[1] == NONE
    gaps = [a + 8 for a, b in zip(want, want[1:]) if b != a + 8]
    for c in gaps:                                                                # the cell behind the lower range, when the two ranges are apart
        assert _closed(in_ptr, length, out_ptr, kind, c)[1] == NONE


def _bisect(a, x):
    import bisect
    return bisect.bisect_left(a, x)


def test_cell_count_and_rank_against_cells_of_on_the_designed_cases():
    base = 0x3000
    for kind in (3, 5, 6):
        offs = (0, 4) if kind == 3 else range(8)
        for length in (0, 1, 7, 8, 9):
            for io in range(8):
                for oo in offs:
                    _check(0x2000 + io, length, base + oo, kind)                  # apart
                    _check(base + io, length, base + oo, kind)                    # in == out (up to the offsets): overlapping from the first cell
        for oo in offs:
            _check(base + oo, 64, base + oo, kind)                                # hash in place
            _check(base, 40, base + 16 + oo, kind)                                # the output inside the input
            _check(base, 20, base + 16 + oo, kind)                                # overlap by a part of a cell
            _check(base, 16 + max(oo, 1), base + 16 + oo, kind)                   # touch in one cell
            _check(base, 16, base + 16 + oo, kind)                                # adjacent cells, none shared
            _check(base, 8, base + 16 + oo, kind)                                 # one cell apart
            _check(base + 64, 9, base + oo, kind)                                 # the output below the input: touching / apart by the offset
            _check(base + 40, 9, base + oo, kind)
        _check(0x100003, 1 << 20, 0x300000, kind, probe_all=False)
        _check(0x100000, 1 << 20, 0x100000 + (1 << 19), kind, probe_all=False)    # 2^20 bytes with the output in the middle
        _check((1 << 40) - 37, 37, (1 << 40) - 32, kind)                          # both buffers end exactly at 2^40
        _check((1 << 40) - (1 << 20), 1 << 20, (1 << 40) - 32, kind, probe_all=False)


def test_cell_count_and_rank_on_random_triples():
    rng = np.random.default_rng(2024)
    for _ in range(10_000):
        kind = (3, 5, 6)[int(rng.integers(0, 3))]
        length = int(rng.integers(0, 300)) if rng.random() < 0.9 else int(rng.integers(0, (1 << 20) + 1))
        in_ptr = int(rng.integers(0, 1 << 16))
        near = rng.random() < 0.7
        out_ptr = max(0, in_ptr + int(rng.integers(-80, length + 80))) if near else int(rng.integers(0, (1 << 40) - 32))
        if kind == 3:
            out_ptr &= ~3
        _check(in_ptr, length, out_ptr, kind, probe_all=length < 300)


def test_calls_outside_what_a_proof_states_are_reported():
    """hashcall::in_range's false cases: the entry returns ~0 (the device witness raises its refusal flag on them)."""
    for in_ptr, length, out_ptr, kind in ((0x2000, 8, 0x3000, 4), (0x100000, (1 << 20) + 1, 0x300000, 5), (0x2000, 8, (1 << 40) - 31, 6), (0x2000, 8, 0x3001, 3), (0x2000, 8, 0x3002, 3),
                                          ((1 << 40) - 4, 5, 0x3000, 5), (1 << 40, 0, 0x3000, 6), (0x2000, 8, 0x3000, 0), (0x2000, 8, 0x3000, 7)):
        assert _closed(in_ptr, length, out_ptr, kind, out_ptr & ~7) == (NONE, NONE)
    assert _closed(0x2000, 1 << 20, (1 << 40) - 32, 3, 0x2000) == ((1 << 17) + 4, 0)                 # the bounds themselves are inside


def test_abi_revision_7_and_the_struct_sizes_agree():
    L = rt.lib()
    assert L.zkir_abi_version() == 7
    assert C.sizeof(rt.PublicInputsC) == L.zkir_public_inputs_size()
    assert rt.PublicInputsC.hash_outs.offset == rt.PublicInputsC.hash_section_words.offset + 8 and rt.PublicInputsC.n_hash_outs.offset + 8 == C.sizeof(rt.PublicInputsC)      # grown at its END
    assert rt.HASH_OUT_DTYPE.itemsize == 40
