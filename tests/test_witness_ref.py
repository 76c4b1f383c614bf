"""The references of tests/witness_ref.py against the independent CPU oracle, and the self-checks of its synthetic event logs.  No GPU: the host interpreter's side logs of
real programs go through the numpy references and must come out as the oracle's ExecutionResult members, record for record."""
import hashlib

import numpy as np
import pytest

from oracle import api as oracle
from zkir_amd import runtime as rt

import programs
import witness_ref as wr
from test_gpu_witness import MEM_PROGRAMS           # the list only: that module needs no GPU (and no torch) to be imported, its tests are what carries the gpu mark

RC_PROGRAMS = ["rc_doubling", "rc_small_consts", "rc_many_pending", "rc_config_30bit"]
DEFERRED_PROGRAMS = ["deferred_add_branch", "deferred_chain_store", "deferred_add_sub_mix", "deferred_negative_and_overflow", "deferred_fib"]
RANDOM_SEEDS = [100, 102]                                      # seeds whose program runs to its end


def _case(name):
    if isinstance(name, int):
        blob, inputs = programs.random_program(name, n_instr=500)
        return blob, inputs, dict(max_cycles=20000, enable_range_checking=True, enable_deferred_model=True)
    return programs.ALL[name]()


@pytest.mark.parametrize("name", sorted(set(MEM_PROGRAMS + RC_PROGRAMS + DEFERRED_PROGRAMS)) + RANDOM_SEEDS)
def test_references_match_the_oracle_on_program_logs(name):
    blob, inputs, cfg = _case(name)
    cfg = dict(cfg, enable_execution_trace=True)
    log = rt.interpret(blob, inputs, rt.VMConfig(**cfg))
    want = oracle.run(blob, inputs, **cfg)
    if name in MEM_PROGRAMS and name not in ("fib30", "q9_access_at_own_pc") or isinstance(name, int):       # those two touch no memory: all offsets zero
        assert len(want.memops) > 0
    if name in RC_PROGRAMS and name != "rc_small_consts" or isinstance(name, int):
        assert len(want.rc_checks) > 0
    if name in DEFERRED_PROGRAMS and name != "deferred_chain_store" or isinstance(name, int):       # chain_store normalises silently (execute.rs:903-916)
        assert len(want.norm_events) > 0
    rows, offsets, srt, _ = wr.memops(log.mem_events, log.n_rows, log.cycle_base)
    assert rows.dtype == want.memops.dtype
    assert np.array_equal(rows, want.memops)
    assert np.array_equal(offsets, want.row_memop_offsets)
    assert np.array_equal(srt, want.sorted_memops)
    value, pc, chunks, mult = wr.range_checks(log.rc_events, log.rc_chunk_bits)
    assert np.array_equal(value, want.rc_checks["value"]) and np.array_equal(pc, want.rc_checks["pc"])
    assert chunks.dtype == want.rc_checks["chunks"].dtype and np.array_equal(chunks, want.rc_checks["chunks"])
    assert np.array_equal(mult, np.bincount(want.rc_checks["chunks"].reshape(-1), minlength=1 << log.rc_chunk_bits))
    got = wr.norm(log.norm_events)
    assert got.dtype == want.norm_events.dtype and np.array_equal(got, want.norm_events)
    log.close()


def test_sha256_columns_match_the_oracle_witness_and_hashlib():
    msgs = [bytes((11 * i + n) & 0xFF for i in range(n)) for n in range(56)]
    blocks = np.stack([wr.sha_pad_single_block(m) for m in msgs])
    cols = wr.sha256_witness_columns(blocks)
    assert cols.shape == (608, 56) and cols.dtype == np.uint32
    for k, m in enumerate(msgs):
        w = oracle.sha256_witness(m, 7 + k)
        assert np.array_equal(blocks[k], w["message_block"])
        assert np.array_equal(cols[:, k], w["flat"]), f"length {k}"
        assert cols[600:608, k].astype(">u4").tobytes() == hashlib.sha256(m).digest()


def test_sha256_columns_of_unpadded_blocks_are_consistent():
    """Any sixteen words: the layout's own identities hold (the schedule starts with the block, the last round state plus H0 is the final state), block by block the same
    as computed alone."""
    blk = wr.sha_blocks(9, 3)["message_block"]
    cols = wr.sha256_witness_columns(blk)
    assert np.array_equal(cols[0:16], blk.T) and np.array_equal(cols[24:40], blk.T)
    assert np.array_equal(cols[600:608], cols[16:24] + cols[592:600])
    assert not blk[0].any() and (blk[-1] == 0xFFFFFFFF).all()
    for k in range(9):
        assert np.array_equal(wr.sha256_witness_columns(blk[k:k + 1])[:, 0], cols[:, k])


def test_memops_reference_on_a_hand_made_log():
    """Six ops on rows 1, 1, 1, 4, 4, 6 of 8, worked out by hand."""
    ev = np.zeros(6, dtype=rt.MEM_EVENT_DTYPE)
    ev["row"] = [1, 1, 1, 4, 4, 6]
    ev["address"] = [2**64 - 1, 5, 5, 9, 9, 0]
    ev["is_write"] = [0, 1, 0, 1, 1, 0]
    ev["width"] = [1, 2, 4, 8, 1, 2]
    ev["value"] = [10, 11, 12, 13, 14, 15]
    rows, offsets, srt, flags = wr.memops(ev, 8, 2**33 + 5)
    assert list(offsets) == [0, 0, 3, 3, 3, 5, 5, 6, 6]
    assert list(rows["timestamp"]) == [2**33 + 5 + int(r) for r in ev["row"]]
    assert list(rows["bound_bits"]) == [8, 16, 32, 64, 8, 16] and list(rows["bound_payload"]) == [8, 16, 32, 64, 8, 16] and set(rows["bound_tag"]) == {1}
    assert list(srt["value"]) == [12, 11, 10, 13, 14, 15]          # row 1: address 5 read, address 5 write, then 2^64 - 1 (unsigned); row 4: equal keys keep their order
    assert list(flags) == [0, 1, 0, 0, 0, 0, 0, 0]
    assert wr.shape_violations(ev) == [(2, "write_before_read")]
    assert list(wr.memops(ev, 8, 2**64 - 1)[0]["timestamp"][:1]) == [0]          # u64 arithmetic wraps


@pytest.mark.parametrize("name", sorted(wr.MEM_CASES))
def test_memory_logs_are_what_their_names_say(name):
    ev, n_rows, marks = wr.MEM_CASES[name]
    row = ev["row"].astype(np.int64)
    assert len(ev) > 0 and (np.diff(row) >= 0).all() and row[-1] < n_rows
    assert set(ev["is_write"]) <= {0, 1}
    viol = wr.shape_violations(ev)
    flags = wr.memops(ev, n_rows, 0)[3]
    assert sorted(set(int(row[i]) for i, _ in viol)) == list(np.nonzero(flags)[0])
    if "flagged" in marks:
        assert int(flags.sum()) == marks["flagged"]
    elif "violations" not in marks:
        assert not viol
    if "kinds" in marks:
        assert {k for _, k in viol} == marks["kinds"]
    if "violations" in marks:
        assert dict(viol) == marks["violations"]
    starts = np.nonzero(np.diff(row, prepend=-1))[0]                 # index of each row's first op
    sizes = np.diff(np.append(starts, len(ev)))
    if name.startswith("gaps_"):
        assert row[0] == marks["first"] and n_rows - 1 - row[-1] == marks["behind"]
        assert tuple(np.diff(row[starts])) == wr.GAP_DIFFS
    if name == "one_op_one_row":
        assert len(ev) == 1 and n_rows == 1
    if name == "one_op_on_last_row_of_40":
        assert len(ev) == 1 and n_rows == 40 and row[0] == 39
    if name == "every_lane_queues":
        assert len(ev) == 513 and row[0] == 40 and (np.diff(row) == 40).all() and n_rows - 1 - row[-1] == 5000
    if name == "rows_start_at_lane0":
        assert set(wr.LANE0) <= set(starts) and sizes.min() >= 3 and sizes.max() <= 9
    if name == "rows_straddle_lane0":
        assert not set(wr.LANE0) & set(starts) and sizes.min() >= 3 and sizes.max() <= 9
    if name == "flags_wrapped_run":
        assert ev["address"].max() == 2**64 - 1 and ev["address"].min() == 0
        hi = ev["address"] >= 2**63
        assert any(hi[a:b].any() and not hi[a:b].all() and not flags[row[a]] for a, b in zip(starts, starts + sizes))      # an unflagged row on both sides of 2^63
    if name == "flags_equal_addresses_ok":
        assert any(len(set(ev["address"][a:b])) < b - a for a, b in zip(starts, starts + sizes))
    if name == "sort_rows_1_2_255_256_257":
        assert {1, 2, 255, 256, 257} <= set(sizes)
    if "big" in marks:
        at, k = marks["big"]
        j = list(starts).index(at)
        assert sizes[j] == k and ev["is_write"][at:at + k].sum() == 32 and not ev["is_write"][at:at + k - 32].any()
    if name == "sort_row_4129":
        assert 4129 in sizes
    if name == "sort_writes_overlap_reads":
        for a, b in zip(starts, starts + sizes):
            if b - a > 100:
                wr_ = ev["is_write"][a:b] == 1
                assert wr_.sum() == 32 and set(ev["address"][a:b][wr_]) <= set(ev["address"][a:b][~wr_])
    if name == "sort_flagged_row_600":
        j = int(np.argmax(sizes))
        assert sizes[j] == 600 and flags[row[starts[j]]] == 1


def test_small_generators():
    for n in (1, 3, 4, 5000):
        ev = wr.rc_log(n, n)
        assert ev.dtype == rt.RC_EVENT_DTYPE and len(ev) == n and ev["value"].max() < 2**40
        assert list(ev["value"][:4]) == list(wr.RC_EDGES[:n])
    assert len(set(wr.rc_log(300, 1, identical=True)["value"])) == 1
    ev = wr.norm_log(1000, 5)
    assert ev.dtype == rt.NORM_EVENT_DTYPE and set(ev["state"]) == {0, 1} and ev["reg"].min() >= 1 and ev["reg"].max() <= 15
    assert {(int(v), int(s)) for v, s in zip(ev["raw_value"][:12], ev["state"][:12])} == {(v, s) for v in wr.NORM_EDGES for s in (0, 1)}
    assert ev["raw_value"].max() >= 2**63
    blk = wr.sha_blocks(5, 1)
    assert blk.dtype == rt.SHA_BLOCK_DTYPE and blk["timestamp"].min() >= 2**32


def test_norm_reference_on_the_raw_value_edges():
    """2^20 - 1 stays in limb 0; 2^20 is limb 1 of a normalized register and a carry out of limb 0 of an accumulated one; 2^64 - 1 carries out of both limbs."""
    ev = np.zeros(4, dtype=rt.NORM_EVENT_DTYPE)
    ev["raw_value"] = [2**20, 2**20, 2**64 - 1, 2**64 - 1]
    ev["state"] = [0, 1, 0, 1]
    got = wr.norm(ev)
    assert got["accumulated"].tolist() == [[0, 1], [2**20, 0], [2**20 - 1, 2**20 - 1], [2**30 - 1, 2**30 - 1]]
    assert got["normalized"].tolist() == [[0, 1], [0, 1], [2**20 - 1, 2**20 - 1], [2**20 - 1, (2**30 - 1 + 1023) & 0xFFFFF]]
    assert got["carries"].tolist() == [[0, 0], [1, 0], [0, 0], [1023, (2**30 - 1 + 1023) >> 20]]
