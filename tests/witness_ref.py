"""What tests/test_witness_ref.py (host) and tests/test_gpu_witness_edges.py (GPU) share: plain numpy / Python-integer references of the witness expansion (the memory ops in
row order and sorted, the CSR row offsets, the per-row shape flags, the range-check chunks and multiplicities, the normalization events, the 608 SHA-256 chip columns) and
seeded generators of synthetic event logs that sit on the kernels' path edges.  Nothing here is computed by the product; the formulas are the reference's:

  memory ops   MemoryOp { address, value, timestamp, is_write, width, bound = TypeWidth(8 width) } (memory.rs:245); TraceRow.memory_ops keeps the order of execution,
               ExecutionResult::get_memory_trace() sorts by (timestamp, address, Read < Write), stable (vm.rs:85-94, trace.rs:210-223)
  range check  per 20-bit limb of the 40-bit value: limb & mask, (limb >> chunk_bits) & mask (range_check.rs:175-192); the table has 2^chunk_bits entries
  norm         limbs read with 20 bits (normalized register) or 30 bits (accumulated), then a 20-bit carry chain (state.rs:202-220, normalize.rs:133-153)
  SHA-256      FIPS 180-4 section 6.2.2 on ONE block from the initial hash value, every intermediate kept (crypto.rs:142-207)"""
import math
from typing import NamedTuple

import numpy as np

from zkir_amd import runtime as rt

U64 = np.uint64
BOUND_TYPE_WIDTH = 1                                          # ValueBound::from_type_width: tag 1, payload = the bits
GAP_DIFFS = (1, 2, 31, 32, 33, 34, 63, 64, 65, 255, 256, 257, 600)       # row differences round the inline / queued gap boundary (32 rows) and the workgroup size
GAP_FIRST = (0, 31, 32, 33)                                   # row of the first op
GAP_TAIL = (0, 1, 31, 32, 33, 5000)                           # rows behind the last op
LANE0 = (64, 128, 256, 512)                                   # first lanes of a wave (64) and of a workgroup (256)
RC_EDGES = (0, 2**20 - 1, 2**20, 2**40 - 1)
NORM_EDGES = (0, 2**20 - 1, 2**20, 2**40 - 1, 2**60 - 1, 2**64 - 1)


# ---- the references -----------------------------------------------------------------------------------------------------------------------------------------------------
def memops(events, n_rows, cycle_base):
    """(row-order records, CSR offsets u64[n_rows + 1], sorted records, shape flag u8[n_rows]) of a row-ordered log of rt.MEM_EVENT_DTYPE."""
    ev = np.asarray(events, dtype=rt.MEM_EVENT_DTYPE)
    n = len(ev)
    rec = np.zeros(n, dtype=rt._MEMOP_DTYPE)
    rec["address"] = ev["address"]; rec["value"] = ev["value"]
    rec["timestamp"] = [(int(cycle_base) + int(r)) & (2**64 - 1) for r in ev["row"]]
    rec["is_write"] = ev["is_write"]; rec["width"] = ev["width"]
    rec["bound_bits"] = 8 * ev["width"].astype(np.uint32)
    rec["bound_tag"] = BOUND_TYPE_WIDTH
    rec["bound_payload"] = 8 * ev["width"].astype(U64)
    row = ev["row"].astype(np.int64)
    offsets = np.searchsorted(row, np.arange(n_rows + 1), "left").astype(U64)
    order = np.lexsort((np.arange(n), ev["is_write"], ev["address"].astype(U64), row))
    flags = np.zeros(n_rows, dtype=np.uint8)
    if n > 1:
        wr, addr = ev["is_write"].astype(np.int64), ev["address"].astype(U64)
        bad = (row[1:] == row[:-1]) & ((wr[1:] < wr[:-1]) | ((wr[1:] == wr[:-1]) & (addr[1:] < addr[:-1])))
        flags[row[1:][bad]] = 1
    return rec, offsets, rec[order], flags


def shape_violations(events):
    """[(index of the second op, "write_before_read" | "descending")] — the same test as the flag of memops(), op by op in Python integers (the generators' self-check)."""
    out = []
    for i in range(1, len(events)):
        a, b = events[i - 1], events[i]
        if int(a["row"]) != int(b["row"]):
            continue
        if int(b["is_write"]) < int(a["is_write"]):
            out.append((i, "write_before_read"))
        elif int(b["is_write"]) == int(a["is_write"]) and int(b["address"]) < int(a["address"]):
            out.append((i, "descending"))
    return out


def range_checks(events, chunk_bits):
    """(value u64[n], pc u64[n], chunks u16[n][4], multiplicity u32[2^chunk_bits])"""
    ev = np.asarray(events, dtype=rt.RC_EVENT_DTYPE)
    mask = U64((1 << chunk_bits) - 1)
    chunks = np.zeros((len(ev), 4), dtype=np.uint16)
    for l in range(2):
        limb = (ev["value"] >> U64(20 * l)) & U64(0xFFFFF)
        chunks[:, 2 * l] = limb & mask
        chunks[:, 2 * l + 1] = (limb >> U64(chunk_bits)) & mask
    mult = np.bincount(chunks.reshape(-1), minlength=1 << chunk_bits).astype(np.uint32)
    return ev["value"].copy(), ev["pc"].copy(), chunks, mult


def norm(events):
    """NormalizationEvent records (rt._NORM_DTYPE) of rt.NORM_EVENT_DTYPE events; normalized_bits = 20, limb_bits = 30, cause 0 as the runtime records them."""
    ev = np.asarray(events, dtype=rt.NORM_EVENT_DTYPE)
    out = np.zeros(len(ev), dtype=rt._NORM_DTYPE)
    out["cycle"] = ev["cycle"]; out["pc"] = ev["pc"]; out["reg"] = ev["reg"]; out["opcode"] = ev["opcode"]
    out["normalized_bits"] = 20; out["limb_bits"] = 30; out["cause"] = 0
    for i, (raw, state) in enumerate(zip(ev["raw_value"], ev["state"])):
        raw, bits = int(raw), (20 if int(state) == 0 else 30)           # read_reg_limbs_extended: a normalized register is read with normalized_bits
        acc = [raw & ((1 << bits) - 1), (raw >> bits) & ((1 << bits) - 1)]
        carry0, norm0 = acc[0] >> 20, acc[0] & 0xFFFFF
        limb1 = acc[1] + carry0
        out["accumulated"][i] = acc
        out["normalized"][i] = [norm0, limb1 & 0xFFFFF]
        out["carries"][i] = [carry0, limb1 >> 20]
    return out


def _icbrt(x):
    r = int(round(x ** (1 / 3)))
    while r ** 3 > x:
        r -= 1
    while (r + 1) ** 3 <= x:
        r += 1
    return r


_PRIMES = [p for p in range(2, 312) if all(p % q for q in range(2, int(p ** 0.5) + 1))][:64]
SHA_H0 = np.array([math.isqrt(p << 64) & 0xFFFFFFFF for p in _PRIMES[:8]], dtype=np.uint32)      # FIPS 180-4 5.3.3: fractional parts of the square roots
SHA_K = np.array([_icbrt(p << 96) & 0xFFFFFFFF for p in _PRIMES], dtype=np.uint32)                # 4.2.2: of the cube roots
assert SHA_H0[0] == 0x6A09E667 and SHA_K[0] == 0x428A2F98 and SHA_K[63] == 0xC67178F2


def _rotr(x, n):
    return (x >> np.uint32(n)) | (x << np.uint32(32 - n))


def sha256_witness_columns(blocks):
    """u32[608][n] of ANY sixteen-word blocks (u32[n][16]): [0,16) message_block, [16,24) initial_state, [24,88) message_schedule, [88,600) round_states[64][8] (a..h after
    each round), [600,608) final_state."""
    m = np.ascontiguousarray(blocks, dtype=np.uint32).reshape(-1, 16)
    n = len(m)
    out = np.zeros((608, n), dtype=np.uint32)
    w = [m[:, t].copy() for t in range(16)]
    for t in range(16, 64):
        s0 = _rotr(w[t - 15], 7) ^ _rotr(w[t - 15], 18) ^ (w[t - 15] >> np.uint32(3))
        s1 = _rotr(w[t - 2], 17) ^ _rotr(w[t - 2], 19) ^ (w[t - 2] >> np.uint32(10))
        w.append(s1 + w[t - 7] + s0 + w[t - 16])
    out[0:16] = m.T
    out[16:24] = SHA_H0[:, None]
    out[24:88] = np.stack(w)
    a, b, c, d, e, f, g, h = [np.full(n, x, dtype=np.uint32) for x in SHA_H0]
    for t in range(64):
        t1 = h + (_rotr(e, 6) ^ _rotr(e, 11) ^ _rotr(e, 25)) + ((e & f) ^ (~e & g)) + SHA_K[t] + w[t]
        t2 = (_rotr(a, 2) ^ _rotr(a, 13) ^ _rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))
        h, g, f, e, d, c, b, a = g, f, e, d + t1, c, b, a, t1 + t2
        out[88 + 8 * t:96 + 8 * t] = np.stack([a, b, c, d, e, f, g, h])
    out[600:608] = SHA_H0[:, None] + np.stack([a, b, c, d, e, f, g, h])
    return out


def sha_pad_single_block(msg: bytes) -> np.ndarray:
    """The sixteen big-endian words of a message below 56 bytes, padded (FIPS 180-4 5.1.1)."""
    assert len(msg) < 56
    padded = msg + b"\x80" + bytes(55 - len(msg)) + (8 * len(msg)).to_bytes(8, "big")
    return np.frombuffer(padded, dtype=">u4").astype(np.uint32)


# ---- synthetic event logs -----------------------------------------------------------------------------------------------------------------------------------------------
class MemCase(NamedTuple):
    events: np.ndarray            # rt.MEM_EVENT_DTYPE, ordered by row
    n_rows: int
    marks: dict                   # what the case is built to contain (checked by tests/test_witness_ref.py)


class _Log:
    """Rows appended in order; a row's ops are (addresses u64[k], is_write u8[k])."""

    def __init__(self, seed, first_row=0):
        self.parts, self.n, self.row, self.rng = [], 0, first_row - 1, np.random.default_rng(seed)

    def add(self, ops, gap=1):
        addr, wr = ops
        self.row += gap
        self.parts.append((self.row, np.asarray(addr, dtype=U64), np.asarray(wr, dtype=np.uint8)))
        self.n += len(addr)
        return self.row

    def small(self, count, lo=1, hi=4, gap=1):
        """`count` ordinary rows: a load, a store or a short hash call"""
        for _ in range(count):
            self.add(_call(int(self.rng.integers(lo, hi + 1)), base=int(self.rng.integers(0, 1 << 40)), writes=None, rng=self.rng), gap)

    def pad_to(self, index):
        """ordinary rows of 3..9 ops until the next op has `index`"""
        while self.n < index:
            rem = index - self.n
            k = rem if rem <= 9 else rem // 2 if rem < 12 else int(self.rng.integers(3, 10))
            assert k >= 3 or rem < 3
            self.add(_call(k, base=int(self.rng.integers(0, 1 << 40)), writes=k // 3), int(self.rng.integers(1, 4)))

    def case(self, tail=0, **marks):
        ev = np.zeros(self.n, dtype=rt.MEM_EVENT_DTYPE)
        ev["row"] = np.concatenate([np.full(len(a), r, dtype=np.uint32) for r, a, _ in self.parts])
        ev["address"] = np.concatenate([a for _, a, _ in self.parts])
        ev["is_write"] = np.concatenate([w for _, _, w in self.parts])
        ev["value"] = self.rng.integers(0, 1 << 64, self.n, dtype=U64)
        ev["width"] = self.rng.choice(np.array([1, 2, 4, 8], dtype=np.uint8), self.n)
        return MemCase(ev, self.row + 1 + tail, marks)


def _call(k, base=0x2000, writes=32, out=None, rng=None):
    """The ops of one instruction: `k - writes` reads ascending from `base`, then `writes` writes ascending from `out` (a hash call's shape; k = 1 is a load or a store).
    Addresses wrap modulo 2^64."""
    if writes is None:
        writes = int(rng.integers(0, 2)) if k == 1 else min(k // 2, 32)
    writes = min(writes, k)
    out = base + 0x10000 if out is None else out
    with np.errstate(over="ignore"):
        addr = np.concatenate([U64(base % 2**64) + np.arange(k - writes, dtype=U64), U64(out % 2**64) + np.arange(writes, dtype=U64)])
    return addr, np.concatenate([np.zeros(k - writes, dtype=np.uint8), np.ones(writes, dtype=np.uint8)])


def _mem_cases():
    cases = {}
    # gaps: row differences round GAP_INLINE = 32 rows, before the first op, between ops and behind the last
    for first in GAP_FIRST:
        for tail in GAP_TAIL:
            log = _Log(1000 + 10 * first + tail, first_row=first)
            log.small(1)
            for j, d in enumerate(GAP_DIFFS):
                log.small(1, lo=1 + j % 3, hi=1 + j % 3, gap=d)
            cases[f"gaps_first{first}_tail{tail}"] = log.case(tail=tail, first=first, behind=tail)
    log = _Log(1); log.small(1, hi=1)
    cases["one_op_one_row"] = log.case()
    log = _Log(2, first_row=39); log.small(1, hi=1)
    cases["one_op_on_last_row_of_40"] = log.case()
    log = _Log(3, first_row=1)
    log.small(513, hi=1, gap=40)                              # one op on each of the rows 40, 80, ...: every lane meets a gap of 40 rows
    cases["every_lane_queues"] = log.case(tail=5000)
    # rows of 3..9 ops whose first op has index 64, 128, 256, 512
    log = _Log(4)
    for idx in LANE0:
        log.pad_to(idx)
    log.pad_to(530)
    cases["rows_start_at_lane0"] = log.case(tail=3)
    # rows that straddle those indices; a violation whose second op has index 64 (descending reads) and one at 256 (a read behind a write)
    log = _Log(5)
    log.pad_to(63); log.add(([0x5008, 0x5000, 0x5001, 0x5002], [0, 0, 0, 1]), 2)
    log.pad_to(126); log.add(_call(5, base=0x6000, writes=2), 1)
    log.pad_to(255); log.add(([0x7000, 0x7000, 0x7001], [1, 0, 0]), 3)
    log.pad_to(508); log.add(_call(9, base=0x8000, writes=3), 1)
    log.pad_to(530)
    cases["rows_straddle_lane0"] = log.case(violations={64: "descending", 256: "write_before_read"})
    # shape flags
    log = _Log(6); log.small(5)
    log.add((0x9000 + 7 - np.arange(8), np.zeros(8)), 2); log.small(3)
    log.add(([0xA000, 0xA004, 0xA002, 0xA003, 0xB000], [0, 0, 0, 0, 1])); log.small(2)
    cases["flags_descending_reads"] = log.case(tail=2, flagged=2, kinds={"descending"})
    log = _Log(7); log.small(5)
    log.add(([0xC000, 0xC000], [1, 0]), 2); log.small(3)
    log.add(([0xD000, 0xD001, 0xE000, 0xD002, 0xE001], [0, 0, 1, 0, 1])); log.small(2)
    cases["flags_write_before_read"] = log.case(tail=2, flagged=2, kinds={"write_before_read"})
    log = _Log(8); log.small(5)
    log.add(_call(64, base=0xF000, writes=32, out=0xF000), 2); log.small(3)           # reads then writes, equal addresses: no violation
    log.add(([0x100, 0x100, 0x100, 0x101, 0x101, 0x100, 0x100, 0x101], [0, 0, 0, 0, 0, 1, 1, 1])); log.small(2)       # equal neighbours inside a run: not strictly decreasing
    cases["flags_equal_addresses_ok"] = log.case(tail=2, flagged=0, kinds=set())
    log = _Log(9); log.small(5)
    log.add(_call(20 + 32, base=2**64 - 8, writes=32, out=2**64 - 16), 2); log.small(3)        # reads from 2^64 - 8 on, then from 0; the writes wrap as well
    log.add(_call(40, base=2**63 - 4, writes=8, out=0x10), 1)                               # ascending ACROSS 2^63: a violation only to a signed comparison
    log.add(_call(40, base=2**63 + 2**40, writes=8, out=2**63 + 2**40 + 3), 1); log.small(2)
    cases["flags_wrapped_run"] = log.case(tail=2, flagged=1, kinds={"descending"})
    # sort spans
    log = _Log(10)
    for k in (1, 2, 255, 256, 257):
        log.small(2); log.add(_call(k, base=0x20000 * k, writes=min(32, k // 2)))
    cases["sort_rows_1_2_255_256_257"] = log.case(tail=1)
    for k in (2048, 2049):
        log = _Log(10 + k); log.pad_to(256)
        log.add(_call(k, base=0x40000, writes=32)); log.small(4)
        cases[f"sort_row_{k}_at_workgroup_start"] = log.case(big=(256, k))
    log = _Log(12); log.add(_call(3, base=0x300, writes=1))
    log.add(_call(2048, base=0x40000, writes=32)); log.small(4)
    cases["sort_row_2048_behind_a_row_of_3"] = log.case(big=(3, 2048))
    log = _Log(13); log.small(3)
    log.add(_call(4129, base=0x50000, writes=32)); log.small(3)
    cases["sort_row_4129"] = log.case()
    log = _Log(14); log.small(3)
    log.add(_call(232, base=0x60000, writes=32, out=0x60000 + 100)); log.small(3)      # the 32 writes land on addresses the row also reads
    log.add(_call(2300, base=0x70000, writes=32, out=0x70000 + 1000)); log.small(3)    # the same searched in global memory
    cases["sort_writes_overlap_reads"] = log.case()
    log = _Log(15); log.small(3)
    rng = np.random.default_rng(16)
    log.add((rng.integers(0, 1 << 64, 600, dtype=U64) >> U64(int(rng.integers(0, 60))), rng.integers(0, 2, 600)))     # any order, duplicates of neither kind excluded
    log.parts[-1][1][100:140] = log.parts[-1][1][300]                                                                     # equal addresses of both kinds: ties by kind, then index
    log.small(3)
    cases["sort_flagged_row_600"] = log.case(flagged=1)
    return cases


MEM_CASES = _mem_cases()


def rc_log(n, seed, identical=False):
    """n range-check events: the edge values first (as far as n goes), then uniform below 2^40 — or n times one value."""
    rng = np.random.default_rng(seed)
    ev = np.zeros(n, dtype=rt.RC_EVENT_DTYPE)
    ev["value"] = rng.integers(0, 1 << 40, n, dtype=U64)
    k = min(n, len(RC_EDGES))
    ev["value"][:k] = RC_EDGES[:k]
    if identical:
        ev["value"] = 0x5A5A5_A5A5A
    ev["pc"] = rng.integers(0, 1 << 64, n, dtype=U64)
    return ev


def norm_log(n, seed):
    """n normalization events over the whole 64-bit raw range, both states; the edge values in both states first (as far as n goes).  Opcodes stay below 0xA5, the byte the
    GPU tests prefill their outputs with."""
    rng = np.random.default_rng(seed)
    ev = np.zeros(n, dtype=rt.NORM_EVENT_DTYPE)
    ev["cycle"] = rng.integers(0, 1 << 64, n, dtype=U64); ev["pc"] = rng.integers(0, 1 << 64, n, dtype=U64)
    ev["raw_value"] = rng.integers(0, 1 << 64, n, dtype=U64)
    ev["reg"] = rng.integers(1, 16, n); ev["state"] = rng.integers(0, 2, n); ev["opcode"] = rng.integers(0, 0xA5, n)
    edges = [(v, s) for s in (1, 0) for v in NORM_EDGES]
    for i, (v, s) in enumerate(edges[:n]):
        ev["raw_value"][i], ev["state"][i] = v, s
    return ev


def sha_blocks(n, seed):
    """n blocks of sixteen random words with timestamps above 2^32; from n = 3 the first is all zero and the last all ones."""
    rng = np.random.default_rng(seed)
    blk = np.zeros(n, dtype=rt.SHA_BLOCK_DTYPE)
    blk["message_block"] = rng.integers(0, 1 << 32, (n, 16), dtype=np.uint32)
    blk["timestamp"] = (1 << 32) + rng.integers(0, 1 << 62, n, dtype=U64)
    if n >= 3:
        blk["message_block"][0] = 0
        blk["message_block"][-1] = 0xFFFFFFFF
    return blk
