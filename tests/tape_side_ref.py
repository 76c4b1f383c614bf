"""What tests/test_tape_table_side.py (host) and tests/test_gpu_tape_table_side.py (GPU) share: the Python-integer reference of the hash tape's and the wide tape's share of
the lookup table side, builders of synthetic tapes, the sections of real runs, and the single-fault mutations of the record checks.  Nothing here is computed by the product.

The convention (oracle: so::hash_table_sum / so::wide_table_sum): N_TUPLE = 11, fp(e; tag) = tag lambda^11 + sum_{j < 11} e_j lambda^j with lambda^0 = 1;
  hash call   e = (cycle mod p; in as limbs 20 / 20 / rest; len likewise; out likewise; kind), tag 12        + 1 / (alpha - fp)    [= the row's HH]
  memory      e = (addr & 0xFFFFF; (addr >> 20) & 0xFFFFF; time; the eight bytes, low first), tag 7           per touched cell - 1 / (alpha - fp(addr, told, old bytes))
                                                                                                                               + 1 / (alpha - fp(addr, (cycle + 1) mod p, new bytes))
  wide record e = (cycle mod p; rs1's three limbs; rs2's three limbs; y & 0xFFFFF; (y >> 20) & 0xFFFFF; y >> 40; opcode), tag 13   + 1 / (alpha - fp)    [= the row's WW]
with y the reference's result on the raw 64-bit registers (execute.rs:101-183)."""
import functools

import numpy as np

from bigint_ref import P, e_inv, e_mul

TAG_MEM, TAG_HASH, TAG_WIDE, N_TUPLE = 7, 12, 13, 11
M64 = (1 << 64) - 1
NT = 256                                                      # the kernels' workgroup size
ALPHA, LAM = [1234567891, 987654321, 5, P - 2], [P - 1, 2, 1357911, 1 << 30]      # canonical challenges nobody derived from the data


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------------------------------
def _lam_pows(lam):
    out = [[1, 0, 0, 0]]
    for _ in range(N_TUPLE):
        out.append(e_mul(out[-1], lam))
    return out


def _den(alpha, pows, e, tag):
    """alpha - fp(e; tag)"""
    assert len(e) == N_TUPLE
    fp = [tag * c % P for c in pows[N_TUPLE]]
    for j, v in enumerate(e):
        fp = [(a + (v % P) * c) % P for a, c in zip(fp, pows[j])]
    return [(a - f) % P for a, f in zip(alpha, fp)]


def _batch_inv(ds):
    """the inverses of nonzero extension elements with ONE e_inv (Montgomery's trick: exact, so the same values as an e_inv each)"""
    pre, acc = [], [1, 0, 0, 0]
    for d in ds:
        pre.append(acc)
        acc = e_mul(acc, d)
    assert any(acc), "a denominator is zero"
    inv, out = e_inv(acc), [None] * len(ds)
    for i in range(len(ds) - 1, -1, -1):
        out[i] = e_mul(inv, pre[i])
        inv = e_mul(inv, ds[i])
    return out


def cells_of(in_ptr, length, out_ptr):
    """the aligned 8-byte cells under [in, in + len) and [out, out + 32), ascending, each once"""
    s = set(range(out_ptr & ~7, out_ptr + 32, 8))
    if length:
        s |= set(range(in_ptr & ~7, in_ptr + length, 8))
    return sorted(s)


def parse_tape(words):
    """[(cycle, in, len, out, kind, [(told, old bytes)])] of a well-formed hash section"""
    w = [int(x) for x in words]
    calls, q = [], 1
    for _ in range(w[0]):
        c = w[q:q + 8]
        n = c[7]
        cells = [(w[q + 8 + 5 * j], sum(w[q + 9 + 5 * j + i] << (16 * i) for i in range(4))) for j in range(n)]
        calls.append((c[0], c[1] | (c[2] << 20), c[3], c[4] | (c[5] << 20), c[6], cells))
        q += 8 + 5 * n
    assert q == len(w)
    return calls


def _signed64(v):
    return v - (1 << 64) if v >> 63 else v


def wide_result(op, a, b):
    """MULH 3 / DIVU 4 / REMU 5 / DIV 6 / REM 7 on raw 64-bit registers (execute.rs:101-183)"""
    if op == 3:
        return ((a * b) >> 40) & ((1 << 40) - 1)
    if op == 4:
        return a // b
    if op == 5:
        return a % b
    sa, sb = _signed64(a), _signed64(b)
    q = abs(sa) // abs(sb) * (1 if (sa < 0) == (sb < 0) else -1)      # truncating; i64::MIN / -1 wraps to i64::MIN, remainder 0
    return (q if op == 6 else sa - q * sb) & M64


def reference(hash_words, new_bytes, wide_words, alpha=ALPHA, lam=LAM):
    """{"sum": [4], "hh": [n_calls][4], "ww": [n_records][4]} in canonical words"""
    pows = _lam_pows(lam)
    limbs = lambda v: [v & 0xFFFFF, (v >> 20) & 0xFFFFF, v >> 40]  # noqa: E731
    dens, signs, h = [], [], 0                                    # sign: +2 a call's own entry, +3 a wide record's, -1 / +1 a cell's two entries
    for cycle, in_ptr, length, out_ptr, kind, cells in parse_tape(hash_words):
        dens.append(_den(alpha, pows, [cycle % P] + limbs(in_ptr) + limbs(length) + limbs(out_ptr) + [kind], TAG_HASH)); signs.append(2)
        addrs = cells_of(in_ptr, length, out_ptr)
        assert len(addrs) == len(cells)
        for addr, (told, old) in zip(addrs, cells):
            nb = int(new_bytes[h]); h += 1
            for t, by, sg in ((told, old, -1), ((cycle + 1) % P, nb, 1)):
                dens.append(_den(alpha, pows, [addr & 0xFFFFF, (addr >> 20) & 0xFFFFF, t] + [(by >> (8 * k)) & 0xFF for k in range(8)], TAG_MEM)); signs.append(sg)
    assert h == len(new_bytes)
    w = [int(x) for x in wide_words]
    assert len(w) == 1 + 8 * w[0]
    for k in range(w[0]):
        r = w[1 + 8 * k:9 + 8 * k]
        a, b = r[1] | (r[2] << 20) | (r[3] << 40), r[4] | (r[5] << 20) | (r[6] << 40)
        dens.append(_den(alpha, pows, [r[0] % P] + r[1:7] + limbs(wide_result(r[7], a, b)) + [r[7]], TAG_WIDE)); signs.append(3)
    T, hh, ww = [0, 0, 0, 0], [], []
    for inv, sg in zip(_batch_inv(dens), signs):
        T = [(a - b) % P for a, b in zip(T, inv)] if sg < 0 else [(a + b) % P for a, b in zip(T, inv)]
        if sg == 2:
            hh.append(inv)
        elif sg == 3:
            ww.append(inv)
    return {"sum": T, "hh": hh, "ww": ww}


def assert_equal(got, want, what=""):
    assert [int(x) for x in got["sum"]] == list(want["sum"]), (what, "sum")
    assert got["hh"].shape == (len(want["hh"]), 4) and got["ww"].shape == (len(want["ww"]), 4), what
    for name in ("hh", "ww"):
        for k, row in enumerate(want[name]):
            assert [int(x) for x in got[name][k]] == list(row), (what, name, k)


# ---- synthetic tapes --------------------------------------------------------------------------------------------------------------------------------------------------------
def make_tape(calls, seed=1):
    """calls: (cycle, in, len, out, kind), cycles increasing -> (section words, new bytes per touched cell): previous-access times at most the cycle (0 and the cycle itself
    among them), old and new bytes random with the extremes mixed in"""
    rng = np.random.default_rng(seed)
    w, nb = [len(calls)], []
    for cycle, in_ptr, length, out_ptr, kind in calls:
        addrs = cells_of(in_ptr, length, out_ptr)
        w += [cycle, in_ptr & 0xFFFFF, in_ptr >> 20, length, out_ptr & 0xFFFFF, out_ptr >> 20, kind, len(addrs)]
        for j in range(len(addrs)):
            told = (0, cycle)[j] if j < 2 else int(rng.integers(0, cycle + 1))
            old = (0, M64)[j] if j < 2 else int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
            w += [told] + [(old >> (16 * i)) & 0xFFFF for i in range(4)]
            nb.append((M64, 0)[j] if j < 2 else int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)))
    return np.array(w, np.uint32), np.array(nb, np.uint64)


def small_calls(n5, n6, first_cycle=3):
    """n5 calls that touch 4 cells (5 items each: len 0, an aligned output) and n6 that touch 5 (6 items: an output at 1 mod 8), the latter in the middle"""
    calls, cycle = [], first_cycle
    for k in range(n5 + n6):
        six = n5 // 2 <= k < n5 // 2 + n6
        calls.append((cycle, 0x2000, 0, 0x30000 + 64 * k + (1 if six else 0), 5 if six else 3))
        cycle += 1 + k % 3
    assert sum(len(cells_of(c[1], c[2], c[3])) for c in calls) == 4 * n5 + 5 * n6
    return calls


RECORD_OPS = [  # one record of each opcode: (cycle, rs1, rs2, opcode)
    (5, (1 << 63) + 12345, (1 << 41) + 99, 3),                  # MULH, both operands above 2^40
    (9, 0xFFFFFFFFFFFFFF80, 7, 4),                             # DIVU of a value above 2^63
    (17, 5, 0x123456789ABCDEF0, 5),                            # REMU with rs2 > rs1
    (21, 1 << 63, M64, 6),                                     # DIV of i64::MIN by -1
    (1000000, 1 << 63, M64, 7),                                # REM of i64::MIN by -1
    (P + 5, 0xFFFFFFFFFFFFFF80, 3, 6),                         # (a cycle above p: taken modulo p; a negative dividend)
]


def make_wide(records):
    w = [len(records)]
    for cycle, a, b, op in records:
        w += [cycle, a & 0xFFFFF, (a >> 20) & 0xFFFFF, a >> 40, b & 0xFFFFF, (b >> 20) & 0xFFFFF, b >> 40, op]
    return np.array(w, np.uint32)


EMPTY = np.array([0], np.uint32)


@functools.lru_cache(maxsize=None)
def synthetic(name):
    """(hash words, new bytes, wide words) of the designed tapes"""
    none = np.zeros(0, np.uint64)
    if name == "empty":
        return EMPTY, none, EMPTY
    if name == "len0":
        return (*make_tape([(7, 0x2001, 0, 0x3000, 3)]), EMPTY)
    if name == "spans":                                          # input and output share cells (one span); two spans, input first and output first; an output at 5 mod 8
        return (*make_tape([(2, 0x3300, 40, 0x3311, 5), (3, 0x2000, 21, 0x3000, 6), (9, 0x5003, 9, 0x4005, 5), (P - 1, (1 << 40) - 37, 37, (1 << 40) - 32, 5)]), EMPTY)
    if name == "len2p17":                                        # 16 388 cells between two 8-cell calls: the search crosses workgroups, many partial sums
        t = make_tape([(10, 0x2000, 32, 0x3000, 3), (11, 0x100000, 1 << 17, 0x300000, 6), (500, 0x2000, 32, 0x3000, 5)])
        assert [int(t[0][1 + 7]), int(t[0][1 + 8 + 40 + 7])] == [8, 16388]
        return (*t, EMPTY)
    if name in ("items255", "items256", "items257"):
        n5, n6 = {"items255": (51, 0), "items256": (50, 1), "items257": (49, 2)}[name]
        t = make_tape(small_calls(n5, n6))
        assert n5 + n6 + len(t[1]) == int(name[5:])
        return (*t, EMPTY)
    if name == "wide_sorted":
        return EMPTY, none, make_wide(sorted(RECORD_OPS))
    if name == "wide_reversed":
        return EMPTY, none, make_wide(sorted(RECORD_OPS)[::-1])
    if name == "wide_blocks":                                    # more records than one workgroup takes
        rng = np.random.default_rng(5)
        recs = [(3 * k + 1, int(rng.integers(1, 1 << 62)) * 4 + k % 4, int(rng.integers(1, 1 << 62)) * 2 + 1, 3 + k % 5) for k in range(NT + 3)]
        return EMPTY, none, make_wide(recs)
    if name == "both":
        return (*make_tape([(2, 0x3300, 40, 0x3311, 5), (30, 0x2000, 100, 0x3000, 3)], seed=4), make_wide(sorted(RECORD_OPS)))
    raise KeyError(name)


SYNTHETIC = ["empty", "len0", "spans", "len2p17", "items255", "items256", "items257", "wide_sorted", "wide_reversed", "wide_blocks", "both"]


@functools.lru_cache(maxsize=None)
def synthetic_reference(name):
    """the reference of a designed tape, computed once for both files"""
    return reference(*synthetic(name))


# ---- real runs --------------------------------------------------------------------------------------------------------------------------------------------------------------
def new_bytes_of(hash_words, hash_outs):
    """per touched cell of a real run's section: the old bytes from the tape, overlaid with the call's 32 bytes from the log's record"""
    out = []
    calls = parse_tape(hash_words)
    assert len(hash_outs) >= len(calls)
    for (cycle, in_ptr, length, out_ptr, kind, cells), rec in zip(calls, hash_outs):
        assert int(rec["row"]) == cycle
        mem = {}
        for addr, (_, old) in zip(cells_of(in_ptr, length, out_ptr), cells):
            for k in range(8):
                mem[addr + k] = (old >> (8 * k)) & 0xFF
        for k in range(32):
            mem[out_ptr + k] = int(rec["bytes"][k])
        out += [sum(mem[addr + k] << (8 * k) for k in range(8)) for addr in cells_of(in_ptr, length, out_ptr)]
    return np.array(out, np.uint64)


def wide_and_hash_program():
    """hash calls and wide-tape rows in one run: DIV / REM / MULH / DIVU / REMU on a register LB sign-extended to 0xFFFF_FFFF_FFFF_FF80, SHA-256 and Keccak-256 calls between"""
    import programs as pg
    from zkir_amd import spec
    A, E, O = pg.A, spec.encode, spec.Opcode
    code = [A(5, 0, 0x4000), A(6, 0, 0x80), E(O.SB, rs1=5, rs2=6, imm=0), E(O.LB, 7, 5, imm=0), A(2, 0, 3), E(O.DIV, 3, 7, 2), E(O.REM, 4, 7, 2)]
    code += pg._call(3, 0x4000, 5, 0x5000) + [E(O.MULH, 8, 7, 7), E(O.DIVU, 9, 7, 2)] + pg._call(5, 0x5000, 32, 0x5021) + [E(O.REMU, 1, 7, 2)]
    return pg._p(code + [pg.EB]), [], {}


def real_program(name):
    import programs as pg
    from zkir_amd import spec
    if name == "wide_and_hash":
        return wide_and_hash_program()
    if name == "signed_division_loop":
        return spec.signed_division_loop_program().to_bytes(), [], {"max_cycles": 300}
    if name == "sha_chain_2p12":
        return spec.sha256_chain_program().to_bytes(), [], {"max_cycles": 1 << 12}
    blob, ins, cfg = getattr(pg, name)()
    return blob, list(ins), {k: v for k, v in cfg.items() if k == "max_cycles"}


REAL = ["sha256_hello", "hashes_all", "hash_edge_calls", "signed_division_loop", "wide_and_hash"]


@functools.lru_cache(maxsize=None)
def real_sections(name):
    """(hash words, new bytes, wide words, n_real, code_end) of a real run: the sections out of the ORACLE's proof, the new bytes from the interpreter's hash_outs records"""
    from oracle import api as oracle, stark_api as so
    from zkir_amd import runtime as rt, stark
    blob, ins, cfg = real_program(name)
    ores = oracle.run(blob, list(ins), enable_execution_trace=True, **cfg)
    opub = so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code), wide_mode=True)
    proof = so.prove(ores.rows, opub)
    lay = stark.proof_layout(proof)
    hs = np.array(proof[lay["hash_section"]:lay["wide_section"]], np.uint32)
    ws = np.array(proof[lay["wide_section"]:lay["rom_mult"]], np.uint32)
    assert np.array_equal(hs, so.hash_section(ores.rows, opub))
    log = rt.interpret(blob, list(ins), rt.VMConfig(enable_execution_trace=True, **cfg))
    nb = new_bytes_of(hs, log.hash_outs)
    log.close()
    return hs, nb, ws, len(ores.rows), 0x1000 + int.from_bytes(blob[16:20], "little")


# ---- the record checks: a valid three-call tape and its single-fault mutations ---------------------------------------------------------------------------------------------
CHECK_N_REAL, CHECK_CODE_END = 4000, 0x1800


def check_tape():
    """three calls: SHA-256 (kind 3) over 40 bytes, Keccak-256 with len 0 at an odd output, BLAKE3 whose input and output share cells; offsets of the records"""
    words, _ = make_tape([(10, 0x2000, 40, 0x3000, 3), (20, 0x2001, 0, 0x3041, 5), (3999, 0x3300, 80, 0x3311, 6)], seed=9)
    w = [int(x) for x in words]
    at, q = [], 1
    for _ in range(3):
        at.append(q); q += 8 + 5 * w[q + 7]
    return words, at


def check_mutations():
    """[(name, words)]: every single fault the issue lists, in the record the name says (r0 / r1 / r2), and the two-fault tapes"""
    base, at = check_tape()
    out = []

    def mut(name, edits, cut=None):
        w = base.copy()
        for pos, val in edits:
            w[pos] = val
        out.append((name, w[:cut] if cut else w))
    for r in range(3):
        a = at[r]
        mut(f"r{r}_limb_2p20", [(a + 1, 1 << 20)])
        mut(f"r{r}_out_limb_2p20", [(a + 5, 1 << 20)])
        mut(f"r{r}_cycle_n_real", [(a, CHECK_N_REAL)])
        mut(f"r{r}_kind_4", [(a + 6, 4)])
        mut(f"r{r}_len_over", [(a + 3, (1 << 20) + 1)])
        mut(f"r{r}_out_in_code", [(a + 4, 0x17F0), (a + 5, 0)])
        mut(f"r{r}_count_plus", [(a + 7, int(base[a + 7]) + 1)])
        mut(f"r{r}_count_minus", [(a + 7, int(base[a + 7]) - 1)])
        mut(f"r{r}_piece_2p16", [(a + 8 + 5 * 2 + 3, 0x10000)])
        mut(f"r{r}_told_after", [(a + 8 + 5 * 1, int(base[a]) + 1)])
    mut("r1_cycle_not_above", [(at[1], int(base[at[0]]))])
    mut("r2_cycle_below", [(at[2], 15)])
    mut("r0_sha_out_misaligned", [(at[0] + 4, 0x3002)])
    mut("cut_in_last_cells", [], cut=len(base) - 7)
    mut("cut_in_last_header", [], cut=at[2] + 5)
    mut("cut_at_last_record", [], cut=at[2])
    mut("count_word_4", [(0, 4)])
    mut("count_above_n_real", [(0, CHECK_N_REAL + 1)])
    # two faults in different records: the lowest record's code
    mut("two_r0_code_r2_piece", [(at[0] + 4, 0x17F0), (at[0] + 5, 0), (at[2] + 8 + 3, 0x10000)])
    mut("two_r1_piece_r2_code", [(at[1] + 8 + 3, 0x10000), (at[2] + 4, 0x17F0), (at[2] + 5, 0)])
    mut("two_r0_kind_cut", [(at[0] + 6, 7)], cut=len(base) - 3)
    mut("two_r1_code_cut", [(at[1] + 4, 0x1000), (at[1] + 5, 0)], cut=len(base) - 3)
    return out


def expected_check_code(words, n_real=CHECK_N_REAL, code_end=CHECK_CODE_END):
    """hashcall::parse_section's result, by its specification (hashcall.h), in Python"""
    w = [int(x) for x in words]
    if len(w) < 1:
        return 4
    if w[0] > n_real:
        return 56
    q, prev = 1, None
    for k in range(w[0]):
        if q + 8 > len(w):
            return 4
        c = w[q:q + 8]
        if max(c[1], c[2], c[4], c[5]) >= 1 << 20:
            return 56
        cycle, in_ptr, length, out_ptr, kind = c[0], c[1] | (c[2] << 20), c[3], c[4] | (c[5] << 20), c[6]
        in_range = kind in (3, 5, 6) and (kind != 3 or out_ptr % 4 == 0) and length <= 1 << 20 and in_ptr + length <= 1 << 40 and out_ptr + 32 <= 1 << 40
        if cycle >= n_real or (prev is not None and cycle <= prev) or not in_range:
            return 56
        if out_ptr < code_end and out_ptr + 32 > 0x1000:
            return 55
        n = len(cells_of(in_ptr, length, out_ptr))
        if c[7] != n:
            return 56
        if q + 8 + 5 * n > len(w):
            return 4
        q += 8
        for _ in range(n):
            if max(w[q + 1:q + 5]) > 0xFFFF or w[q] > cycle:
                return 56
            q += 5
        prev = cycle
    return 0
