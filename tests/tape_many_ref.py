"""The reference and the corpora for a mode-4 proof's tape stages over a LIST of proofs (zkir_tape_sections_stage_*, zkir_verify_many_tapes_*,
zkir_verify_rate_many_tapes_*): per pair of sections the verdicts are hashcall::parse_section's by its specification (tests/tape_side_ref.py: expected_check_code) and the
wide record rules written out below, the chunk digests the oracle's (so.hash_elems), the bytes every call wrote tests/tape_digest_ref.py's (the oracle's three hash
functions), the two sums tests/tape_side_ref.py's Python integers — and a batch's answer is the list of its pairs' answers: nothing of one proof may reach another.
Nothing here is computed by the product.  The expected verdict of every proof is the single-proof host verifier's."""
import functools

import numpy as np

import tape_digest_ref as D
import tape_side_ref as R
import test_gpu_verify_device as tv
import test_prove_rate_modes_verify as RM
from oracle import api as oracle, stark_api as so
from zkir_amd import stark

P = so.P
EMPTY = R.EMPTY


# ---- the list stage ------------------------------------------------------------------------------------------------------------------------------------------------------
def wide_verdict(words, n_real):
    """the wide tape's checks (verify.cpp: 57) on [n] + 8 n words"""
    w = [int(x) for x in words]
    if w[0] > n_real:
        return 57
    for k in range(w[0]):
        c = w[1 + 8 * k:9 + 8 * k]
        if max(c[1], c[2], c[4], c[5]) >= 1 << 20 or max(c[3], c[6]) >= 1 << 24 or not 3 <= c[7] <= 7:
            return 57
        if c[0] >= n_real or (k and c[0] <= w[1 + 8 * (k - 1)]) or (c[7] >= 4 and not (c[4] | c[5] | c[6])):
            return 57
    return 0


def chunk_digests(words):
    w = np.ascontiguousarray(words, dtype=np.uint32)
    return [[int(x) for x in so.hash_elems(w[at:at + 512])] for at in range(0, len(w), 512)]


@functools.lru_cache(maxsize=None)
def _pair_ref(hs_bytes, ws_bytes, n_real, code_end, alpha, lam):
    hs, ws = np.frombuffer(hs_bytes, np.uint32), np.frombuffer(ws_bytes, np.uint32)
    hv, wv = R.expected_check_code(hs, n_real, code_end), wide_verdict(ws, n_real)
    zeros = lambda n: [[0, 0, 0, 0]] * ((n + 511) // 512)  # noqa: E731
    dg = (chunk_digests(hs) if hv == 0 else zeros(len(hs)), chunk_digests(ws) if wv == 0 else zeros(len(ws)))
    sums = [[0, 0, 0, 0], [0, 0, 0, 0]]
    if hv == 0 and wv == 0:
        sums = [R.reference(hs, D.expected_new_bytes(hs), EMPTY, list(alpha), list(lam))["sum"], R.reference(EMPTY, [], ws, list(alpha), list(lam))["sum"]]
    return hv, wv, dg, sums


def stage_ref(hash_secs, wide_secs, n_real, code_end, alphas, lams):
    """(hash verdicts, wide verdicts, digests per pair ([chunks][4], [chunks][4]), sums [n][2][4]) — zero where the entries return zero"""
    out = [_pair_ref(np.ascontiguousarray(h, np.uint32).tobytes(), np.ascontiguousarray(w, np.uint32).tobytes(), int(nr), int(ce), tuple(a), tuple(l))
           for h, w, nr, ce, a, l in zip(hash_secs, wide_secs, n_real, code_end, alphas, lams)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], [o[3] for o in out]


def challenge(seed):
    """a canonical E4 nobody derived from the data, another one per seed"""
    rng = np.random.default_rng(2000 + seed)
    return [int(x) for x in rng.integers(0, P, 4)]


def batch(pairs, n_real=1 << 22, code_end=0x1800, seed=0):
    """(hash_secs, wide_secs, n_real, code_end, alphas, lams) over the given (hash words, wide words) pairs, ANOTHER alpha and lambda per pair; n_real and code_end: one
    value for all, or one per pair"""
    n = len(pairs)
    per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n  # noqa: E731
    return ([np.ascontiguousarray(h, np.uint32) for h, _ in pairs], [np.ascontiguousarray(w, np.uint32) for _, w in pairs], per(n_real), per(code_end),
            [challenge(2 * i + 100 * seed) for i in range(n)], [challenge(2 * i + 1 + 100 * seed) for i in range(n)])


def assert_stage(got, want, what=""):
    ghv, gwv, gd, gs = got
    whv, wwv, wd, ws = want
    assert list(ghv) == list(whv), (what, "hash verdicts", list(ghv), list(whv))
    assert list(gwv) == list(wwv), (what, "wide verdicts", list(gwv), list(wwv))
    for i, (a, b) in enumerate(zip(gd, wd)):
        for which in (0, 1):
            assert np.asarray(a[which], dtype=np.int64).reshape(-1, 4).tolist() == np.asarray(b[which], dtype=np.int64).reshape(-1, 4).tolist(), (what, "digests of pair", i, which)
    assert np.asarray(gs, dtype=np.int64).tolist() == np.asarray(ws, dtype=np.int64).tolist(), (what, "sums")


def one_call(k, cycle=None):
    """a one-call tape; kind, length and both alignments vary with k"""
    kind = (3, 5, 6)[k % 3]
    return D.fast_tape([(3 + k if cycle is None else cycle, 0x2000 + 64 * k + k % 8, 20 + (k * 7) % 50, 0x400000 + 64 * k + (4 * (k % 2) if kind == 3 else (3 * k + 1) % 8), kind)], seed=100 + k)


def wide_of(n, first_cycle=1, seed=5):
    rng = np.random.default_rng(seed + n)
    return R.make_wide([(first_cycle + 3 * k, int(rng.integers(1, 1 << 62)) * 4 + k % 4, int(rng.integers(1, 1 << 62)) * 2 + 1, 3 + k % 5) for k in range(n)])


def offsets(words):
    """where the records of a well-formed hash section start"""
    at, q = [], 1
    for _ in range(int(words[0])):
        at.append(q); q += 8 + 5 * int(words[q + 7])
    return at


def padded_to(n_words):
    """a well-formed hash section of EXACTLY n_words words: a record is 8 + 5 n words (n >= 4 cells), so k records hold (n_words - 1 - 8 k) / 5 cells — k - 1 calls
    of four cells (len 0, an aligned output) and one whose input (at most 1024 bytes) lies on the cells that are left"""
    for k in range(1, n_words // 28 + 1):
        rest = n_words - 1 - 8 * k
        if rest % 5 or rest // 5 < 4 * k or rest // 5 - 4 * k > 128:
            continue
        extra = rest // 5 - 4 * k
        calls = [(2 + 2 * j, 0x2000, 0, 0x30000 + 64 * j, 5) for j in range(k - 1)] + [(2 + 2 * k, 0x100000, 8 * extra, 0x200000, 6)]
        t = D.fast_tape(calls, seed=n_words)
        assert len(t) == n_words
        return t
    raise ValueError(n_words)


def designed_batches():
    """{name: batch}: the smallest shapes at which the list kernels can still go wrong (each named in tests/test_gpu_verify_many_tapes.py)"""
    out = {}
    c = [D.tape(f"calls{n}") for n in (255, 256, 257)]
    for name, order in (("calls_012", (0, 1, 2)), ("calls_210", (2, 1, 0)), ("calls_102", (1, 0, 2))):
        out[name] = batch([(c[i], EMPTY) for i in order], seed=1)
    out["one_call_x64"] = batch([(one_call(k), EMPTY) for k in range(64)], seed=2)
    out["designed_l_dev"] = batch([(D.tape("designed"), EMPTY), (D.tape("l_dev"), wide_of(3)), (D.tape("designed"), EMPTY)], seed=3)
    # the second tape's first cycle lies below the first's last one: call 0 and record 0 of a section have no predecessor
    out["no_predecessor"] = batch([(D.fast_tape([(50, 0x2000, 8, 0x3000, 3), (90, 0x2000, 8, 0x3000, 5)]), wide_of(4, first_cycle=60)), (one_call(1, cycle=7), wide_of(3, first_cycle=2))], seed=4)
    # a failing call of proof 1 in the same wave as passing calls of proofs 0 and 2
    bad = D.fast_tape([(5, 0x2000, 8, 0x3000, 3), (9, 0x2000, 8, 0x3000, 5), (12, 0x2000, 8, 0x3000, 6)]).copy()
    bad[offsets(bad)[1] + 6] = 4                                   # (call 1's kind)
    out["failing_between"] = batch([(one_call(0), EMPTY), (bad, EMPTY), (one_call(2), EMPTY)], seed=5)
    # the lowest failing call wins across workgroups inside one proof: calls 300 and 20 of calls513 fail, with different codes
    many = D.fast_tape([(1 + k, 0x2000 + 64 * k, 8, 0x400000 + 64 * k, 5) for k in range(513)], seed=7).copy()
    at = offsets(many)
    many[at[300] + 8 + 1] = 0x10000                                # (56: a piece of call 300's first cell)
    many[at[20] + 4], many[at[20] + 5] = 0x17F0, 0                 # (55: call 20's output on code bytes)
    out["lowest_wins"] = batch([(one_call(3), EMPTY), (many, EMPTY)], seed=6)
    # a header-only truncated last record among whole tapes
    t = D.fast_tape([(5, 0x2000, 8, 0x3000, 3), (9, 0x2000, 8, 0x3000, 5)])
    out["header_only"] = batch([(one_call(4), EMPTY), (t[:offsets(t)[1] + 8], EMPTY), (one_call(5), wide_of(2))], seed=7)
    out["empty_and_not"] = batch([(EMPTY, wide_of(5)), (one_call(6), EMPTY), (EMPTY, EMPTY)], seed=8)
    out["wide_sizes"] = batch([(EMPTY, wide_of(n)) for n in (1, 255, 256, 257)], seed=9)
    zero_div = wide_of(6).copy(); zero_div[1 + 8 * 2 + 4:1 + 8 * 2 + 7] = 0; zero_div[1 + 8 * 2 + 7] = 4
    bad_op = wide_of(6).copy(); bad_op[1 + 8 * 5 + 7] = 8
    out["wide_failing"] = batch([(EMPTY, wide_of(6)), (EMPTY, zero_div), (one_call(7), wide_of(7)), (EMPTY, bad_op), (EMPTY, wide_of(6))], seed=10)
    out["ragged_chunks"] = batch([(padded_to(512), wide_of(2)), (padded_to(513), EMPTY), (padded_to(1023), wide_of(64)), (one_call(8), EMPTY)], seed=11)
    return out


WANT_VERDICTS = {"failing_between": ([0, 56, 0], [0, 0, 0]), "lowest_wins": ([0, 55], [0, 0]), "header_only": ([0, 4, 0], [0, 0, 0]),
                 "wide_failing": ([0, 0, 0, 0, 0], [0, 57, 0, 57, 0]), "no_predecessor": ([0, 0], [0, 0])}


# ---- the corpora of proofs -----------------------------------------------------------------------------------------------------------------------------------------------
def pub_c(pub):
    return RM.pub_c(pub)


@functools.lru_cache(maxsize=None)
def oracle_mode4(name):
    """(proof, public inputs) of a mode-4 oracle proof of tests/tape_side_ref.py's real_program(name)"""
    blob, ins, cfg = R.real_program(name)
    ores = oracle.run(blob, list(ins), enable_execution_trace=True, **cfg)
    pub = so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code), wide_mode=True)
    return so.prove(ores.rows, pub), pub_c(pub)


def records(proof, rate=False):
    """the hash calls plus wide records of a proof's tapes by its count words (0: not mode 4)"""
    if int(proof[9]) != 4:
        return 0
    lay = stark.rate_proof_layout(proof) if rate else stark.proof_layout(proof)
    return int(proof[lay["hash_section"]]) + int(proof[lay["wide_section"]])


@functools.lru_cache(maxsize=None)
def honest_corpus():
    """[(what, proof, public inputs)]: mode-4 oracle proofs of sha256_hello, hashes_all, blake3_multi_chunk (a call above 1024 bytes: a patch), signed_division_loop (wide
    arithmetic) and wide_and_hash, and fib30 in modes 0, 3 and 4 (mode 4 with both tapes empty)"""
    out = [(f"{name} mode 4", *oracle_mode4(name)) for name in ("sha256_hello", "hashes_all", "blake3_multi_chunk", "signed_division_loop", "wide_and_hash")]
    for what, mode in (("fib30 mode 0", {}), ("fib30 mode 3", {"mem_mode": True}), ("fib30 mode 4", {"wide_mode": True})):
        out.append((what, *tv._oracle_case("fib30", **mode)))
    return out


@functools.lru_cache(maxsize=None)
def mutants():
    """test_gpu_verify_device.mutations(): [(what, proof)] with the honest proof first"""
    return tv.mutations()


@functools.lru_cache(maxsize=None)
def forged():
    """[(case, proof, the oracle's verdict)]: the eight forged hash tapes of test_gpu_verify_device.FORGED, rebuilt as that file does"""
    M, pub, cells, hs, rec = tv._chain()
    out = []
    for case, want in tv.FORGED.items():
        t = hs.copy()
        if case == "message bit":
            t[rec + 8 + 5 * 1 + 1] ^= 1
        elif case == "length":
            t[rec + 3] = int(t[rec + 3]) - 1
        elif case == "kind":
            t[rec + 6] = 5
        elif case == "future time":
            t[rec + 8] = int(t[rec]) + 1
        elif case == "earlier time":
            t[rec + 8] = int(t[rec + 8]) - 1
        elif case == "dropped record":
            t = np.concatenate([[int(hs[0]) - 1], hs[1:rec], hs[rec + 48:]]).astype(np.uint32)
        elif case == "order":
            t[rec] = int(t[rec - 48])
        so.set_hash_calls(t)
        try:
            pr = so.prove_matrix_mem(M, pub, cells)
        finally:
            so.set_hash_calls(None)
        out.append((case, pr, want))
    return out


RATE_MUTATION_SEED = 0      # chosen with the host verifier alone (rt.verify_rate on a CPU, seeds 0, 1, ..: the first whose codes on the mutants include 10, 56 and 57)
RATE_MUTATION_CODES = {10, 56, 57}      # the host's codes on it (the frozen proof has hash calls AND wide records).  A 'ZKSR' front has no grinding before check 10:
                                        # a changed byte of a touched cell, or a changed operand of a wide record, reaches the check itself through the tape's share alone


@functools.lru_cache(maxsize=None)
def rate_corpus(seed=None):
    """[(what, proof, public inputs, min_queries, min_pow_bits)]: the frozen mode-4 'ZKSR' proof and ~40 single-word mutants of its tape sections (count words among them)"""
    rng = np.random.default_rng(RATE_MUTATION_SEED if seed is None else seed)
    proof, opub, rows, b, nq, bits = RM.golden("mode4")
    pub = RM.pub_c(opub)
    lay = stark.rate_proof_layout(proof)
    lo, hi = lay["hash_section"], lay["rom_mult"]
    out = [("mode4 honest", proof, pub, nq, bits)]
    for trial in range(40):
        pos = lo + (0 if trial == 0 else int(rng.integers(0, hi - lo)))
        old = int(proof[pos])
        new = [0, 1, 8, 0x1000, 1 << 16, 1 << 20, P - 1, (old + 1) % P, (old + 8) % P][int(rng.integers(0, 9))]
        if new == old:
            continue
        t = proof.copy(); t[pos] = new
        out.append((f"mode4 word {pos}: {old} -> {new}", t, pub, nq, bits))
    return out
