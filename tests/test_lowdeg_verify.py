"""zkir_lowdeg_verify / zkir_lowdeg_proof_words without a GPU, against tests/lowdeg_ref.py: the reference itself anchored on the oracle's FRI layers, acceptance over every
schedule class, every rejection code named, and a soundness smoke (a matrix that is NOT low-degree is refused)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import lowdeg_ref as ld
from oracle import api as oracle, stark_api as so
from zkir_amd import runtime as rt, spec

P = ld.P
# (log_n, b, width, num_queries, pow_bits): schedules [1], [1], [1,1], [1,2], [1,3], [1,3,1]; final sizes 8, 16, 32; ragged widths; zero grinding
SHAPES = [(3, 1, 1, 3, 0), (3, 3, 8, 2, 4), (4, 2, 9, 4, 4), (5, 3, 8, 3, 0), (6, 1, 5, 5, 6), (7, 2, 17, 4, 4)]


@functools.lru_cache(maxsize=None)
def _matrix(log_n: int, b: int, width: int) -> np.ndarray:
    rng = np.random.default_rng(1000 * log_n + 10 * b + width)
    cols = rng.integers(0, P, (width, 1 << log_n), dtype=np.uint32)
    out = np.stack([so.lde(c, b)[1] for c in cols])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _proof(shape) -> np.ndarray:
    log_n, b, width, nq, bits = shape
    pr = ld.prove_ref(_matrix(log_n, b, width), b, nq, bits)
    pr.setflags(write=False)
    return pr


def _both(proof, root=None) -> int:
    """the product's verdict, which must be the reference's"""
    got, want = rt.lowdeg_verify(proof, root), ld.verify_ref(proof, root)
    assert got == want, f"zkir_lowdeg_verify says {got}, the reference {want}"
    return got


def test_schedules_cover_the_classes():
    assert [ld.schedule(s[0], s[1]) for s in SHAPES] == [[1], [1], [1, 1], [1, 2], [1, 3], [1, 3, 1]]
    assert ld.schedule(5, 1) == [1, 2] and ld.schedule(20, 3) == [1, 3, 3, 3, 3, 3, 2]
    assert sorted({4 << s[1] for s in SHAPES}) == [8, 16, 32]


# ---- the reference's own anchor: the oracle's FRI layers of a mode-0 proof (b = 1) ------------------------------------------------------------------
def test_reference_fold_trees_and_challenger_are_the_oracles():
    """lowdeg_ref.fold maps the oracle's FRI layer j to its layer j + 1 for every j, and lowdeg_ref.layer_tree gives the layer roots of the oracle's proof.  The oracle hands
    out alpha, zeta and gamma (so.last_challenges) but not its betas: lowdeg_ref.Challenger replays the mode-0 transcript from the proof's own words (verify.cpp lists the
    order), has to arrive at the oracle's three challenges, and goes on to the betas."""
    blob = spec.fib_endless_program().to_bytes()
    res = oracle.run(blob, max_cycles=50, enable_execution_trace=True)
    pub = so.public_inputs(len(res.rows), blob, [], list(res.outputs), (res.halt_kind, res.halt_code))
    pr = so.prove(res.rows, pub)
    assert so.verify(pr, pub) == 0
    alpha, zeta, gamma = so.last_challenges()
    log_n = so.padded_log_n(len(res.rows))
    assert log_n == 6
    ks = ld.schedule(log_n, 1)
    assert ks == [1, 3]
    lay = so.proof_layout(pr)
    wt = int(pr[3]) + so.W_AUX
    ch = ld.Challenger()
    ch.observe_n(pr[2:so.HEADER_WORDS])
    ch.observe_n(pr[lay["trace_root"]:lay["trace_root"] + 4])
    ch.observe_n(pr[lay["rom_mult"]:lay["rom_mult"] + lay["n_rom"]])
    ch.observe_n(pr[lay["rc_mult"]:lay["rc_mult"] + so.RC_TABLE])
    ch.sample_ext(); ch.sample_ext()                                 # the lookup argument's two challenges
    ch.observe_n(pr[lay["aux_root"]:lay["aux_root"] + 4])
    assert np.array_equal(ch.sample_ext(), alpha)
    ch.observe_n(pr[lay["quotient_root"]:lay["quotient_root"] + 4])
    assert np.array_equal(ch.sample_ext(), zeta)
    ch.observe_n(pr[lay["t_z"]:lay["t_z"] + 4 * (2 * wt + 4)])
    assert np.array_equal(ch.sample_ext(), gamma)
    at = lay["q_z"] + 16
    assert int(pr[at]) == len(ks)
    layers = [so.last_fri_layer(j).astype(np.uint64) for j in range(len(ks) + 1)]
    assert [len(x) for x in layers] == [128, 64, 8]
    shift, log_m = ld.GEN, log_n + 1
    for j, k in enumerate(ks):
        root, _ = ld.layer_tree(layers[j], k)
        assert np.array_equal(root, pr[at + 1 + 4 * j:at + 5 + 4 * j]), f"layer {j}: root"
        ch.observe_n(root)
        nxt, shift = ld.fold(layers[j], k, shift, log_m, ch.sample_ext())
        log_m -= k
        assert np.array_equal(nxt, layers[j + 1]), f"layer {j}: fold"
    assert shift == pow(ld.GEN, 16, P) and log_m == 3
    fin = at + 1 + 4 * len(ks)
    assert np.array_equal(pr[fin:fin + 32], layers[-1].astype(np.uint32).reshape(-1))
    ch.observe_n(pr[fin:fin + 32])
    assert ch.grind(so.lib().so_pow_bits()) == int(pr[fin + 32]) and ch.check_pow(int(pr[fin + 32]), so.lib().so_pow_bits())


def test_reference_combine_and_transcript_pieces():
    """combine against a direct sum with so.emul; the Challenger's grind gives the smallest nonce check_pow takes"""
    m = _matrix(3, 3, 8)
    gamma = np.array([5, 7, 11, 13], np.uint32)
    c = ld.combine(m, gamma)
    g, want = np.array([1, 0, 0, 0], np.uint32), np.zeros(4, np.uint64)
    for k in range(8):
        want = (want + g.astype(np.uint64) * np.uint64(m[k, 37])) % np.uint64(P)
        g = so.emul(g, gamma)
    assert np.array_equal(c[37], want)
    ch = ld.Challenger(); ch.observe_n([1, 2, 3])
    nonce = ch.grind(6)
    for lower in range(nonce + 1):
        c2 = ld.Challenger(); c2.observe_n([1, 2, 3])
        assert c2.check_pow(lower, 6) == (lower == nonce)


# ---- acceptance -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_proofs_are_accepted(shape):
    log_n, b, width, nq, bits = shape
    pr = _proof(shape)
    assert rt.lowdeg_proof_words(log_n, b, width, nq) == len(pr) == ld.proof_words(log_n, b, width, nq)
    assert ld.verify_ref(pr) == 0 and rt.lowdeg_verify(pr) == 0
    root = so.merkle(_matrix(log_n, b, width))
    assert np.array_equal(pr[8:12], root) and _both(pr, root) == 0
    # the matrix records are opening records of the root
    at = ld.layout(pr)
    M = 1 << (log_n + b)
    for t in range(nq):
        p0 = at["queries"] + t * at["qsize"]
        q = int(pr[p0])
        idx = np.array([q, q + M // 2], np.uint64)
        v, s = rt.merkle_verify_host(root, width, M, idx, pr[p0 + 1:p0 + 1 + 2 * at["rec"]])
        assert not v.any()


def test_proof_words_of_bad_parameters_is_zero():
    for args in [(2, 1, 8, 4), (27, 1, 8, 4), (3, 0, 8, 4), (3, 4, 8, 4), (25, 3, 8, 4), (3, 1, 0, 4), (3, 1, 513, 4), (3, 1, 8, 0), (3, 1, 8, 129)]:
        assert rt.lowdeg_proof_words(*args) == 0 == ld.proof_words(*args), args
    assert rt.lowdeg_proof_words(26, 1, 512, 128) == ld.proof_words(26, 1, 512, 128) > 0
    assert rt.lowdeg_proof_words(24, 3, 1, 1) == ld.proof_words(24, 3, 1, 1) > 0


def test_proof_words_over_every_size_and_rate():
    """The one schedule and the one query-words function (fri_shape.h) against the reference's, at every (log_n, b) a proof can state: arithmetic only."""
    n = 0
    for log_n in range(3, 27):
        for b in range(1, 4):
            if log_n + b > 27:
                continue
            assert rt.lowdeg_proof_words(log_n, b, 8, 4) == ld.proof_words(log_n, b, 8, 4) > 0, (log_n, b)
            n += 1
    assert n == 24 + 23 + 22


# ---- rejection: every code, the product's verdict = the reference's = the one named -------------------------------------------------------------------
def _bump(pr, at, d=1):
    t = pr.copy()
    t[at] = (int(t[at]) + d) % P
    return t


@pytest.mark.parametrize("shape", SHAPES)
def test_malformed_root_and_range(shape):
    pr = _proof(shape)
    at = ld.layout(pr)
    assert _both(pr[:-1]) == 1 and _both(np.concatenate([pr, np.zeros(1, np.uint32)])) == 1 and _both(pr[:11]) == 1 and _both(pr[:0]) == 1
    for d in (1, P - 1):
        assert _both(_bump(pr, 7, d)) == 1                           # n_layers off by one
    for word in (0, 1):
        assert _both(_bump(pr, word)) == 1                           # magic, version
    for word, bad in [(2, 2), (2, 27), (3, 0), (3, 4), (4, 0), (4, 513), (5, 0), (5, 129), (6, 25)]:
        t = pr.copy(); t[word] = bad
        assert _both(t) == 1, (word, bad)
    t = pr.copy(); t[4] = P                                          # a header word >= p is a range error first
    assert _both(t) == 1
    assert _both(pr, _bump(pr[8:12], 2)) == 2                        # not the expected root
    t = pr.copy(); t[9] = P
    assert _both(t, pr[8:12]) == 2                                   # .. which is compared before the canonical scan
    # a word >= p in every section
    p0 = at["queries"] + (at["num_queries"] - 1) * at["qsize"]
    v0, path0, _ = at["layers"][0]
    v1, path1, _ = at["layers"][-1]
    for where in [8, 11, 12, at["final"] - 1, at["final"], at["nonce"] - 1, at["nonce"], p0, p0 + 1, p0 + at["width"], p0 + 1 + at["width"], p0 + at["rec"], p0 + 2 * at["rec"],
                  p0 + v0, p0 + path0, p0 + v1 + 3, p0 + path1, len(pr) - 1]:
        for bad in (P, 0xFFFFFFFF):
            t = pr.copy(); t[where] = bad
            assert _both(t) == 3, (where, bad)


@pytest.mark.parametrize("shape", SHAPES)
def test_final_layer_grinding_and_queries(shape):
    log_n, b, width, nq, bits = shape
    pr = _proof(shape)
    at = ld.layout(pr)
    for where in (at["final"], at["final"] + 4 * at["n_fin"] - 1, at["final"] + 6):
        assert _both(_bump(pr, where)) == 4                          # a final-layer word + 1: one value off a word of degree < 4 over >= 8 points
    if bits:
        d = next(d for d in range(1, 64) if ld.verify_ref(_bump(pr, at["nonce"], d)) == 5)      # nonce + d where that nonce fails (d = 1 but for a 2^-bits chance)
        assert d <= 2 and _both(_bump(pr, at["nonce"], d)) == 5
    else:
        assert _both(_bump(pr, at["nonce"])) in (0, 6)               # no grinding: every nonce passes, but the queries are drawn after it
    last = nq - 1
    for t in (0, last):
        p0 = at["queries"] + t * at["qsize"]
        assert _both(_bump(pr, p0)) == 6                             # the index word
        tq = pr.copy(); tq[p0] ^= 1
        assert _both(tq) == 6
        for where in (p0 + 1, p0 + width, p0 + 1 + width, p0 + at["rec"], p0 + 1 + at["rec"], p0 + 1 + at["rec"] + width + 5, p0 + 2 * at["rec"]):
            assert _both(_bump(pr, where)) == 7, where               # a row word / a path word of record(q), of record(q + M/2)
        v0, path0, depth0 = at["layers"][0]
        for where in (p0 + v0, p0 + v0 + 3, p0 + v0 + 4, p0 + v0 + 7):
            assert _both(_bump(pr, where)) == 8, where               # a layer-0 value: the equality with the rows is checked before the leaf's path
        for where in (p0 + path0, p0 + path0 + 4 * depth0 - 1):
            assert _both(_bump(pr, where)) == 9, where               # layer 0's path
        for v_at, p_at, depth in at["layers"][1:]:
            for where in (p0 + p_at, p0 + p_at + 4 * depth - 1):
                assert _both(_bump(pr, where)) == 9, where           # a later layer's path
            assert _both(_bump(pr, p0 + v_at)) == 9                  # .. and a later layer's value alone: its leaf no longer hashes to the path
    # lowest query first: a path word of query 0 (9) wins over the index word of the last query (6)
    if nq > 1:
        t = _bump(_bump(pr, at["queries"] + last * at["qsize"]), at["queries"] + at["layers"][0][1])
        assert _both(t) == 9


@pytest.mark.parametrize("shape", SHAPES)
def test_layers_that_are_not_the_fold(shape):
    """A prover that commits, honestly, to a layer that is NOT the fold of the one before (every value + 1: still a low-degree word, so the final check passes): the leaf and
    its path are consistent, the carried value is not — 10 at a middle layer, 11 at the final one."""
    log_n, b, width, nq, bits = shape
    n_layers = len(ld.schedule(log_n, b))

    def plus_one(which):
        def hook(j, layer):
            if j != which:
                return layer
            out = layer.copy(); out[:, 0] = (out[:, 0] + np.uint64(1)) % np.uint64(P)
            return out
        return hook
    m = _matrix(log_n, b, width)
    for j in range(1, n_layers):
        assert _both(ld.prove_ref(m, b, nq, bits, layer_hook=plus_one(j))) == 10, j
    assert _both(ld.prove_ref(m, b, nq, bits, layer_hook=plus_one(n_layers))) == 11


# ---- soundness smoke: a committed matrix that is not a low-degree extension ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 2, 9, 4, 4), (6, 1, 5, 5, 6), (5, 3, 8, 3, 0)])
def test_matrices_that_are_not_low_degree_are_refused(shape):
    """The honest procedure over a matrix with ONE value of one extended column changed, and over one with a column of M random words: the error survives every fold (a
    one-point error folds to a one-point error; a cancellation has probability ~2^-124 over beta) and the final layer is not of degree < 4."""
    log_n, b, width, nq, bits = shape
    M = 1 << (log_n + b)
    m = _matrix(log_n, b, width).copy()
    m[width // 2, M // 3] = (int(m[width // 2, M // 3]) + 1) % P
    pr = ld.prove_ref(m, b, nq, bits)
    assert ld.verify_ref(pr) == 4 and rt.lowdeg_verify(pr) == 4
    m = _matrix(log_n, b, width).copy()
    m[width - 1] = np.random.default_rng(7).integers(0, P, M, dtype=np.uint32)
    pr = ld.prove_ref(m, b, nq, bits)
    assert ld.verify_ref(pr) == 4 and rt.lowdeg_verify(pr) == 4
    # a codeword that is not the combination of the committed rows (the matrix itself is honest): layer 0 does not match the rows
    m = _matrix(log_n, b, width)
    gamma_free = ld.combine(m, np.array([1, 2, 3, 4], np.uint32))     # low-degree, but for another gamma than the transcript's
    assert _both(ld.prove_ref(m, b, nq, bits, codeword=gamma_free)) == 8
