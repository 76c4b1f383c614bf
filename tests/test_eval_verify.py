"""zkir_eval_verify / zkir_eval_proof_words without a GPU, against tests/eval_ref.py: the reference's evaluations against an independent route (interpolation and Horner),
both verifiers on reference proofs and on a family of mutants (same code from both), false claims, word counts."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import eval_ref as ev
import lowdeg_ref as ld
from oracle import stark_api as so
from zkir_amd import runtime as rt

P = ld.P
# (log_n, b, width, n_points, num_queries, pow_bits): three distinct schedules, final sizes 8, 16, 32, ragged widths, both point counts
SHAPES = [(3, 1, 3, 1, 3, 4), (5, 2, 5, 2, 4, 3), (6, 3, 9, 2, 3, 4)]
EDGES = [0, 1, 1 << 16, (1 << 20) - 1, 1 << 24, (1 << 30) + 1, P - 1, P, 1 << 31, 0xFFFFFFFF]


def points_for(seed: int, n_points: int) -> np.ndarray:
    return np.random.default_rng(5000 + seed).integers(1, P, (n_points, 4), dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def matrix(log_n: int, b: int, width: int) -> np.ndarray:
    rng = np.random.default_rng(2000 * log_n + 20 * b + width)
    out = np.stack([so.lde(c, b)[1] for c in rng.integers(0, P, (width, 1 << log_n), dtype=np.uint32)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def proof(shape) -> np.ndarray:
    log_n, b, width, n_points, nq, bits = shape
    pr = ev.prove_ref(matrix(log_n, b, width), b, points_for(log_n, n_points), nq, bits)
    pr.setflags(write=False)
    return pr


def expectations(t, pr):
    """(root, points, evals) of the honest proof `pr`, as far as they can be held against the mutant `t`: the library reads as many expected words as t's header states"""
    at = ev.layout(pr)
    same = len(t) >= 9 and int(t[4]) == at["width"] and int(t[5]) == at["n_points"]
    return pr[at["root"]:at["root"] + 4], pr[at["points"]:at["evals"]] if same else None, pr[at["evals"]:at["layer_roots"]] if same else None


def both(t, root=None, points=None, evals=None) -> int:
    """the product's verdict, which must be the reference's"""
    got, want = rt.eval_verify(t, root, points, evals), ev.verify_ref(t, root, points, evals)
    assert got == want, f"zkir_eval_verify says {got}, the reference {want}"
    return got


def eval_mutants(pr, rng):
    """[(label, words)] modelled on the low-degree proof's family: header words at edges, the point and evaluation words, query words, cuts at every section boundary,
    extensions, bumps, words >= p, swaps and zeroed runs"""
    at = ev.layout(pr)
    n = len(pr)
    out = []

    def put(label, pos, val):
        t = pr.copy(); t[pos] = val & 0xFFFFFFFF
        out.append((label, t))
    for pos in range(9):                                             # magic, version, log_n, b, width, n_points, num_queries, pow_bits, n_layers
        for v in EDGES + [int(pr[pos]) + 1, max(int(pr[pos]) - 1, 0), 2, 3, 4, 24, 25, 26, 27, 128, 129, 512, 513]:
            put(f"header{pos}={v}", pos, v)
    for i in range(at["n_points"]):                                  # a point pushed into the base field, made the other point, a coordinate at the edges
        p0 = at["points"] + 4 * i
        t = pr.copy(); t[p0 + 1:p0 + 4] = 0
        out.append((f"point{i} in the base field", t))
        t = pr.copy(); t[p0:p0 + 4] = [0, 0, 0, 0]
        out.append((f"point{i} zero", t))
        for c in range(4):
            for v in (0, 1, P - 1, P, 0xFFFFFFFF, int(pr[p0 + c]) + 1):
                put(f"point{i}.{c}={v}", p0 + c, v)
    if at["n_points"] == 2:
        for a, b in ((0, 1), (1, 0)):
            t = pr.copy(); t[at["points"] + 4 * a:at["points"] + 4 * a + 4] = pr[at["points"] + 4 * b:at["points"] + 4 * b + 4]
            out.append((f"point{a} = point{b}", t))
    for pos in [at["evals"], at["evals"] + 3, at["layer_roots"] - 1] + [int(x) for x in rng.integers(at["evals"], at["layer_roots"], 4)]:
        for v in (0, P - 1, P, (int(pr[pos]) + 1) % P, (int(pr[pos]) + P - 1) % P):
            put(f"eval@{pos}={v}", pos, v)
    starts = [at["queries"] + t * at["qsize"] for t in range(at["num_queries"])]
    for s in starts:                                                 # the query index words
        for v in EDGES + [int(pr[s]) ^ 1, int(pr[s]) + (1 << (at["log_n"] + at["b"] - 1))]:
            put(f"query@{s}={v}", s, v)
    bounds = [9, 13, at["evals"], at["layer_roots"], at["final"], at["nonce"], at["queries"]] + starts + [starts[0] + 1 + at["rec"], starts[0] + at["layers"][0][0],
                                                                                                          starts[0] + at["layers"][0][1], n]
    for b in bounds:
        for cut in (b - 1, b, b + 1):
            if 0 <= cut <= n:
                out.append((f"cut{cut}", pr[:cut].copy()))
    for cut in rng.integers(0, n, 8):
        out.append((f"cut{cut}", pr[:int(cut)].copy()))
    for extra in (1, 3, 32):
        out.append((f"extend{extra}", np.concatenate([pr, rng.integers(0, P, extra).astype(np.uint32)])))
    for pos in [9, 12, at["layer_roots"], at["final"], at["final"] + 4 * at["n_fin"] - 1, at["nonce"], starts[0] + 1, starts[0] + at["layers"][0][0], starts[0] + at["layers"][0][0] + 5,
                starts[0] + at["layers"][0][1], starts[-1] + at["layers"][0][0], starts[-1] + at["layers"][-1][0], starts[-1] + at["layers"][-1][1], n - 1] + [int(x) for x in rng.integers(13, n, 20)]:
        put(f"word{pos}+1", pos, (int(pr[pos]) + 1) % P)
    for pos in rng.integers(0, n, 8):
        put(f"word{pos}>=p", int(pos), [P, P + 1, 0xFFFFFFFF][int(pos) % 3])
    for _ in range(8):
        a, b = (int(x) for x in rng.integers(9, n, 2))
        t = pr.copy(); t[a], t[b] = t[b], t[a]
        out.append((f"swap{a},{b}", t))
        a = int(rng.integers(9, n))
        t = pr.copy(); t[a:a + int(rng.integers(1, 40))] = 0
        out.append((f"zero{a}", t))
    return [(label, t) for label, t in out if not (len(t) == n and np.array_equal(t, pr))]


# ---- the reference's evaluations: an independent route -----------------------------------------------------------------------------------------------------------------
def _horner(coeffs, z) -> np.ndarray:
    acc = np.zeros((1, 4), np.uint64)
    for c in coeffs[::-1]:
        acc = ld.e_mul(acc, z)
        acc[0, 0] = (acc[0, 0] + np.uint64(int(c))) % np.uint64(P)
    return acc[0]


@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
def test_evaluate_is_the_interpolants_value(log_n):
    """for true extensions, the barycentric sums over the sub-coset equal Horner in E4 on the coefficients of the N trace values (a plain inverse DFT in Python integers),
    at every rate"""
    N = 1 << log_n
    rng = np.random.default_rng(log_n)
    trace = rng.integers(0, P, (3, N), dtype=np.uint32)
    w_inv, n_inv = pow(ld.root_of_unity(log_n), P - 2, P), pow(N, P - 2, P)
    coeffs = [[sum(int(col[j]) * pow(w_inv, j * k, P) for j in range(N)) * n_inv % P for k in range(N)] for col in trace]
    pts = np.array([[5, 7, 11, 13], [P - 1, P - 2, P - 3, P - 4], [0, 1, 0, 0]], np.uint32)
    want = np.array([[_horner(c, z) for c in coeffs] for z in pts], np.uint64)
    for b in (1, 2, 3):
        cols = np.stack([so.lde(col, b)[1] for col in trace])
        assert np.array_equal(ev.evaluate(cols, b, pts), want), (log_n, b)


def test_e_inv_is_the_oracles():
    a = np.random.default_rng(3).integers(0, P, (16, 4), dtype=np.uint32)
    a[0] = [0, 1, 0, 0]; a[1] = [P - 1, 0, 0, P - 1]
    got = ev.e_inv(a)
    for x, y in zip(a, got):
        assert np.array_equal(so.einv(x), y.astype(np.uint32))
        assert np.array_equal(ld.e_mul(x.reshape(1, 4), y.reshape(1, 4))[0], [1, 0, 0, 0])


# ---- both verifiers --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_shapes_have_distinct_schedules():
    assert len({tuple(ld.schedule(s[0], s[1])) for s in SHAPES}) == 3


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_proofs_are_accepted_by_both(shape):
    log_n, b, width, n_points, nq, bits = shape
    pr = proof(shape)
    assert rt.eval_proof_words(log_n, b, width, n_points, nq) == len(pr) == ev.proof_words(log_n, b, width, n_points, nq)
    root, pts, ys = expectations(pr, pr)
    assert np.array_equal(root, so.merkle(matrix(log_n, b, width))) and np.array_equal(pts, points_for(log_n, n_points).reshape(-1))
    assert np.array_equal(ys.reshape(n_points, width, 4), ev.evaluate(matrix(log_n, b, width), b, points_for(log_n, n_points)))
    assert both(pr) == 0 and both(pr, root) == 0 and both(pr, root, pts, ys) == 0 and both(pr, None, pts) == 0 and both(pr, None, None, ys) == 0
    # what the caller expects and the proof does not state
    wrong = root.copy(); wrong[1] ^= 1
    assert both(pr, wrong, pts, ys) == 2
    wrong = pts.copy(); wrong[-1] ^= 1
    assert both(pr, root, wrong, ys) == 13 and both(pr, None, wrong) == 13
    wrong = ys.copy(); wrong[0] ^= 1
    assert both(pr, root, pts, wrong) == 13 and both(pr, None, None, wrong) == 13
    with pytest.raises(ValueError):
        rt.eval_verify(pr, None, pts[:-1])
    with pytest.raises(ValueError):
        rt.eval_verify(pr, None, None, np.concatenate([ys, ys]))


@pytest.mark.parametrize("shape", SHAPES)
def test_mutants_get_the_same_code_from_both(shape):
    pr = proof(shape)
    rng = np.random.default_rng(77 + shape[0])
    codes = {}
    for i, (label, t) in enumerate(eval_mutants(pr, rng)):
        root, pts, ys = expectations(t, pr)
        code = both(t, *[(None, None, None), (root, None, None), (root, pts, ys), (None, pts, ys)][i % 4])
        assert code != 0, f"a mutant is accepted: {label}"
        codes[code] = codes.get(code, 0) + 1
    print(shape, dict(sorted(codes.items())))
    assert len(codes) >= 5 and {8, 12, 13} <= set(codes), codes


@pytest.mark.parametrize("shape", SHAPES)
def test_named_rejections(shape):
    """the codes a mutant family meets by chance, met on purpose"""
    log_n, b, width, n_points, nq, bits = shape
    pr = proof(shape)
    at = ev.layout(pr)
    t = pr.copy(); t[at["points"] + 1:at["points"] + 4] = 0
    assert both(t) == 12                                             # a point in the base field
    t = pr.copy(); t[at["points"]] = P
    assert both(t) == 3                                              # a point word >= p is a range error before the point is looked at
    if n_points == 2:
        t = pr.copy(); t[at["points"] + 4:at["points"] + 8] = t[at["points"]:at["points"] + 4]
        assert both(t) == 12                                         # two equal points
    p0 = at["queries"]
    v0, path0, depth0 = at["layers"][0]
    for where in (p0 + v0, p0 + v0 + 3, p0 + v0 + 4, p0 + v0 + 7):
        t = pr.copy(); t[where] = (int(t[where]) + 1) % P
        assert both(t) == 8, where                                   # a layer-0 value is not F at its row: checked before the leaf's path
    t = pr.copy(); t[p0 + path0] = (int(t[p0 + path0]) + 1) % P
    assert both(t) == 9
    t = pr.copy(); t[p0 + 1] = (int(t[p0 + 1]) + 1) % P
    assert both(t) == 7
    t = pr.copy(); t[at["final"]] = (int(t[at["final"]]) + 1) % P
    assert both(t) == 4
    for word, bad in [(2, 2), (3, 0), (3, 4), (4, 0), (4, 513), (5, 0), (5, 3), (6, 0), (6, 129), (7, 25), (8, int(pr[8]) + 1)]:
        t = pr.copy(); t[word] = bad
        assert both(t) == 1, (word, bad)
    assert both(pr[:-1]) == 1 and both(pr[:8]) == 1 and both(pr[:0]) == 1 and both(np.concatenate([pr, pr[:1]])) == 1


# ---- false claims ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_a_false_claim_is_refused(shape):
    """evaluations that are honest for ANOTHER point, and evaluations with one word off by one: the prover follows the honest procedure from there (eval_ref.prove_ref's
    `evals`), and F is no polynomial of degree < N; and the same changes made to a finished proof."""
    log_n, b, width, n_points, nq, bits = shape
    m, pts = matrix(log_n, b, width), points_for(log_n, n_points)
    other = pts.copy(); other[0, 2] = (int(other[0, 2]) + 1) % P
    y = ev.evaluate(m, b, pts)
    off = y.copy(); off[-1, width // 2, 3] = (off[-1, width // 2, 3] + np.uint64(1)) % np.uint64(P)
    for claim in (ev.evaluate(m, b, other), off):
        pr = ev.prove_ref(m, b, pts, nq, bits, evals=claim)
        code = ev.verify_ref(pr)
        assert code != 0 and both(pr) == code
        assert code == 4                                             # a pole of F at z does not fold away: the final layer is not of degree < 4
    pr = proof(shape)
    at = ev.layout(pr)
    t = pr.copy(); t[at["evals"] + 4 * (width - 1) + 1] = (int(t[at["evals"] + 4 * (width - 1) + 1]) + 1) % P
    code = ev.verify_ref(t)
    assert code != 0 and both(t) == code
    t = pr.copy(); t[at["points"] + 2] = (int(t[at["points"] + 2]) + 1) % P
    code = ev.verify_ref(t)
    assert code != 0 and both(t) == code


def test_proof_words_of_bad_parameters_is_zero():
    for args in [(2, 1, 8, 1, 4), (27, 1, 8, 1, 4), (3, 0, 8, 1, 4), (3, 4, 8, 1, 4), (25, 3, 8, 1, 4), (3, 1, 0, 1, 4), (3, 1, 513, 1, 4), (3, 1, 8, 1, 0), (3, 1, 8, 1, 129),
                 (3, 1, 8, 0, 4), (3, 1, 8, 3, 4)]:
        assert rt.eval_proof_words(*args) == 0 == ev.proof_words(*args), args
    for args in [(26, 1, 512, 2, 128), (24, 3, 1, 1, 1), (10, 2, 152, 2, 25)]:
        assert rt.eval_proof_words(*args) == ev.proof_words(*args) > 0
    assert ev.proof_words(10, 2, 152, 2, 25) == ld.proof_words(10, 2, 152, 25) + 1 + 4 * 2 * 153
