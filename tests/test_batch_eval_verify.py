"""zkir_batch_eval_verify / zkir_batch_eval_proof_words without a GPU, against tests/batch_eval_ref.py: both verifiers on reference proofs and on mutants of every check
(same code from both), expectations that do not match, the two identities of the codeword, word counts."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import batch_eval_ref as be
import eval_ref as ev
import lowdeg_ref as ld
from oracle import stark_api as so
from zkir_amd import runtime as rt

P = ld.P
# (log_n, b, ((width, mask), ..), n_points, num_queries, pow_bits): one matrix of one column at one point; blow-up 8 with a matrix opened at the first point only;
# three matrices, ragged widths, one opened at the second point only
SHAPES = [(3, 1, ((1, 1),), 1, 3, 4), (3, 3, ((8, 0b11), (1, 0b01)), 2, 3, 3), (4, 2, ((9, 0b11), (7, 0b01), (8, 0b10)), 2, 3, 4)]
EDGES = [0, 1, 1 << 16, (1 << 20) - 1, 1 << 24, (1 << 30) + 1, P - 1, P, 1 << 31, 0xFFFFFFFF]


def points_for(seed: int, n_points: int) -> np.ndarray:
    return np.random.default_rng(6000 + seed).integers(1, P, (n_points, 4), dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def matrix(log_n: int, b: int, width: int, m: int) -> np.ndarray:
    rng = np.random.default_rng(3000 * log_n + 30 * b + 7 * width + m)
    out = np.stack([so.lde(c, b)[1] for c in rng.integers(0, P, (width, 1 << log_n), dtype=np.uint32)])
    out.setflags(write=False)
    return out


def matrices(shape):
    log_n, b, wm = shape[:3]
    return [matrix(log_n, b, w, m) for m, (w, _) in enumerate(wm)]


@functools.lru_cache(maxsize=None)
def proof(shape) -> np.ndarray:
    log_n, b, wm, n_points, nq, bits = shape
    pr = be.prove_ref(matrices(shape), b, [k for _, k in wm], points_for(log_n, n_points), nq, bits)
    pr.setflags(write=False)
    return pr


def expectations(t, pr):
    """(roots, points, evals) of the honest proof `pr`, as far as they can be held against the mutant `t`: the library reads as many expected words as t's header states"""
    at = be.layout(pr)
    n = 9 + 2 * at["n_mats"]
    same = len(t) >= n and np.array_equal(t[4:6], pr[4:6]) and np.array_equal(t[9:n], pr[9:n])
    if not same:
        return None, None, None
    return pr[at["roots"]:at["points"]], pr[at["points"]:at["evals"]], pr[at["evals"]:at["layer_roots"]]


def both(t, roots=None, points=None, evals=None) -> int:
    """the product's verdict, which must be the reference's"""
    got, want = rt.batch_eval_verify(t, roots, points, evals), be.verify_ref(t, roots, points, evals)
    assert got == want, f"zkir_batch_eval_verify says {got}, the reference {want}"
    return got


def batch_mutants(pr, rng):
    """[(label, words)]: each header word at edges, every width / mask word, a root of each matrix, the points, an evaluation of each matrix, the layer roots, final words, the
    nonce, q, a record word (row and path) of each matrix at both rows, layer values, path words, cuts at every section boundary, extensions, words >= p, swaps, zeroed runs"""
    at = be.layout(pr)
    n = len(pr)
    out = []

    def put(label, pos, val):
        t = pr.copy(); t[pos] = val & 0xFFFFFFFF
        out.append((label, t))

    def bump(label, pos):
        put(f"{label}@{pos}+1", pos, (int(pr[pos]) + 1) % P)
    for pos in range(9):                                             # magic, version, log_n, b, n_mats, n_points, num_queries, pow_bits, n_layers
        for v in EDGES + [int(pr[pos]) + 1, max(int(pr[pos]) - 1, 0), 2, 3, 4, 5, 24, 25, 26, 27, 128, 129]:
            put(f"header{pos}={v}", pos, v)
    for m in range(at["n_mats"]):
        for v in (0, 1, 8, 511, 512, 513, at["widths"][m] + 1, at["widths"][m] - 1, P, 0xFFFFFFFF):
            put(f"width{m}={v}", at["shape"] + 2 * m, v)
        for v in (0, 1, 2, 3, 4, 7, P, 0xFFFFFFFF):
            put(f"mask{m}={v}", at["shape"] + 2 * m + 1, v)
        for c in (0, 3):
            bump(f"root{m}", at["roots"] + 4 * m + c)
        put(f"root{m}>=p", at["roots"] + 4 * m + 1, P)
    for i in range(at["n_points"]):                                  # a point pushed into the base field, made the other point, a coordinate at the edges
        p0 = at["points"] + 4 * i
        t = pr.copy(); t[p0 + 1:p0 + 4] = 0
        out.append((f"point{i} in the base field", t))
        t = pr.copy(); t[p0:p0 + 4] = [0, 0, 0, 0]
        out.append((f"point{i} zero", t))
        t = pr.copy(); t[p0:p0 + 4] = [P - 1, 0, 0, 0]
        out.append((f"point{i} = -1", t))
        for c in range(4):
            for v in (0, P - 1, P, 0xFFFFFFFF, int(pr[p0 + c]) + 1):
                put(f"point{i}.{c}={v}", p0 + c, v)
    if at["n_points"] == 2:
        for a, b in ((0, 1), (1, 0)):
            t = pr.copy(); t[at["points"] + 4 * a:at["points"] + 4 * a + 4] = pr[at["points"] + 4 * b:at["points"] + 4 * b + 4]
            out.append((f"point{a} = point{b}", t))
    for (i, m), pos in at["evals_of"].items():                       # an evaluation of every selected (point, matrix): its first and its last word
        for where in (pos, pos + 4 * at["widths"][m] - 1):
            for v in (0, P - 1, P, (int(pr[where]) + 1) % P):
                put(f"eval({i},{m})@{where}={v}", where, v)
    for j in range(len(at["ks"])):
        bump("layer root", at["layer_roots"] + 4 * j + j % 4)
    for pos in (at["final"], at["final"] + 5, at["nonce"] - 1):
        bump("final", pos)
    for v in (0, int(pr[at["nonce"]]) + 1, P - 1, P):
        put(f"nonce={v}", at["nonce"], v)
    starts = [at["queries"] + t * at["qsize"] for t in range(at["num_queries"])]
    for s in starts:                                                 # the query index words
        for v in EDGES + [int(pr[s]) ^ 1, int(pr[s]) + (1 << (at["log_n"] + at["b"] - 1))]:
            put(f"query@{s}={v}", s, v)
    for s in (starts[0], starts[-1]):
        for m in range(at["n_mats"]):                                # a record of every matrix: a row word and a path word, at q and at q + M/2
            for r0 in at["records"][m]:
                bump(f"record{m} row", s + r0)
                bump(f"record{m} row", s + r0 + at["widths"][m] - 1)
                bump(f"record{m} path", s + r0 + at["widths"][m])
                bump(f"record{m} path", s + r0 + at["recs"][m] - 1)
        for v_at, p_at, depth in at["layers"]:
            bump("layer value", s + v_at); bump("layer value", s + v_at + 7)
            if depth:
                bump("layer path", s + p_at); bump("layer path", s + p_at + 4 * depth - 1)
    bounds = [9, at["roots"], at["points"], at["evals"], at["layer_roots"], at["final"], at["nonce"], at["queries"]] + starts + \
             [starts[0] + r for rs in at["records"] for r in rs] + [starts[0] + at["layers"][0][0], starts[0] + at["layers"][0][1], n]
    for b in bounds:
        for cut in (b - 1, b, b + 1):
            if 0 <= cut <= n:
                out.append((f"cut{cut}", pr[:cut].copy()))
    for cut in rng.integers(0, n, 8):
        out.append((f"cut{cut}", pr[:int(cut)].copy()))
    for extra in (1, 3, 32):
        out.append((f"extend{extra}", np.concatenate([pr, rng.integers(0, P, extra).astype(np.uint32)])))
    for pos in rng.integers(at["roots"], n, 20):
        bump("word", int(pos))
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


# ---- the reference's own identities ----------------------------------------------------------------------------------------------------------------------------------------
def test_one_matrix_with_a_full_mask_is_the_evaluation_proofs_codeword():
    cols, pts = matrix(4, 2, 9, 0), points_for(4, 2)
    gamma = np.array([3, P - 1, 7, 11], np.uint32)
    y = be.evaluate([cols], 2, [3], pts)
    assert np.array_equal(y.reshape(2, 9, 4), ev.evaluate(cols, 2, pts))
    assert np.array_equal(be.quotient([cols], [3], pts, y, gamma), ev.quotient(cols, 2, pts, y, gamma))
    assert np.array_equal(be.quotient([cols], [1], pts[:1], y[:9], gamma), ev.quotient(cols, 2, pts[:1], y[:9], gamma))


def test_a_split_at_a_multiple_of_eight_columns_leaves_the_codeword_unchanged():
    cols, pts = np.concatenate([matrix(4, 2, 9, 0), matrix(4, 2, 7, 1), matrix(4, 2, 8, 2)]), points_for(4, 2)
    gamma = np.array([5, 6, P - 2, 1], np.uint32)
    y = be.evaluate([cols], 2, [3], pts).reshape(2, 24, 4)
    whole = be.quotient([cols], [3], pts, y, gamma)
    for cut in (8, 16):
        y2 = np.concatenate([y[0, :cut], y[0, cut:], y[1, :cut], y[1, cut:]])
        assert np.array_equal(be.quotient([cols[:cut], cols[cut:]], [3, 3], pts, y2, gamma), whole)


# ---- both verifiers --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_proofs_are_accepted_by_both(shape):
    log_n, b, wm, n_points, nq, bits = shape
    widths, masks = [w for w, _ in wm], [k for _, k in wm]
    pr = proof(shape)
    assert rt.batch_eval_proof_words(log_n, b, widths, masks, n_points, nq) == len(pr) == be.proof_words(log_n, b, widths, masks, n_points, nq)
    roots, pts, ys = expectations(pr, pr)
    assert np.array_equal(roots, np.concatenate([so.merkle(c) for c in matrices(shape)])) and np.array_equal(pts, points_for(log_n, n_points).reshape(-1))
    assert np.array_equal(ys.reshape(-1, 4), be.evaluate(matrices(shape), b, masks, points_for(log_n, n_points)))
    assert both(pr) == 0 and both(pr, roots) == 0 and both(pr, roots, pts, ys) == 0 and both(pr, None, pts) == 0 and both(pr, None, None, ys) == 0
    # what the caller expects and the proof does not state: a root of EACH matrix, a point, an evaluation of each matrix
    for m in range(len(wm)):
        wrong = roots.copy(); wrong[4 * m + 1] ^= 1
        assert both(pr, wrong, pts, ys) == 2
    wrong = pts.copy(); wrong[-1] ^= 1
    assert both(pr, roots, wrong, ys) == 13 and both(pr, None, wrong) == 13
    at = be.layout(pr)
    for pos in at["evals_of"].values():
        wrong = ys.copy(); wrong[pos - at["evals"]] ^= 1
        assert both(pr, roots, pts, wrong) == 13 and both(pr, None, None, wrong) == 13
    with pytest.raises(ValueError):
        rt.batch_eval_verify(pr, roots[:-4])
    with pytest.raises(ValueError):
        rt.batch_eval_verify(pr, None, np.concatenate([pts, pts]))
    with pytest.raises(ValueError):
        rt.batch_eval_verify(pr, None, None, ys[:-4])


@pytest.mark.parametrize("shape", SHAPES)
def test_mutants_get_the_same_code_from_both(shape):
    pr = proof(shape)
    rng = np.random.default_rng(177 + shape[0])
    codes = {}
    for i, (label, t) in enumerate(batch_mutants(pr, rng)):
        roots, pts, ys = expectations(t, pr)
        code = both(t, *[(None, None, None), (roots, None, None), (roots, pts, ys), (None, pts, ys)][i % 4])
        assert code != 0, f"a mutant is accepted: {label}"
        codes[code] = codes.get(code, 0) + 1
    print(shape, dict(sorted(codes.items())))
    assert {1, 2, 3, 5, 6, 7, 8, 9, 12, 13} <= set(codes), codes


@pytest.mark.parametrize("shape", SHAPES)
def test_named_rejections(shape):
    """every check met on purpose, with the code it must give"""
    log_n, b, wm, n_points, nq, bits = shape
    pr = proof(shape)
    at = be.layout(pr)
    n_mats = len(wm)
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
    for m in range(n_mats):                                          # a record of ANY matrix is a 7, at either row, in its row words and in its path
        for r0 in at["records"][m]:
            for where in (p0 + r0, p0 + r0 + at["widths"][m]):
                t = pr.copy(); t[where] = (int(t[where]) + 1) % P
                assert both(t) == 7, (m, where)
        t = pr.copy(); t[at["roots"] + 4 * m] = (int(t[at["roots"] + 4 * m]) + 1) % P
        assert both(t) != 0 and both(t, pr[at["roots"]:at["points"]]) == 2
    for (i, m), pos in at["evals_of"].items():                       # a changed evaluation of any matrix changes gamma and a_i: refused, and a 13 for who expects the true one
        t = pr.copy(); t[pos + 2] = (int(t[pos + 2]) + 1) % P
        assert both(t) != 0 and both(t, None, None, pr[at["evals"]:at["layer_roots"]]) == 13
    t = pr.copy(); t[at["final"]] = (int(t[at["final"]]) + 1) % P
    assert both(t) == 4
    t = pr.copy(); t[at["nonce"]] = (int(t[at["nonce"]]) + 1) % P
    assert both(t) in (5, 6)                                         # (another nonce may pass the grinding by chance: then the queries differ)
    t = pr.copy(); t[p0] ^= 1
    assert both(t) == 6
    for word, bad in [(2, 2), (3, 0), (3, 4), (4, 0), (4, 5), (4, n_mats + 1), (5, 0), (5, 3), (6, 0), (6, 129), (7, 25), (8, int(pr[8]) + 1)]:
        t = pr.copy(); t[word] = bad
        assert both(t) == 1, (word, bad)
    for m in range(n_mats):                                          # a width, a mask
        for bad in (0, 513, at["widths"][m] + 1):
            t = pr.copy(); t[at["shape"] + 2 * m] = bad
            assert both(t) == 1, (m, bad)
        for bad in (0, 1 << n_points, 7):
            t = pr.copy(); t[at["shape"] + 2 * m + 1] = bad
            assert both(t) == 1, (m, bad)
    if n_points == 2:                                                # a point no matrix is opened at: every mask 1
        t = pr.copy(); t[at["shape"] + 1:at["roots"]:2] = 1
        assert both(t) == 1
    assert both(pr[:-1]) == 1 and both(pr[:8]) == 1 and both(pr[:9]) == 1 and both(pr[:0]) == 1 and both(np.concatenate([pr, pr[:1]])) == 1


def test_widths_summing_above_512_are_malformed():
    """a header no proof can have, at a length that would match it: code 1 before anything is read past the shape words"""
    for widths, masks in (([512, 1], [1, 1]), ([256, 256, 1], [3, 3, 3]), ([128, 128, 128, 129], [1, 2, 3, 3])):
        assert rt.batch_eval_proof_words(3, 1, widths, masks, 2 if max(masks) > 1 else 1, 3) == 0 == be.proof_words(3, 1, widths, masks, 2 if max(masks) > 1 else 1, 3)
        n_points = 2 if max(masks) > 1 else 1
        head = [be.MAGIC, 1, 3, 1, len(widths), n_points, 3, 0, 1] + [x for wk in zip(widths, masks) for x in wk]
        assert both(np.array(head + [0] * 4000, np.uint32)) == 1
    assert rt.batch_eval_proof_words(3, 1, [512], [1], 1, 3) > 0 and rt.batch_eval_proof_words(3, 1, [256, 256], [3, 3], 2, 3) > 0


# ---- false claims ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES[1:])
def test_a_false_claim_about_any_matrix_is_refused(shape):
    """evaluations with one word of ONE matrix off by one: the prover follows the honest procedure from there, and F is no polynomial of degree < N"""
    log_n, b, wm, n_points, nq, bits = shape
    mats, masks, pts = matrices(shape), [k for _, k in wm], points_for(log_n, n_points)
    y = be.evaluate(mats, b, masks, pts)
    at = be.layout(proof(shape))
    for (i, m), pos in at["evals_of"].items():
        off = y.copy()
        e = (pos - at["evals"]) // 4 + wm[m][0] - 1
        off[e, 3] = (off[e, 3] + np.uint64(1)) % np.uint64(P)
        pr = be.prove_ref(mats, b, masks, pts, nq, bits, evals=off)
        code = be.verify_ref(pr)
        assert code == 4 and both(pr) == code, (i, m)                # a pole of F at z does not fold away: the final layer is not of degree < 4


def test_proof_words():
    for args in [(2, 1, [8], [1], 1, 4), (27, 1, [8], [1], 1, 4), (3, 0, [8], [1], 1, 4), (3, 4, [8], [1], 1, 4), (25, 3, [8], [1], 1, 4), (3, 1, [0], [1], 1, 4), (3, 1, [513], [1], 1, 4),
                 (3, 1, [8], [1], 1, 0), (3, 1, [8], [1], 1, 129), (3, 1, [8], [1], 0, 4), (3, 1, [8], [1], 3, 4), (3, 1, [8], [0], 1, 4), (3, 1, [8], [2], 1, 4), (3, 1, [8], [1], 2, 4),
                 (3, 1, [8, 8], [1, 1], 2, 4), (3, 1, [8, 8], [2, 2], 2, 4), (3, 1, [8, 8], [3, 4], 2, 4), (3, 1, [1] * 5, [1] * 5, 1, 4), (3, 1, [], [], 1, 4)]:
        assert rt.batch_eval_proof_words(*args) == 0 == be.proof_words(*args), args
    for args in [(26, 1, [128] * 4, [3] * 4, 2, 128), (24, 3, [1], [1], 1, 1), (10, 2, [152, 40, 4], [3, 3, 1], 2, 25), (10, 2, [1, 1, 1, 1], [1, 2, 3, 3], 2, 25)]:
        assert rt.batch_eval_proof_words(*args) == be.proof_words(*args) > 0
    # one matrix with a full mask: the evaluation proof's words, two more for the (width, mask) pair
    assert be.proof_words(10, 2, [152], [3], 2, 25) == ev.proof_words(10, 2, 152, 2, 25) + 2


def test_proof_words_over_every_size_and_rate():
    """One fixed batch shape at every (log_n, b) a proof can state: the count follows the one schedule and the one query-words function (fri_shape.h)."""
    for log_n in range(3, 27):
        for b in range(1, 4):
            if log_n + b <= 27:
                assert rt.batch_eval_proof_words(log_n, b, [8, 3], [3, 1], 2, 4) == be.proof_words(log_n, b, [8, 3], [3, 1], 2, 4) > 0, (log_n, b)
