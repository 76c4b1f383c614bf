"""zkir_mixed_eval_verify / zkir_mixed_eval_proof_words without a GPU, against tests/mixed_eval_ref.py: the schedule over every pair and triple of heights, both verifiers
on reference proofs and on mutants of every section (same code from both), the named rejections of the lower groups, word counts against separate batched proofs."""
from __future__ import annotations

import functools
import itertools

import numpy as np
import pytest

import batch_eval_ref as be
import lowdeg_ref as ld
import mixed_eval_ref as mx
from oracle import stark_api as so
from zkir_amd import runtime as rt

P = ld.P
# (log_ns, b, per group (((width, mask), ..), n_points), num_queries, pow_bits)
SHAPES = [
    ((4, 3), 1, ((((1, 1),), 1), (((1, 1),), 1)), 3, 3),
    ((5, 4), 1, ((((3, 0b11), (2, 0b01)), 2), (((2, 1),), 1)), 3, 3),
    ((6, 3), 2, ((((9, 1),), 1), (((3, 0b10), (1, 0b01)), 2)), 3, 4),
    ((8, 4), 1, ((((8, 0b11),), 2), (((5, 0b11),), 2)), 3, 3),
    ((7, 5, 3), 1, ((((9, 3), (7, 1)), 2), (((8, 2), (1, 3)), 2), (((5, 1),), 1)), 3, 4),
    ((5, 3), 3, ((((4, 1),), 1), (((2, 1), (2, 1)), 1)), 3, 3),
]
KNOWN_KS = {((5, 4), 1): [1, 2], ((6, 3), 2): [1, 2, 1], ((7, 5, 3), 1): [1, 1, 2, 1], ((5, 3), 3): [1, 1, 1], ((8, 4), 1): [1, 3, 2]}


def shapes_of(shape):
    """[(widths, masks, n_points)] of a SHAPES entry"""
    return [([w for w, _ in wm], [k for _, k in wm], n) for wm, n in shape[2]]


@functools.lru_cache(maxsize=None)
def matrix(log_n: int, b: int, width: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(5000 * log_n + 50 * b + 9 * width + seed)
    out = np.stack([so.lde(c, b)[1] for c in rng.integers(0, P, (width, 1 << log_n), dtype=np.uint32)])
    out.setflags(write=False)
    return out


def points_for(seed: int, n_points: int) -> np.ndarray:
    return np.random.default_rng(8000 + seed).integers(1, P, (n_points, 4), dtype=np.uint32)


def groups_of(shape):
    """mixed_eval_ref's groups of a SHAPES entry: (mats, masks, points) per group"""
    log_ns, b = shape[:2]
    return [([matrix(log_n, b, w, 10 * h + m) for m, w in enumerate(widths)], masks, points_for(100 * h + log_n, n))
            for h, (log_n, (widths, masks, n)) in enumerate(zip(log_ns, shapes_of(shape)))]


@functools.lru_cache(maxsize=None)
def proof(shape) -> np.ndarray:
    pr = mx.prove_ref(groups_of(shape), shape[1], shape[3], shape[4])
    pr.setflags(write=False)
    return pr


def expectations(t, pr):
    """(roots, points, evals) of the honest proof `pr`, as far as they can be held against the mutant `t`: the library reads as many expected words as t's header states"""
    at = mx.layout(pr)
    if rt.mixed_eval_sizes(t) != rt.mixed_eval_sizes(pr):
        return None, None, None
    return pr[at["roots"]:at["points"]], pr[at["points"]:at["evals"]], pr[at["evals"]:at["layer_roots"]]


def both(t, roots=None, points=None, evals=None) -> int:
    """the product's verdict, which must be the reference's"""
    got, want = rt.mixed_eval_verify(t, roots, points, evals), mx.verify_ref(t, roots, points, evals)
    assert got == want, f"zkir_mixed_eval_verify says {got}, the reference {want}"
    return got


def bumped(pr, pos):
    t = pr.copy(); t[pos] = (int(t[pos]) + 1) % P
    return t


def mixed_mutants(pr, rng):
    """[(label, words)]: one flipped word in every section, in every record and every layer of a query, in group 0 and in the lower groups; header and group words at their
    edges; cuts and extensions; swapped groups, equal heights, n_groups 1 and 4; a mask leaving a point unused in a lower group; words = p"""
    at = mx.layout(pr)
    n, G = len(pr), at["groups"]
    out = []

    def put(label, pos, val):
        t = pr.copy(); t[pos] = val & 0xFFFFFFFF
        out.append((label, t))

    def bump(label, pos):
        out.append((f"{label}@{pos}+1", bumped(pr, pos)))
    for pos in range(7):                                             # magic, version, b, n_groups, num_queries, pow_bits, n_layers
        for v in [0, 1, 2, 3, 4, 5, 24, 25, 128, 129, P, 0xFFFFFFFF, int(pr[pos]) + 1, max(int(pr[pos]) - 1, 0)]:
            put(f"header{pos}={v}", pos, v)
    for h, g in enumerate(G):
        for v in (2, 3, 26, 27, g["log_n"] + 1, g["log_n"] - 1, P):
            put(f"group{h} log_n={v}", g["shape"], v)
        for v in (0, 5, len(g["widths"]) + 1, len(g["widths"]) - 1):
            put(f"group{h} n_mats={v}", g["shape"] + 1, v)
        for v in (0, 3, 3 - g["n_points"]):
            put(f"group{h} n_points={v}", g["shape"] + 2, v)
        for m in range(len(g["widths"])):
            for v in (0, 513, g["widths"][m] + 1, P):
                put(f"group{h} width{m}={v}", g["shape"] + 3 + 2 * m, v)
            for v in (0, 1, 2, 3, 4, P):
                put(f"group{h} mask{m}={v}", g["shape"] + 4 + 2 * m, v)
            bump(f"group{h} root{m}", g["roots"] + 4 * m + m % 4)
            put(f"group{h} root{m}=p", g["roots"] + 4 * m + 1, P)
        if g["n_points"] == 2:                                       # every mask 1: the second point of the group is opened by no matrix
            t = pr.copy(); t[g["shape"] + 4:g["shape"] + 3 + 2 * len(g["widths"]):2] = 1
            out.append((f"group{h}: a point unused", t))
            t = pr.copy(); t[g["points"] + 4:g["points"] + 8] = t[g["points"]:g["points"] + 4]
            out.append((f"group{h}: equal points", t))
        for i in range(g["n_points"]):
            p0 = g["points"] + 4 * i
            t = pr.copy(); t[p0 + 1:p0 + 4] = 0
            out.append((f"group{h} point{i} in the base field", t))
            bump(f"group{h} point{i}", p0 + i)
            put(f"group{h} point{i}=p", p0 + 2, P)
        for (i, m), pos in g["evals_of"].items():
            for where in (pos, pos + 4 * g["widths"][m] - 1):
                bump(f"group{h} eval({i},{m})", where)
            put(f"group{h} eval({i},{m})=p", pos + 1, P)
    if len(G) == 2 and len(G[0]["widths"]) == len(G[1]["widths"]):  # the two groups' log_n swapped: heights rising
        t = pr.copy(); t[G[0]["shape"]], t[G[1]["shape"]] = pr[G[1]["shape"]], pr[G[0]["shape"]]
        out.append(("swapped heights", t))
    t = pr.copy(); t[G[1]["shape"]] = G[0]["log_n"]
    out.append(("equal heights", t))
    for j in range(len(at["ks"])):
        bump("layer root", at["layer_roots"] + 4 * j + j % 4)
    for pos in (at["final"], at["final"] + 5, at["nonce"] - 1):
        bump("final", pos)
    for v in (0, int(pr[at["nonce"]]) + 1, P - 1, P):
        put(f"nonce={v}", at["nonce"], v)
    starts = [at["queries"] + t * at["qsize"] for t in range(at["num_queries"])]
    for s in starts:
        for v in (0, P, 0xFFFFFFFF, int(pr[s]) ^ 1, int(pr[s]) + (1 << (G[0]["log_M"] - 1))):
            put(f"query@{s}={v}", s, v)
    for s in (starts[0], starts[-1]):
        for h, g in enumerate(G):                                    # every record of every group: a row word and a path word
            for m in range(len(g["widths"])):
                for r0 in g["records"][m]:
                    bump(f"group{h} record{m} row", s + r0)
                    bump(f"group{h} record{m} row", s + r0 + g["widths"][m] - 1)
                    bump(f"group{h} record{m} path", s + r0 + g["widths"][m])
                    bump(f"group{h} record{m} path", s + r0 + g["recs"][m] - 1)
        for v_at, p_at, depth in at["layers"]:                       # every layer of the query: a value and a path word
            bump("layer value", s + v_at); bump("layer value", s + v_at + 7)
            if depth:
                bump("layer path", s + p_at); bump("layer path", s + p_at + 4 * depth - 1)
    bounds = [7, at["roots"], at["points"], at["evals"], at["layer_roots"], at["final"], at["nonce"], at["queries"]] + starts + [g["shape"] for g in G] + \
             [starts[0] + r for g in G for rs in g["records"] for r in rs] + [starts[0] + at["layers"][0][0], n]
    for b in bounds:
        for cut in (b - 1, b, b + 1):
            if 0 <= cut <= n:
                out.append((f"cut{cut}", pr[:cut].copy()))
    for extra in (1, 3, 32):
        out.append((f"extend{extra}", np.concatenate([pr, rng.integers(0, P, extra).astype(np.uint32)])))
    for pos in rng.integers(at["roots"], n, 12):
        bump("word", int(pos))
    for pos in rng.integers(0, n, 6):
        put(f"word{pos}>=p", int(pos), [P, P + 1, 0xFFFFFFFF][int(pos) % 3])
    return [(label, t) for label, t in out if not (len(t) == n and np.array_equal(t, pr))]


# ---- the schedule ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_known_schedules():
    """The five known answers, held against the reference AND against the library's fri_mixed_schedule, which shows in two numbers of zkir_mixed_eval_proof_words: the words
    that do not depend on the queries (4 a layer root) and the words of a query (per layer 4 * 2^k values and 4 * (log_m - k) path words), both written out here from the
    KNOWN steps; and in header word 6 of a proof zkir_mixed_eval_verify accepts."""
    for (log_ns, b), ks in KNOWN_KS.items():
        assert mx.schedule(log_ns, b) == ks, (log_ns, b)
        shapes = [([2 + h], [1], 1) for h in range(len(log_ns))]
        fixed = 7 + sum(3 + 2 + 4 + 4 + 4 * (2 + h) for h in range(len(log_ns))) + 4 * len(ks) + 4 * (4 << b) + 1
        qsize, log_m = 1 + sum((1 if h else 2) * (2 + h + 4 * (log_n + b)) for h, log_n in enumerate(log_ns)), log_ns[0] + b
        for k in ks:
            qsize, log_m = qsize + 4 * (1 << k) + 4 * (log_m - k), log_m - k
        for nq in (1, 2, 7):
            assert rt.mixed_eval_proof_words(log_ns, b, shapes, nq) == fixed + nq * qsize, (log_ns, b, nq)
    for shape in SHAPES:
        if (shape[0], shape[1]) in KNOWN_KS:
            pr = proof(shape)
            assert int(pr[6]) == len(KNOWN_KS[(shape[0], shape[1])]) and rt.mixed_eval_verify(pr) == 0
            t = pr.copy(); t[6] += 1
            assert rt.mixed_eval_verify(t) == 1


def test_schedule_and_words_over_every_pair_and_triple():
    """ks[0] = 1, every k <= 3, the steps sum to log_n_0 - 2, every M_h is a committed layer's size; the C words function counts what the reference counts"""
    n = 0
    for b in (1, 2, 3):
        for r in (2, 3):
            for log_ns in itertools.combinations(range(12, 2, -1), r):
                ks = mx.schedule(log_ns, b)
                assert ks[0] == 1 and max(ks) <= 3 and sum(ks) == log_ns[0] - 2, (log_ns, b, ks)
                sizes, log_m = [], log_ns[0] + b
                for k in ks:
                    sizes.append(log_m)                              # the committed layers: the sizes before each step
                    log_m -= k
                assert log_m == 2 + b and all(x + b in sizes[1:] for x in log_ns[1:]), (log_ns, b, ks)
                shapes = [([3 + h], [1], 1) for h in range(r)]
                want = mx.proof_words(log_ns, b, shapes, 2)
                assert rt.mixed_eval_proof_words(log_ns, b, shapes, 2) == want > 0, (log_ns, b)
                n += 1
    assert n == 3 * (45 + 120)


def test_words_of_bad_shapes_are_zero():
    ok = ([5, 3], 1, [([2, 1], [3, 1], 2), ([4], [1], 1)], 3)
    assert rt.mixed_eval_proof_words(*ok) == mx.proof_words(*ok) > 0
    one = ([1], [1], 1)
    for args in [([5], 1, [one], 3), ([6, 5, 4, 3], 1, [one] * 4, 3), ([5, 5], 1, [one, one], 3), ([4, 5], 1, [one, one], 3), ([5, 4, 4], 1, [one] * 3, 3), ([5, 2], 1, [one, one], 3),
                 ([27, 3], 1, [one, one], 3), ([26, 3], 2, [one, one], 3), ([5, 3], 0, [one, one], 3), ([5, 3], 4, [one, one], 3), ([5, 3], 1, [one, one], 0), ([5, 3], 1, [one, one], 129),
                 ([5, 3], 1, [one, ([513], [1], 1)], 3), ([5, 3], 1, [one, ([0], [1], 1)], 3), ([5, 3], 1, [one, ([256, 257], [1, 1], 1)], 3), ([5, 3], 1, [one, ([1], [0], 1)], 3),
                 ([5, 3], 1, [one, ([1], [2], 1)], 3), ([5, 3], 1, [one, ([1, 1], [1, 1], 2)], 3), ([5, 3], 1, [one, ([1], [1], 0)], 3), ([5, 3], 1, [one, ([1], [1], 3)], 3),
                 ([5, 3], 1, [([1] * 5, [1] * 5, 1), one], 3), ([5, 3], 1, [([], [], 1), one], 3)]:
        assert rt.mixed_eval_proof_words(*args) == 0 == mx.proof_words(*args), args


@pytest.mark.parametrize("shape", SHAPES)
def test_mixed_words_are_below_the_separate_proofs(shape):
    log_ns, b, _, nq, _ = shape
    """by the library's two words functions, which are the reference's"""
    separate = sum(rt.batch_eval_proof_words(log_n, b, w, k, n, nq) for log_n, (w, k, n) in zip(log_ns, shapes_of(shape)))
    assert separate == sum(be.proof_words(log_n, b, w, k, n, nq) for log_n, (w, k, n) in zip(log_ns, shapes_of(shape)))
    mixed = rt.mixed_eval_proof_words(log_ns, b, shapes_of(shape), nq)
    assert 0 < mixed == mx.proof_words(log_ns, b, shapes_of(shape), nq) == len(proof(shape)) < separate


# ---- both verifiers --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_proofs_are_accepted_by_both(shape):
    log_ns, b, _, nq, _ = shape
    pr = proof(shape)
    assert rt.mixed_eval_proof_words(log_ns, b, shapes_of(shape), nq) == len(pr)
    assert mx.layout(pr)["ks"] == mx.schedule(log_ns, b) and int(pr[6]) == len(mx.schedule(log_ns, b))
    roots, pts, ys = expectations(pr, pr)
    groups = groups_of(shape)
    assert np.array_equal(roots, np.concatenate([so.merkle(c) for mats, _, _ in groups for c in mats]))
    assert np.array_equal(pts, np.concatenate([p.reshape(-1) for _, _, p in groups])) and np.array_equal(ys.reshape(-1, 4), mx.evaluate(groups, b))
    for exp in itertools.product((None, roots), (None, pts), (None, ys)):
        assert both(pr, *exp) == 0
    wrong = roots.copy(); wrong[-1] ^= 1                            # what the caller expects and the proof does not state: also of the LAST group
    assert both(pr, wrong, pts, ys) == 2
    wrong = pts.copy(); wrong[-1] ^= 1
    assert both(pr, roots, wrong, ys) == 13 and both(pr, None, wrong) == 13
    wrong = ys.copy(); wrong[-1] ^= 1
    assert both(pr, roots, pts, wrong) == 13 and both(pr, None, None, wrong) == 13
    for bad in ((roots[:-4], None, None), (None, np.concatenate([pts, pts[:4]]), None), (None, None, ys[:-4])):
        with pytest.raises(ValueError):
            rt.mixed_eval_verify(pr, *bad)


@pytest.mark.parametrize("shape", SHAPES)
def test_mutants_get_the_same_code_from_both(shape):
    pr = proof(shape)
    rng = np.random.default_rng(277 + sum(shape[0]))
    codes = {}
    for i, (label, t) in enumerate(mixed_mutants(pr, rng)):
        roots, pts, ys = expectations(t, pr)
        code = both(t, *[(None, None, None), (roots, None, None), (roots, pts, ys), (None, pts, ys)][i % 4])
        assert code != 0, f"a mutant is accepted: {label}"
        codes[code] = codes.get(code, 0) + 1
    print(shape[:2], dict(sorted(codes.items())))
    assert {1, 2, 3, 5, 6, 7, 8, 9, 12, 13} <= set(codes), codes          # (10 takes a consistent leaf with another value: the false-claim tests below)


@pytest.mark.parametrize("shape", SHAPES)
def test_named_rejections(shape):
    """every check met on purpose, in group 0 and in a lower group, with the code it must give"""
    log_ns, b, _, nq, bits = shape
    pr = proof(shape)
    at = mx.layout(pr)
    G, p0 = at["groups"], at["queries"]
    for h, g in enumerate(G):
        t = pr.copy(); t[g["points"] + 1:g["points"] + 4] = 0
        assert both(t) == 12, h                                      # a point of ANY group in the base field
        t = pr.copy(); t[g["points"]] = P
        assert both(t) == 3
        if g["n_points"] == 2:
            t = pr.copy(); t[g["points"] + 4:g["points"] + 8] = t[g["points"]:g["points"] + 4]
            assert both(t) == 12
            t = pr.copy(); t[g["shape"] + 4:g["shape"] + 3 + 2 * len(g["widths"]):2] = 1
            assert both(t) == 1                                      # a mask leaving a point unused, also in a lower group
        for m in range(len(g["widths"])):                            # a record of any matrix of any group is a 7, in its row words and in its path
            for r0 in g["records"][m]:
                for where in (p0 + r0, p0 + r0 + g["widths"][m]):
                    assert both(bumped(pr, where)) == 7, (h, m, where)
            assert both(bumped(pr, g["roots"] + 4 * m), pr[at["roots"]:at["points"]]) == 2
        for pos in g["evals_of"].values():
            t = bumped(pr, pos + 2)
            assert both(t) != 0 and both(t, None, None, pr[at["evals"]:at["layer_roots"]]) == 13
    if G[1]["n_points"] == 2:                                        # the two groups may share a point: only points WITHIN a group must differ
        assert not np.array_equal(pr[G[0]["points"]:G[0]["points"] + 4], pr[G[1]["points"]:G[1]["points"] + 4])
    v0, path0, _ = at["layers"][0]
    for where in (p0 + v0, p0 + v0 + 3, p0 + v0 + 4, p0 + v0 + 7):
        assert both(bumped(pr, where)) == 8, where
    assert both(bumped(pr, p0 + path0)) == 9
    for j in range(1, len(at["ks"])):                                # a later layer's first value: its leaf no longer hashes to the root
        assert both(bumped(pr, p0 + at["layers"][j][0])) == 9, j
    assert both(bumped(pr, at["final"])) == 4
    assert both(bumped(pr, at["nonce"])) in (5, 6)
    t = pr.copy(); t[p0] ^= 1
    assert both(t) == 6
    for word, bad in [(0, mx.MAGIC + 1), (1, 2), (2, 0), (2, 4), (3, 1), (3, 4), (4, 0), (4, 129), (5, 25), (6, int(pr[6]) + 1), (6, int(pr[6]) - 1)]:
        t = pr.copy(); t[word] = bad
        assert both(t) == 1, (word, bad)
    t = pr.copy(); t[G[1]["shape"]] = G[0]["log_n"]
    assert both(t) == 1                                              # equal heights
    t = pr.copy(); t[G[0]["shape"]], t[G[1]["shape"]] = pr[G[1]["shape"]], pr[G[0]["shape"]]
    assert both(t) == 1                                              # heights rising
    assert both(pr[:-1]) == 1 and both(pr[:6]) == 1 and both(pr[:7]) == 1 and both(pr[:0]) == 1 and both(np.concatenate([pr, pr[:1]])) == 1


# ---- false claims ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[4]])
def test_a_false_evaluation_with_the_honest_procedure_after_it_is_refused(shape):
    """One evaluation word of ANY group off by one (`evals=`), the prover honest from there: its F_h has a pole at the point, the layer it enters is no low-degree word and
    the final layer is not of degree < 4.  The verifier meets that check first (4 stands before the queries in the order of checks)."""
    log_ns, b, _, nq, bits = shape
    groups = groups_of(shape)
    y = mx.evaluate(groups, b)
    for h, g in enumerate(mx.layout(proof(shape))["groups"]):
        off = y.copy()
        e = g["first_e"] + g["n_evals"] - 1
        off[e, 3] = (off[e, 3] + np.uint64(1)) % np.uint64(P)
        assert both(mx.prove_ref(groups, b, nq, bits, evals=off)) == 4, h


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[4]])
def test_a_false_evaluation_over_the_true_codewords_is_an_8_in_group_0_and_a_10_below(shape):
    """The prover STATES one false evaluation (`evals=`: the transcript and gamma are the false statement's) and follows the honest procedure from there over the codewords
    of the true values (`quotient_evals=`), which are low-degree: the final layer, the grinding, the index and every record pass.  The verifier recomputes F_h from the
    records and the stated values: in group 0 the layer-0 values are not F_0 (8); in a lower group the value carried into the layer of size M_h is not that layer's (10)."""
    log_ns, b, _, nq, bits = shape
    groups = groups_of(shape)
    y = mx.evaluate(groups, b)
    for h, g in enumerate(mx.layout(proof(shape))["groups"]):
        off = y.copy()
        off[g["first_e"], 0] = (off[g["first_e"], 0] + np.uint64(1)) % np.uint64(P)
        assert both(mx.prove_ref(groups, b, nq, bits, evals=off, quotient_evals=y)) == (8 if h == 0 else 10), h


def test_a_lower_matrix_that_is_not_low_degree_is_proven_into_a_refused_proof():
    """group 1's matrix with one word changed after the extension: its column is no polynomial of degree < N_1, its F_1 neither, and the sum of the layer does not fold to a
    final layer of degree < 4"""
    shape = SHAPES[1]
    groups = groups_of(shape)
    mats, masks, pts = groups[1]
    bad = mats[0].copy(); bad[0, 5] = (int(bad[0, 5]) + 1) % P
    pr = mx.prove_ref([groups[0], ([bad] + list(mats[1:]), masks, pts)], shape[1], shape[3], shape[4])
    assert both(pr) == 4
    mats0, masks0, pts0 = groups[0]                                  # .. and the same in group 0
    bad = mats0[1].copy(); bad[1, 9] = (int(bad[1, 9]) + 1) % P
    assert both(mx.prove_ref([([mats0[0], bad], masks0, pts0), groups[1]], shape[1], shape[3], shape[4])) == 4


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[4]])
def test_a_lower_record_opened_at_another_row_than_q_mod_m_is_a_7(shape):
    """A lower group's domain has no row q once q >= M_h.  A prover that opens it at q's HIGH bits (q scaled down to M_h rows) and not at q mod M_h — the index the walk
    stands at when it reaches the layer of that size — opens a true row with a true path, of another leaf: 7."""
    M0 = 1 << (shape[0][0] + shape[1])
    pr = mx.prove_ref(groups_of(shape), shape[1], shape[3], shape[4], low_q=lambda q, Mh: q * Mh // (M0 // 2))
    at = mx.layout(pr)
    qs = [int(pr[at["queries"] + t * at["qsize"]]) for t in range(at["num_queries"])]
    assert any(q * (1 << g["log_M"]) // (M0 // 2) != q % (1 << g["log_M"]) for q in qs for g in at["groups"][1:])
    assert both(pr) == 7


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4], SHAPES[5]])
def test_a_final_layer_the_last_fold_does_not_give_is_an_11(shape):
    """The same E4 constant added to every value of the final layer (`final_add=`), the prover honest before and after: the layer is still of degree < 4 (4 passes), the
    grinding and the queries are the new transcript's, every record, leaf and carried value is true — and what the last committed layer folds to is not the final value."""
    pr = mx.prove_ref(groups_of(shape), shape[1], shape[3], shape[4], final_add=[1, 0, 2, P - 1])
    assert both(pr) == 11
