"""zkir_mixed_eval_prove on the device: word-for-word parity with tests/mixed_eval_ref.prove_ref over the downloaded extensions (two and three groups, every blow-up, the add
form of the fold kernel at K = 1, 2 and 3, an injection into the last committed layer, the lane-form leaf hash), the proof's records against merkle_open, the fold kernel
alone against lowdeg_ref.fold plus the addend, nothing written past n_words, the argument edges of the C ABI, and arena reuse on the first context.  A shape's matrices,
commitments and proofs are computed once and shared."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import batch_eval_ref as be
import lowdeg_ref as ld
import mixed_eval_ref as mx
from zkir_amd import runtime as rt

pytestmark = pytest.mark.gpu

P = ld.P
GUARD = 0xA5A5A5A5
# (log_ns, b, per group (((width, mask), ..), n_points), num_queries, pow_bits): the six CPU shapes; M_0 = 2^16 (the lane-form leaf hash; the add form at K = 3); the shape a
# prover with a main trace, a chip and a table would use (the add form at K = 3 twice, the second time into the last committed layer).  (5,4)/1 adds at K = 1, (6,3)/2 at K = 2.
SHAPES = [
    ((4, 3), 1, ((((1, 1),), 1), (((1, 1),), 1)), 3, 3),
    ((5, 4), 1, ((((3, 0b11), (2, 0b01)), 2), (((2, 1),), 1)), 3, 3),
    ((6, 3), 2, ((((9, 1),), 1), (((3, 0b10), (1, 0b01)), 2)), 3, 4),
    ((8, 4), 1, ((((8, 0b11),), 2), (((5, 0b11),), 2)), 3, 3),
    ((7, 5, 3), 1, ((((9, 3), (7, 1)), 2), (((8, 2), (1, 3)), 2), (((5, 1),), 1)), 3, 4),
    ((5, 3), 3, ((((4, 1),), 1), (((2, 1), (2, 1)), 1)), 3, 3),
    ((13, 9), 3, ((((8, 3),), 2), (((8, 1),), 1)), 4, 6),
    ((10, 6, 3), 2, ((((152, 3), (40, 3), (4, 1)), 2), (((16, 3),), 2), (((8, 1),), 1)), 4, 6),
]


def _shapes_of(shape):
    return [([w for w, _ in wm], [k for _, k in wm], n) for wm, n in shape[2]]


@functools.lru_cache(maxsize=None)
def _ctx(log_n, b):
    from zkir_amd import stark
    return stark.StarkContext(log_n, b)


def _i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _commit(log_n, b, cols_lde):
    """(B8 matrix on the device, tree) of a GIVEN extended matrix uint32[width][M]"""
    from zkir_amd import stark
    width, m = cols_lde.shape
    mat = stark.to_b8(_i32(cols_lde).view(width, m))
    return mat, stark.merkle_commit(_ctx(log_n, b), mat, width)


@functools.lru_cache(maxsize=None)
def _shape(shape):
    """(EvalGroups on the device, the reference's groups over the downloaded extensions, the device's proof, the reference's proof)"""
    from zkir_amd import stark
    log_ns, b, _, nq, bits = shape
    dev, ref = [], []
    for h, (log_n, (widths, masks, n_points)) in enumerate(zip(log_ns, _shapes_of(shape))):
        ctx = _ctx(log_n, b)
        mats, trees, h_cols = [], [], []
        for m, width in enumerate(widths):
            cols = np.random.default_rng(131 * log_n + 7 * b + 13 * width + 3 * h + m).integers(0, P, (width, 1 << log_n), dtype=np.uint32)
            mat = stark.lde(ctx, stark.to_b8(_i32(cols).view(width, 1 << log_n)), clobber=True)
            mats.append(mat); trees.append(stark.merkle_commit(ctx, mat, width)); h_cols.append(_u32(stark.from_b8(mat, width)))
        pts = np.random.default_rng(9000 + 100 * h + log_n).integers(1, P, (n_points, 4), dtype=np.uint32)
        dev.append(stark.EvalGroup(ctx, mats, trees, widths, masks, pts))
        ref.append((h_cols, masks, pts))
    got = stark.mixed_eval_prove(dev, nq, bits)
    want = mx.prove_ref(ref, b, nq, bits)
    return dev, ref, got, want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}/{s[1]}")
def test_proof_equals_reference(shape):
    from zkir_amd import stark
    log_ns, b, _, nq, bits = shape
    dev, ref, got, want = _shape(shape)
    assert len(got) == len(want) == rt.mixed_eval_proof_words(log_ns, b, _shapes_of(shape), nq)
    at, lay = mx.layout(want), stark.mixed_eval_layout(got)
    for key in ("roots", "points", "evals", "n_evals", "layer_roots", "final", "nonce", "queries", "qsize"):
        assert lay[key] == at[key], key
    for g, l in zip(at["groups"], lay["groups"]):
        for key in ("log_n", "widths", "masks", "n_points", "roots", "points", "evals", "n_evals", "evals_of", "records"):
            assert l[key] == g[key], key
    assert np.array_equal(got[:at["evals"]], want[:at["evals"]]), "header / groups / roots / points"
    assert np.array_equal(got[at["evals"]:at["layer_roots"]], want[at["evals"]:at["layer_roots"]]), "evaluations"
    assert np.array_equal(got[at["layer_roots"]:at["layer_roots"] + 4], want[at["layer_roots"]:at["layer_roots"] + 4]), "layer 0's root: F_0"
    assert np.array_equal(got[at["layer_roots"]:at["queries"]], want[at["layer_roots"]:at["queries"]]), "layer roots / final layer / nonce"
    assert np.array_equal(got, want)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}/{s[1]}")
def test_proof_verifies_and_its_records_are_openings(shape):
    from zkir_amd import stark
    log_ns, b, _, nq, bits = shape
    dev, ref, got, want = _shape(shape)
    at = mx.layout(got)
    roots = np.concatenate([_u32(t[-4:]) for g in dev for t in g.trees])
    pts, ys = np.concatenate([g.points.reshape(-1) for g in dev]), got[at["evals"]:at["layer_roots"]]
    assert rt.mixed_eval_verify(got) == 0 and rt.mixed_eval_verify(got, roots, pts, ys) == 0 and mx.verify_ref(got, roots, pts, ys) == 0
    M0 = 1 << (log_ns[0] + b)
    starts = [at["queries"] + t * at["qsize"] for t in range(nq)]
    qs = [int(got[p0]) for p0 in starts]
    assert all(q < M0 // 2 for q in qs)
    for h, (g, lg) in enumerate(zip(dev, at["groups"])):
        Mh = 1 << lg["log_M"]
        idx = [x for q in qs for x in ((q, q + M0 // 2) if h == 0 else (q % Mh,))]
        per = 2 if h == 0 else 1
        for m, width in enumerate(lg["widths"]):
            recs = np.concatenate([got[p0 + lg["records"][m][0]:p0 + lg["records"][m][0] + per * lg["recs"][m]] for p0 in starts])
            want_recs = _u32(stark.merkle_open(g.ctx, g.mats[m], g.trees[m], np.array(idx, np.uint64), width))
            assert np.array_equal(recs, want_recs.reshape(-1)), (h, m)


# ---- the fold kernel alone ------------------------------------------------------------------------------------------------------------------------------
FOLD_LOG_N, FOLD_B = 14, 1                                          # a context whose FRI has layers of 2^15 values and below


def _fold_ref(layer, k, log_m, beta, addend):
    shift = pow(ld.GEN, 1 << (FOLD_LOG_N + FOLD_B - log_m), P)
    out, _ = ld.fold(layer.T.astype(np.uint64), k, shift, log_m, np.array(beta, np.uint32))
    return ld.e_add(out, addend.T.astype(np.uint64)) if addend is not None else out


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("log_g", [4, 12])
def test_fold_kernel_with_and_without_an_addend(k, log_g):
    """2^4 outputs (less than one workgroup) and 2^12 (sixteen workgroups): random words; every word p - 1 in layer and addend; no addend = the plain fold"""
    from zkir_amd import stark
    ctx = _ctx(FOLD_LOG_N, FOLD_B)
    log_m, g = log_g + k, 1 << log_g
    rng = np.random.default_rng(50 * k + log_g)
    for case, beta in (("random", rng.integers(0, P, 4)), ("p-1", [P - 1] * 4)):
        layer = rng.integers(0, P, (4, g << k), dtype=np.uint32) if case == "random" else np.full((4, g << k), P - 1, np.uint32)
        addend = rng.integers(0, P, (4, g), dtype=np.uint32) if case == "random" else np.full((4, g), P - 1, np.uint32)
        plain = _u32(stark.fri_fold(ctx, _i32(layer), k, beta))
        added = _u32(stark.fri_fold(ctx, _i32(layer), k, beta, _i32(addend)))
        assert plain.shape == added.shape == (4, g)
        assert np.array_equal(plain.T.astype(np.uint64), _fold_ref(layer, k, log_m, beta, None)), case
        assert np.array_equal(added.T.astype(np.uint64), _fold_ref(layer, k, log_m, beta, addend)), case
        zero = _u32(stark.fri_fold(ctx, _i32(layer), k, beta, _i32(np.zeros((4, g), np.uint32))))
        assert np.array_equal(zero, plain)


def test_fold_refuses_wrong_sizes():
    from zkir_amd import stark
    ctx = _ctx(FOLD_LOG_N, FOLD_B)
    layer = _i32(np.zeros((4, 64), np.uint32))
    for bad in (lambda: stark.fri_fold(ctx, layer, 0, [1, 0, 0, 0]), lambda: stark.fri_fold(ctx, layer, 4, [1, 0, 0, 0]),
                lambda: stark.fri_fold(ctx, layer, 2, [1, 0, 0, 0], _i32(np.zeros((4, 32), np.uint32))), lambda: stark.fri_fold(ctx, _i32(np.zeros((4, 48), np.uint32)), 1, [1, 0, 0, 0])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(rt.RuntimeError) as e:                       # a layer larger than the context's codeword; a challenge word that is not canonical
        stark.fri_fold(_ctx(4, 1), layer, 1, [1, 0, 0, 0])
    assert e.value.code == rt.ERR_ARGUMENT
    with pytest.raises(rt.RuntimeError) as e:
        stark.fri_fold(ctx, layer, 1, [P, 0, 0, 0])
    assert e.value.code == rt.ERR_ARGUMENT


# ---- a lower matrix that is not low-degree ----------------------------------------------------------------------------------------------------------------
def test_a_lower_matrix_that_is_not_low_degree_is_proven_into_a_refused_proof():
    from zkir_amd import stark
    shape = SHAPES[4]
    log_ns, b, _, nq, bits = shape
    dev, ref, _, _ = _shape(shape)
    cols = ref[1][0][0].copy()
    cols[3, 17] = (int(cols[3, 17]) + 1) % P
    mat, tree = _commit(log_ns[1], b, cols)
    g1 = dev[1]._replace(mats=[mat, dev[1].mats[1]], trees=[tree, dev[1].trees[1]])
    got = stark.mixed_eval_prove([dev[0], g1, dev[2]], nq, bits)
    assert np.array_equal(got, mx.prove_ref([ref[0], ([cols, ref[1][0][1]], ref[1][1], ref[1][2]), ref[2]], b, nq, bits))
    code = mx.verify_ref(got)
    assert code != 0 and rt.mixed_eval_verify(got) == code


# ---- the C ABI's edges ----------------------------------------------------------------------------------------------------------------------------------
def _last_error() -> str:
    return rt.lib().zkir_last_error().decode()


def _ptrs(xs):
    if xs is None:
        return None
    return (C.c_void_p * max(len(xs), 1))(*[(x.data_ptr() if hasattr(x, "data_ptr") else x) if x is not None else None for x in xs])


def _prove_raw(groups, nq, bits, buf, cap, n_groups=None, null=None, ctxs=None, n_words_null=False):
    """zkir_mixed_eval_prove on the flat arrays of `groups` ((ctx, mats, trees, widths, masks, points) each); null: the name of an array handed as NULL"""
    u = lambda xs: np.array(xs, np.uint32)
    a = {"ctxs": _ptrs([g[0].handle if g[0] is not None else None for g in groups] if ctxs is None else ctxs), "n_mats": u([len(g[3]) for g in groups]),
         "mats": _ptrs([m for g in groups for m in g[1]]), "widths": u([w for g in groups for w in g[3]]), "trees": _ptrs([t for g in groups for t in g[2]]),
         "masks": u([k for g in groups for k in g[4]]), "points": np.ascontiguousarray(np.concatenate([np.asarray(g[5], np.uint32).reshape(-1) for g in groups])),
         "n_points": u([len(np.asarray(g[5]).reshape(-1)) // 4 for g in groups]), "buf": buf}
    if null:
        a[null] = None
    ptr = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x
    n_words = C.c_uint64(12345)
    rc = rt.lib().zkir_mixed_eval_prove(a["ctxs"], len(groups) if n_groups is None else n_groups, ptr(a["n_mats"]), a["mats"], ptr(a["widths"]), a["trees"], ptr(a["masks"]),
                                       ptr(a["points"]), ptr(a["n_points"]), nq, bits, ptr(a["buf"]), cap, None if n_words_null else C.byref(n_words), None)
    return rc, n_words.value


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4], SHAPES[7]], ids=lambda s: f"{s[0]}/{s[1]}")
def test_nothing_is_written_past_n_words_and_a_short_buffer_is_refused(shape):
    _, _, _, nq, bits = shape
    dev, ref, got, want = _shape(shape)
    total = len(want)
    buf = np.full(total + 64, GUARD, np.uint32)
    rc, n = _prove_raw(dev, nq, bits, buf, total + 64)
    assert rc == rt.ZKIR_OK and n == total
    assert np.array_equal(buf[:total], want) and (buf[total:] == GUARD).all(), "words past n_words were written"
    buf = np.full(total + 64, GUARD, np.uint32)
    rc, n = _prove_raw(dev, nq, bits, buf, total - 1)
    assert rc == rt.ERR_ARGUMENT and n == 0 and (buf == GUARD).all()
    assert "zkir_mixed_eval_prove" in _last_error() and "cap_words" in _last_error()
    rc, n = _prove_raw(dev, nq, bits, buf, total)                    # exactly enough
    assert rc == rt.ZKIR_OK and n == total and np.array_equal(buf[:total], want) and (buf[total:] == GUARD).all()


def test_argument_edges():
    from zkir_amd import stark
    shape = SHAPES[4]
    log_ns, b, _, nq, bits = shape
    dev, ref, got, want = _shape(shape)
    buf = np.full(len(want) + 8, GUARD, np.uint32)
    big = 1 << 30
    BIG = [P - 1, P - 2, P - 3, P - 4]

    def refused(groups, word, nq=nq, bits=bits, cap=big, **kw):
        rc, n = _prove_raw(groups, nq, bits, buf, cap, **kw)
        assert rc == rt.ERR_ARGUMENT and n == 0 and (buf == GUARD).all(), word
        assert "zkir_mixed_eval_prove" in _last_error() and word in _last_error(), _last_error()
    # null pointers: every array, an entry of them, the buffer, n_words
    for name in ("ctxs", "n_mats", "mats", "widths", "trees", "masks", "points", "n_points", "buf"):
        refused(dev, "null", null=name)
    refused([dev[0], dev[1]._replace(ctx=None), dev[2]], "null")
    refused([dev[0], dev[1]._replace(mats=[dev[1].mats[0], None]), dev[2]], "null")
    refused([dev[0], dev[1], dev[2]._replace(trees=[None])], "null")
    assert _prove_raw(dev, nq, bits, buf, big, n_words_null=True)[0] == rt.ERR_ARGUMENT and (buf == GUARD).all()
    # the number of groups: one is zkir_batch_eval_prove's, four are too many
    refused(dev[:1], "n_groups")
    refused(dev, "n_groups", n_groups=1)
    other = stark.EvalGroup(_ctx(4, b), *dev[2][1:])
    refused([dev[0], dev[1], other, dev[2]], "n_groups")
    # a context of another blow-up; heights that do not strictly decrease
    refused([dev[0], dev[1]._replace(ctx=_ctx(log_ns[1], b + 1)), dev[2]], "log_blowup")
    refused([dev[1], dev[0], dev[2]], "decrease")
    refused([dev[0], dev[1], dev[1]], "decrease")
    refused([dev[0], dev[1]._replace(ctx=_ctx(log_ns[0], b)), dev[2]], "decrease")
    # a group's shape: n_mats, a width, the widths' sum above 512, a mask, an unused point
    refused([dev[0], dev[1]._replace(mats=dev[1].mats * 3, trees=dev[1].trees * 3, widths=[1] * 6, masks=[3] * 6), dev[2]], "n_mats")
    refused([dev[0], dev[1]._replace(widths=[0, 1]), dev[2]], "width")
    refused([dev[0]._replace(widths=[500, 13]), dev[1], dev[2]], "sum")
    refused([dev[0], dev[1]._replace(widths=[256, 257]), dev[2]], "sum")
    refused([dev[0], dev[1]._replace(masks=[2, 4]), dev[2]], "mask")
    refused([dev[0], dev[1]._replace(masks=[1, 1]), dev[2]], "opened by no matrix")
    refused([dev[0], dev[1], dev[2]._replace(masks=[2])], "mask")
    # the points of a lower group: in the base field, equal, not canonical
    refused([dev[0], dev[1]._replace(points=[[7, 0, 0, 0], BIG]), dev[2]], "points")
    refused([dev[0], dev[1]._replace(points=[BIG, BIG]), dev[2]], "points")
    refused([dev[0], dev[1], dev[2]._replace(points=[[1, P, 0, 0]])], "points")
    # queries, grinding
    refused(dev, "num_queries", nq=0)
    refused(dev, "num_queries", nq=129)
    refused(dev, "pow_bits", bits=25)
    # tensors of another size do not reach the library: a matrix of the wrong group's size, a tree of another, lists of different lengths
    for bad in ([dev[0], dev[1]._replace(mats=[dev[1].mats[0], dev[2].mats[0]]), dev[2]], [dev[0], dev[1], dev[2]._replace(trees=[dev[1].trees[0]])],
                [dev[0], dev[1]._replace(trees=dev[1].trees[:1]), dev[2]], [dev[0], dev[1]._replace(widths=[8]), dev[2]], [dev[0], dev[1], dev[2]._replace(points=[1, 2, 3])], []):
        with pytest.raises(ValueError):
            stark.mixed_eval_prove(bad, nq, bits)
    with pytest.raises(rt.RuntimeError) as e:
        stark.mixed_eval_prove(dev[:1], nq, bits)
    assert e.value.code == rt.ERR_ARGUMENT
    # .. and the contexts still prove
    assert np.array_equal(stark.mixed_eval_prove(dev, nq, bits), want)


def test_arena_is_reused_on_the_first_context():
    """a mixed proof, then a batched proof, then a low-degree proof on the FIRST group's context (whose arena the mixed proof uses), then the mixed proof again: each is its
    reference's"""
    from zkir_amd import stark
    shape = SHAPES[7]
    log_ns, b, _, nq, bits = shape
    dev, ref, got, want = _shape(shape)
    g0, (h_cols, masks, pts) = dev[0], ref[0]
    first = stark.mixed_eval_prove(dev, nq, bits)
    batch = stark.batch_eval_prove(g0.ctx, g0.mats, g0.trees, g0.widths, g0.masks, g0.points, nq, bits)
    low = stark.lowdeg_prove(g0.ctx, g0.mats[1], g0.trees[1], g0.widths[1], nq, bits)
    last = stark.mixed_eval_prove(dev, nq, bits)
    assert np.array_equal(first, want) and np.array_equal(last, want)
    assert np.array_equal(batch, be.prove_ref(h_cols, b, masks, pts, nq, bits)) and rt.batch_eval_verify(batch) == 0
    assert np.array_equal(low, ld.prove_ref(h_cols[1], b, nq, bits)) and rt.lowdeg_verify(low) == 0
