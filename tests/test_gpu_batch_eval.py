"""zkir_batch_eval_prove on the device: word-for-word parity with tests/batch_eval_ref.prove_ref over the downloaded extensions (every schedule class, the three leaf-hash
forms, one to four matrices, ragged and wide, matrices opened at one point of two), the quotient kernel alone at its column, mask and accumulator edges, the two identities
of the codeword, a matrix that is not low-degree, nothing written past n_words, the argument edges of the C ABI, and arena reuse across the three proofs.  A shape's matrices,
commitments and proofs are computed once and shared."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import batch_eval_ref as be
import eval_ref as ev
import lowdeg_ref as ld
from zkir_amd import runtime as rt

pytestmark = pytest.mark.gpu

P = ld.P
GUARD = 0xA5A5A5A5
# (log_n, b, ((width, mask), ..), n_points, num_queries, pow_bits): the three CPU shapes; b = 1, two ragged matrices at one point; four matrices with every mask; the shape
# a STARK would use (trace, auxiliary, quotient at the first point only); M = 2^16 (the lane-form leaf hash); b = 1 with a matrix opened at the second point only; ONE ragged
# matrix at two points (a batch of one runs the single-matrix quotient kernel under the 'ZKBE' header)
SHAPES = [(3, 1, ((1, 1),), 1, 3, 0), (3, 3, ((8, 3), (1, 1)), 2, 2, 4), (4, 2, ((9, 3), (7, 1), (8, 2)), 2, 4, 4), (6, 1, ((5, 1), (3, 1)), 1, 5, 6),
          (7, 2, ((17, 3), (8, 1), (1, 2), (9, 3)), 2, 4, 4), (10, 2, ((152, 3), (40, 3), (4, 1)), 2, 8, 8), (13, 3, ((8, 3), (8, 1)), 2, 6, 8), (11, 1, ((9, 3), (9, 2)), 2, 8, 8),
          (4, 2, ((9, 3),), 2, 4, 4)]
BIG, SMALL = [P - 1, P - 2, P - 3, P - 4], [0, 1, 0, 0]


def _points(seed: int, n_points: int) -> np.ndarray:
    return np.random.default_rng(8000 + seed).integers(1, P, (n_points, 4), dtype=np.uint32)


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


def _wm(shape):
    return [w for w, _ in shape[2]], [k for _, k in shape[2]]


@functools.lru_cache(maxsize=None)
def _shape(shape):
    """(B8 extensions on the device, their trees, the extensions downloaded [uint32[width_m][M]], the points, the device's proof, the reference's proof)"""
    from zkir_amd import stark
    log_n, b, wm, n_points, nq, bits = shape
    widths, masks = _wm(shape)
    ctx = _ctx(log_n, b)
    mats, trees, h_cols = [], [], []
    for m, width in enumerate(widths):
        cols = np.random.default_rng(97 * log_n + 5 * b + 11 * width + m).integers(0, P, (width, 1 << log_n), dtype=np.uint32)
        mat = stark.lde(ctx, stark.to_b8(_i32(cols).view(width, 1 << log_n)), clobber=True)
        mats.append(mat); trees.append(stark.merkle_commit(ctx, mat, width)); h_cols.append(_u32(stark.from_b8(mat, width)))
    pts = _points(log_n, n_points)
    got = stark.batch_eval_prove(ctx, mats, trees, widths, masks, pts, nq, bits)
    want = be.prove_ref(h_cols, b, masks, pts, nq, bits)
    return mats, trees, h_cols, pts, got, want


@pytest.mark.parametrize("shape", SHAPES)
def test_proof_equals_reference(shape):
    from zkir_amd import stark
    log_n, b, wm, n_points, nq, bits = shape
    widths, masks = _wm(shape)
    mats, trees, h_cols, pts, got, want = _shape(shape)
    assert len(got) == len(want) == rt.batch_eval_proof_words(log_n, b, widths, masks, n_points, nq)
    at, lay = be.layout(want), stark.batch_eval_layout(got)
    for key in ("shape", "roots", "points", "evals", "evals_of", "n_evals", "layer_roots", "final", "nonce", "queries", "qsize", "records", "widths", "masks"):
        assert lay[key] == at[key], key
    assert np.array_equal(got[:at["evals"]], want[:at["evals"]]), "header / shape / roots / points"
    assert np.array_equal(got[at["evals"]:at["layer_roots"]], want[at["evals"]:at["layer_roots"]]), "evaluations"
    assert np.array_equal(got[at["layer_roots"]:at["queries"]], want[at["layer_roots"]:at["queries"]]), "layer roots / final layer / nonce"
    assert np.array_equal(got, want)
    assert np.array_equal(got[at["roots"]:at["points"]], np.concatenate([_u32(t[-4:]) for t in trees]))


@pytest.mark.parametrize("shape", SHAPES)
def test_proof_verifies_and_its_records_are_openings(shape):
    from zkir_amd import stark
    log_n, b, wm, n_points, nq, bits = shape
    widths, masks = _wm(shape)
    mats, trees, h_cols, pts, got, want = _shape(shape)
    at = be.layout(got)
    roots, ys = np.concatenate([_u32(t[-4:]) for t in trees]), got[at["evals"]:at["layer_roots"]]
    assert rt.batch_eval_verify(got) == 0 and rt.batch_eval_verify(got, roots, pts, ys) == 0 and be.verify_ref(got, roots, pts, ys) == 0
    M = 1 << (log_n + b)
    starts = [at["queries"] + t * at["qsize"] for t in range(nq)]
    idx = []
    for p0 in starts:
        q = int(got[p0])
        assert q < M // 2
        idx += [q, q + M // 2]
    for m, width in enumerate(widths):
        recs = np.concatenate([got[p0 + at["records"][m][0]:p0 + at["records"][m][0] + 2 * at["recs"][m]] for p0 in starts])
        want_recs = _u32(stark.merkle_open(_ctx(log_n, b), mats[m], trees[m], np.array(idx, np.uint64), width))
        assert np.array_equal(recs, want_recs.reshape(-1)), m


# ---- the quotient kernel alone ------------------------------------------------------------------------------------------------------------------------
KERNEL_LOG_N, KERNEL_B = 6, 2
KERNEL_M = 1 << (KERNEL_LOG_N + KERNEL_B)
POINT_SETS = [[BIG], [SMALL, BIG], [[5, 0, 0, 7], [5, 0, 0, 8]]]
WIDTH_SETS = [((1, 3),), ((7, 3), (9, 1)), ((8, 2), (8, 1)), ((152, 3), (40, 3), (4, 1)), ((1, 1), (1, 2), (1, 3), (1, 3))]
GAMMAS = [[P - 1] * 4, [1, 0, 0, 0], [0, 1, 0, 0]]


@functools.lru_cache(maxsize=None)
def _kernel_matrix(width, seed):
    """(columns uint32[width][M], B8 matrix on the device with garbage in the columns a ragged last block does not have): the matrix need not be an extension"""
    from zkir_amd import stark
    cols = np.random.default_rng(1000 * seed + width).integers(0, P, (width, KERNEL_M), dtype=np.uint32)
    cols[:, 0], cols[:, KERNEL_M - 1] = P - 1, 0
    cols.setflags(write=False)
    mat = stark.to_b8(_i32(cols).view(width, KERNEL_M))
    if width % 8:                                                        # whatever sits in the columns a ragged last block does not have must not count
        mat[-1, :, width % 8:] = 12345
    return cols, mat


def _masks_for(wm, n_points):
    """the width set's masks cut to the points there are; with one point every matrix is opened at it"""
    return [(k & ((1 << n_points) - 1)) or 1 for _, k in wm]


def _quotient(cols, mats, masks, gamma, pts, ys):
    from zkir_amd import stark
    cw = _u32(stark.batch_eval_quotient(_ctx(KERNEL_LOG_N, KERNEL_B), mats, gamma, pts, ys, [len(c) for c in cols], masks))
    assert cw.shape == (4, KERNEL_M)
    return cw.T.astype(np.uint64)


@pytest.mark.parametrize("wm", WIDTH_SETS)
def test_quotient_kernel_against_the_reference(wm):
    """one block; a ragged block of seven before a second matrix (the prefetch crosses from a ragged last block); two full blocks with disjoint masks; 25 blocks in three
    matrices; four matrices of one column with every mask: against the reference's quotient, with arbitrary claims (the kernel subtracts what it is given)"""
    pairs = [_kernel_matrix(w, m) for m, (w, _) in enumerate(wm)]
    cols, mats = [c for c, _ in pairs], [d for _, d in pairs]
    rng = np.random.default_rng(len(wm) + 40)
    for pts in POINT_SETS:
        masks = _masks_for(wm, len(pts))
        n_evals = be.selected([w for w, _ in wm], masks, len(pts))[1]
        ys = rng.integers(0, P, (n_evals, 4), dtype=np.uint32)
        ys[0] = [P - 1] * 4
        for gamma in GAMMAS:
            assert np.array_equal(_quotient(cols, mats, masks, gamma, pts, ys), be.quotient(cols, masks, pts, ys, np.array(gamma, np.uint32))), (masks, gamma)


def test_one_matrix_with_a_full_mask_is_eval_quotient():
    """the two entries run one launch path (a batch of one takes eval_quotient_kernel): they agree with each other AND with the batch reference's quotient"""
    from zkir_amd import stark
    ctx = _ctx(KERNEL_LOG_N, KERNEL_B)
    rng = np.random.default_rng(5)
    for width in (9, 152):
        cols, mat = _kernel_matrix(width, 0)
        for pts in POINT_SETS[:2]:
            ys = rng.integers(0, P, (len(pts), width, 4), dtype=np.uint32)
            want = _u32(stark.eval_quotient(ctx, mat, GAMMAS[0], pts, ys, width))
            got = _u32(stark.batch_eval_quotient(ctx, [mat], GAMMAS[0], pts, ys, [width], [(1 << len(pts)) - 1]))
            assert np.array_equal(got, want)
            assert np.array_equal(got.T.astype(np.uint64), be.quotient([cols], [(1 << len(pts)) - 1], pts, ys.reshape(-1, 4), np.array(GAMMAS[0], np.uint32)))


def test_a_24_column_matrix_equals_its_split_into_16_and_8():
    from zkir_amd import stark
    ctx = _ctx(KERNEL_LOG_N, KERNEL_B)
    cols, mat = _kernel_matrix(24, 3)
    head, tail = mat[:2].contiguous(), mat[2:].contiguous()
    pts = POINT_SETS[1]
    ys = np.random.default_rng(6).integers(0, P, (2, 24, 4), dtype=np.uint32)
    whole = _u32(stark.batch_eval_quotient(ctx, [mat], GAMMAS[0], pts, ys, [24], [3]))
    split_ys = np.concatenate([ys[0, :16], ys[0, 16:], ys[1, :16], ys[1, 16:]])
    assert np.array_equal(_u32(stark.batch_eval_quotient(ctx, [head, tail], GAMMAS[0], pts, split_ys, [16, 8], [3, 3])), whole)
    assert np.array_equal(whole.T.astype(np.uint64), be.quotient([cols], [3], pts, ys.reshape(-1, 4), np.array(GAMMAS[0], np.uint32)))


@pytest.mark.parametrize("widths", [(512,), (256, 256), (128, 128, 128, 128)])
def test_accumulator_bound_with_every_word_p_minus_1(widths):
    """512 terms a sum, every word and every coordinate of gamma at its largest, the claims zero: a_i = 0 and the sums are at their bound; then with the true claims (a
    constant column is the constant polynomial, p - 1 at every point) a_i = A_i(x) at every row and the codeword is zero everywhere — an identity, not a comparison"""
    from zkir_amd import stark
    cols = [np.full((w, KERNEL_M), P - 1, np.uint32) for w in widths]
    mats = [stark.to_b8(_i32(c).view(len(c), KERNEL_M)) for c in cols]
    for pts in ([BIG], [SMALL, BIG]):
        mk = _masks_for([(w, 3) for w in widths], len(pts))
        zeros = np.zeros((len(pts) * 512, 4), np.uint32)
        gamma = [P - 1] * 4
        assert np.array_equal(_quotient(cols, mats, mk, gamma, pts, zeros), be.quotient(cols, mk, pts, zeros, np.array(gamma, np.uint32)))
        true = np.tile(np.array([P - 1, 0, 0, 0], np.uint32), (len(pts) * 512, 1))
        for gamma in ([P - 1] * 4, [2, 0, 0, 0]):
            assert not _quotient(cols, mats, mk, gamma, pts, true).any()


@pytest.mark.parametrize("mask", [1, 2])
def test_a_masked_out_point_counts_for_nothing(mask):
    """the second matrix is opened at ONE of the two points: the codeword is the reference's, in which the matrix does not occur at the other point at all — neither its
    columns nor any claim about it nor a power of gamma; and it is NOT the codeword with the matrix opened at both"""
    wm = ((9, 3), (7, mask))
    pairs = [_kernel_matrix(w, 10 + m) for m, (w, _) in enumerate(wm)]
    cols, mats = [c for c, _ in pairs], [d for _, d in pairs]
    pts = POINT_SETS[1]
    rng = np.random.default_rng(mask)
    ys = rng.integers(0, P, (9 + 9 + 7, 4), dtype=np.uint32)
    got = _quotient(cols, mats, [3, mask], GAMMAS[0], pts, ys)
    assert np.array_equal(got, be.quotient(cols, [3, mask], pts, ys, np.array(GAMMAS[0], np.uint32)))
    full = np.concatenate([ys[:9], rng.integers(0, P, (7, 4), dtype=np.uint32), ys[9:]]) if mask == 2 else np.concatenate([ys, rng.integers(0, P, (7, 4), dtype=np.uint32)])
    assert not np.array_equal(_quotient(cols, mats, [3, 3], GAMMAS[0], pts, full), got)


# ---- a matrix that is not low-degree ------------------------------------------------------------------------------------------------------------------
def test_a_matrix_that_is_not_low_degree_is_proven_into_a_refused_proof():
    """the device prover follows the honest procedure whatever the matrices hold: one changed extension word of the SECOND matrix gives the reference's proof, which both
    verifiers refuse with the same code"""
    from zkir_amd import stark
    shape = SHAPES[2]
    log_n, b, wm, n_points, nq, bits = shape
    widths, masks = _wm(shape)
    mats, trees, h_cols, pts, _, _ = _shape(shape)
    cols = h_cols[1].copy()
    cols[3, 17] = (int(cols[3, 17]) + 1) % P
    mat1, tree1 = _commit(log_n, b, cols)
    got = stark.batch_eval_prove(_ctx(log_n, b), [mats[0], mat1, mats[2]], [trees[0], tree1, trees[2]], widths, masks, pts, nq, bits)
    assert np.array_equal(got, be.prove_ref([h_cols[0], cols, h_cols[2]], b, masks, pts, nq, bits))
    code = be.verify_ref(got)
    assert code != 0 and rt.batch_eval_verify(got) == code


# ---- the C ABI's edges ----------------------------------------------------------------------------------------------------------------------------------
def _last_error() -> str:
    return rt.lib().zkir_last_error().decode()


def _ptrs(tensors):
    if tensors is None:
        return None
    return (C.c_void_p * max(len(tensors), 1))(*[t.data_ptr() if t is not None else None for t in tensors])


def _prove_raw(ctx, mats, trees, widths, masks, pts, n_points, nq, bits, buf, cap, n_mats=None):
    n_words = C.c_uint64(12345)
    pts = None if pts is None else np.ascontiguousarray(pts, dtype=np.uint32)
    ws = None if widths is None else np.ascontiguousarray(widths, dtype=np.uint32)
    ks = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = rt.lib().zkir_batch_eval_prove(ctx.handle, len(mats) if n_mats is None else n_mats, _ptrs(mats), ptr(ws), _ptrs(trees), ptr(ks), ptr(pts), n_points, nq, bits, ptr(buf), cap,
                                       C.byref(n_words), None)
    return rc, n_words.value


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[5], SHAPES[7]])
def test_nothing_is_written_past_n_words_and_a_short_buffer_is_refused(shape):
    log_n, b, wm, n_points, nq, bits = shape
    widths, masks = _wm(shape)
    mats, trees, h_cols, pts, got, want = _shape(shape)
    total = len(want)
    buf = np.full(total + 64, GUARD, np.uint32)
    rc, n = _prove_raw(_ctx(log_n, b), mats, trees, widths, masks, pts, n_points, nq, bits, buf, total + 64)
    assert rc == rt.ZKIR_OK and n == total
    assert np.array_equal(buf[:total], want) and (buf[total:] == GUARD).all(), "words past n_words were written"
    buf = np.full(total + 64, GUARD, np.uint32)
    rc, n = _prove_raw(_ctx(log_n, b), mats, trees, widths, masks, pts, n_points, nq, bits, buf, total - 1)
    assert rc == rt.ERR_ARGUMENT and n == 0 and (buf == GUARD).all()
    assert "zkir_batch_eval_prove" in _last_error() and "cap_words" in _last_error()
    rc, n = _prove_raw(_ctx(log_n, b), mats, trees, widths, masks, pts, n_points, nq, bits, buf, total)      # exactly enough
    assert rc == rt.ZKIR_OK and n == total and np.array_equal(buf[:total], want) and (buf[total:] == GUARD).all()


def test_argument_edges():
    from zkir_amd import stark
    shape = SHAPES[2]
    log_n, b, wm, n_points, nq, bits = shape
    widths, masks = _wm(shape)
    mats, trees, h_cols, pts, got, want = _shape(shape)
    ctx = _ctx(log_n, b)
    buf = np.full(len(want) + 8, GUARD, np.uint32)
    big = 1 << 30

    def refused(*args, word, **kw):
        rc, n = _prove_raw(*args, **kw)
        assert rc == rt.ERR_ARGUMENT and n == 0 and (buf == GUARD).all(), args[3:]
        assert "zkir_batch_eval_prove" in _last_error() and word in _last_error(), _last_error()
    # the number of matrices
    refused(ctx, mats, trees, widths, masks, pts, n_points, nq, bits, buf, big, word="n_mats", n_mats=0)
    refused(ctx, mats + mats[:2], trees + trees[:2], widths + widths[:2], masks + masks[:2], pts, n_points, nq, bits, buf, big, word="n_mats")
    # a width, the widths' sum
    refused(ctx, mats, trees, [0] + widths[1:], masks, pts, n_points, nq, bits, buf, big, word="width")
    refused(ctx, mats, trees, widths[:2] + [513], masks, pts, n_points, nq, bits, buf, big, word="width")
    refused(ctx, mats, trees, [500, 7, 8], masks, pts, n_points, nq, bits, buf, big, word="sum")
    refused(ctx, mats, trees, [256, 256, 1], masks, pts, n_points, nq, bits, buf, big, word="sum")
    # a mask, a point nobody opens
    refused(ctx, mats, trees, widths, [3, 0, 2], pts, n_points, nq, bits, buf, big, word="mask")
    refused(ctx, mats, trees, widths, [3, 4, 2], pts, n_points, nq, bits, buf, big, word="mask")
    refused(ctx, mats, trees, widths, [1, 2, 2], pts[:1], 1, nq, bits, buf, big, word="mask")               # bit 1 with one point
    refused(ctx, mats, trees, widths, [1, 1, 1], pts, n_points, nq, bits, buf, big, word="opened by no matrix")
    refused(ctx, mats, trees, widths, [2, 2, 2], pts, n_points, nq, bits, buf, big, word="opened by no matrix")
    # the points
    three = np.concatenate([pts, [[1, 2, 3, 4]]]).astype(np.uint32)
    refused(ctx, mats, trees, widths, masks, pts, 0, nq, bits, buf, big, word="n_points")
    refused(ctx, mats, trees, widths, masks, three, 3, nq, bits, buf, big, word="n_points")
    refused(ctx, mats, trees, widths, masks, [[7, 0, 0, 0], BIG], 2, nq, bits, buf, len(buf), word="points")      # a base-field point
    refused(ctx, mats, trees, widths, masks, [BIG, BIG], 2, nq, bits, buf, len(buf), word="points")               # equal points
    refused(ctx, mats, trees, widths, masks, [BIG, [1, P, 0, 0]], 2, nq, bits, buf, len(buf), word="points")      # a word that is not canonical
    # queries, grinding
    refused(ctx, mats, trees, widths, masks, pts, n_points, 0, bits, buf, len(buf), word="num_queries")
    refused(ctx, mats, trees, widths, masks, pts, n_points, 129, bits, buf, big, word="num_queries")
    refused(ctx, mats, trees, widths, masks, pts, n_points, nq, 25, buf, len(buf), word="pow_bits")
    # null pointers: the arrays, an entry of them, the points, the buffer, the context, n_words
    refused(ctx, None, trees, widths, masks, pts, n_points, nq, bits, buf, len(buf), word="null", n_mats=3)
    refused(ctx, mats, None, widths, masks, pts, n_points, nq, bits, buf, len(buf), word="null", n_mats=3)
    refused(ctx, mats, trees, None, masks, pts, n_points, nq, bits, buf, len(buf), word="null")
    refused(ctx, mats, trees, widths, None, pts, n_points, nq, bits, buf, len(buf), word="null")
    refused(ctx, [mats[0], None, mats[2]], trees, widths, masks, pts, n_points, nq, bits, buf, len(buf), word="null")
    refused(ctx, mats, [trees[0], trees[1], None], widths, masks, pts, n_points, nq, bits, buf, len(buf), word="null")
    refused(ctx, mats, trees, widths, masks, None, n_points, nq, bits, buf, len(buf), word="null")
    refused(ctx, mats, trees, widths, masks, pts, n_points, nq, bits, None, len(buf), word="null")
    ws, ks, p32 = np.array(widths, np.uint32), np.array(masks, np.uint32), np.ascontiguousarray(pts, dtype=np.uint32)
    n_words = C.c_uint64(7)
    args = (3, _ptrs(mats), ws.ctypes.data, _ptrs(trees), ks.ctypes.data, p32.ctypes.data, n_points, nq, bits, buf.ctypes.data, len(buf))
    assert rt.lib().zkir_batch_eval_prove(None, *args, C.byref(n_words), None) == rt.ERR_ARGUMENT and n_words.value == 0
    assert rt.lib().zkir_batch_eval_prove(ctx.handle, *args, None, None) == rt.ERR_ARGUMENT
    assert (buf == GUARD).all()
    # a context of log_n 2 has no layer to commit (its matrix and tree exist: the context serves the commitment)
    small = _ctx(2, 1)
    cols = np.random.default_rng(2).integers(0, P, (8, 4), dtype=np.uint32)
    m2 = stark.lde(small, stark.to_b8(_i32(cols).view(8, 4)))
    t2 = stark.merkle_commit(small, m2, 8)
    refused(small, [m2], [t2], [8], [3], pts, n_points, nq, bits, buf, len(buf), word="log_n")
    with pytest.raises(rt.RuntimeError) as e:
        stark.batch_eval_prove(small, [m2], [t2], [8], [3], pts, nq, bits)
    assert e.value.code == rt.ERR_ARGUMENT
    # tensors of another size do not reach the library
    other = _ctx(5, 3)
    with pytest.raises(ValueError):
        stark.batch_eval_prove(other, mats, trees, widths, masks, pts, nq, bits)
    with pytest.raises(ValueError):
        stark.batch_eval_prove(ctx, mats, [trees[0], trees[1][4:], trees[2]], widths, masks, pts, nq, bits)
    with pytest.raises(ValueError):
        stark.batch_eval_prove(ctx, mats, trees[:2], widths, masks, pts, nq, bits)
    with pytest.raises(ValueError):
        stark.batch_eval_prove(ctx, mats, trees, widths[:2], masks, pts, nq, bits)
    with pytest.raises(ValueError):
        stark.batch_eval_prove(ctx, mats, trees, [widths[0], 8 * mats[1].shape[0] + 1, widths[2]], masks, pts, nq, bits)
    with pytest.raises(ValueError):
        stark.batch_eval_prove(ctx, mats, trees, widths, masks, [1, 2, 3], nq, bits)
    with pytest.raises(ValueError):
        stark.batch_eval_quotient(ctx, mats, [1, 0, 0, 0], pts, np.zeros((5, 4), np.uint32), widths, masks)
    # .. and the context still proves
    assert np.array_equal(stark.batch_eval_prove(ctx, mats, trees, widths, masks, pts, nq, bits), want)


def test_arena_is_reused_across_the_three_proofs():
    """a batch proof, an evaluation proof, a low-degree proof, a batch proof on one context: the first and the last are identical, the two in between are their references'"""
    from zkir_amd import stark
    shape = SHAPES[4]
    log_n, b, wm, n_points, nq, bits = shape
    widths, masks = _wm(shape)
    mats, trees, h_cols, pts, got, want = _shape(shape)
    ctx = _ctx(log_n, b)
    first = stark.batch_eval_prove(ctx, mats, trees, widths, masks, pts, nq, bits)
    one = stark.eval_prove(ctx, mats[0], trees[0], widths[0], pts, nq, bits)
    low = stark.lowdeg_prove(ctx, mats[3], trees[3], widths[3], nq, bits)
    last = stark.batch_eval_prove(ctx, mats, trees, widths, masks, pts, nq, bits)
    assert np.array_equal(first, want) and np.array_equal(last, want)
    assert np.array_equal(one, ev.prove_ref(h_cols[0], b, pts, nq, bits)) and rt.eval_verify(one) == 0
    assert np.array_equal(low, ld.prove_ref(h_cols[3], b, nq, bits)) and rt.lowdeg_verify(low) == 0
