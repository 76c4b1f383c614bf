"""zkir_eval_prove on the device: word-for-word parity with tests/eval_ref.prove_ref over the downloaded extension (every schedule class, the three leaf-hash forms, ragged
and wide matrices, one and two points), the evaluation and quotient kernels alone at their column, row-count and accumulator edges, a matrix that is not low-degree, nothing
written past n_words, the argument edges of the C ABI, and arena reuse across the two proofs.  A shape's matrix, commitment and proofs are computed once and shared."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import eval_ref as ev
import lowdeg_ref as ld
from zkir_amd import runtime as rt

pytestmark = pytest.mark.gpu

P = ld.P
GUARD = 0xA5A5A5A5
# (log_n, b, width, n_points, num_queries, pow_bits): schedules [1], [1], [1,1], [1,3], [1,3,1], ..; 152 columns; M = 2^16 (the lane-form leaf hash; the quad form from 2^12
# leaves); b = 1 with a ragged width
SHAPES = [(3, 1, 1, 1, 3, 0), (3, 3, 8, 2, 2, 4), (4, 2, 9, 2, 4, 4), (6, 1, 5, 1, 5, 6), (7, 2, 17, 2, 4, 4), (10, 2, 152, 2, 8, 8), (13, 3, 8, 1, 6, 8), (11, 1, 9, 2, 8, 8)]
BIG, SMALL = [P - 1, P - 2, P - 3, P - 4], [0, 1, 0, 0]


def _points(seed: int, n_points: int) -> np.ndarray:
    return np.random.default_rng(7000 + seed).integers(1, P, (n_points, 4), dtype=np.uint32)


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
    """(B8 extension on the device, its tree, the extension downloaded uint32[width][M], the points, the device's proof, the reference's proof)"""
    from zkir_amd import stark
    log_n, b, width, n_points, nq, bits = shape
    ctx = _ctx(log_n, b)
    cols = np.random.default_rng(89 * log_n + 5 * b + width).integers(0, P, (width, 1 << log_n), dtype=np.uint32)
    mat = stark.lde(ctx, stark.to_b8(_i32(cols).view(width, 1 << log_n)), clobber=True)
    tree = stark.merkle_commit(ctx, mat, width)
    h_cols = _u32(stark.from_b8(mat, width))
    pts = _points(log_n, n_points)
    got = stark.eval_prove(ctx, mat, tree, width, pts, nq, bits)
    want = ev.prove_ref(h_cols, b, pts, nq, bits)
    return mat, tree, h_cols, pts, got, want


@pytest.mark.parametrize("shape", SHAPES)
def test_proof_equals_reference(shape):
    from zkir_amd import stark
    log_n, b, width, n_points, nq, bits = shape
    mat, tree, h_cols, pts, got, want = _shape(shape)
    assert len(got) == len(want) == rt.eval_proof_words(log_n, b, width, n_points, nq)
    at, lay = ev.layout(want), stark.eval_layout(got)
    for key in ("root", "points", "evals", "layer_roots", "final", "nonce", "queries", "qsize"):
        assert lay[key] == at[key], key
    assert np.array_equal(got[:at["evals"]], want[:at["evals"]]), "header / root / points"
    assert np.array_equal(got[at["evals"]:at["layer_roots"]], want[at["evals"]:at["layer_roots"]]), "evaluations"
    assert np.array_equal(got, want)
    assert np.array_equal(got[9:13], _u32(tree[-4:]))


@pytest.mark.parametrize("shape", SHAPES)
def test_proof_verifies_and_its_records_are_openings(shape):
    from zkir_amd import stark
    log_n, b, width, n_points, nq, bits = shape
    mat, tree, h_cols, pts, got, want = _shape(shape)
    at = ev.layout(got)
    ys = got[at["evals"]:at["layer_roots"]]
    assert rt.eval_verify(got) == 0 and rt.eval_verify(got, _u32(tree[-4:]), pts, ys) == 0 and ev.verify_ref(got, _u32(tree[-4:]), pts, ys) == 0
    M = 1 << (log_n + b)
    idx, recs = [], []
    for t in range(nq):
        p0 = at["queries"] + t * at["qsize"]
        q = int(got[p0])
        assert q < M // 2
        idx += [q, q + M // 2]
        recs.append(got[p0 + 1:p0 + 1 + 2 * at["rec"]])
    want_recs = _u32(stark.merkle_open(_ctx(log_n, b), mat, tree, np.array(idx, np.uint64), width))
    assert np.array_equal(np.concatenate(recs), want_recs.reshape(-1))


# ---- the evaluation kernels alone ---------------------------------------------------------------------------------------------------------------------
KERNEL_LOG_N, KERNEL_B = 6, 2
POINT_SETS = [[BIG], [SMALL, BIG], [[5, 0, 0, 7], [5, 0, 0, 8]]]


def _garbage_in_the_ragged_block(mat, width):
    if width % 8:                                                        # whatever sits in the columns a ragged last block does not have must not count
        mat[-1, :, width % 8:] = 12345


@functools.lru_cache(maxsize=None)
def _kernel_matrix(width):
    from zkir_amd import stark
    M = 1 << (KERNEL_LOG_N + KERNEL_B)
    cols = np.random.default_rng(width).integers(0, P, (width, M), dtype=np.uint32)
    cols[:, 0], cols[:, M - 1] = P - 1, 0
    mat = stark.to_b8(_i32(cols).view(width, M))
    _garbage_in_the_ragged_block(mat, width)
    return cols, mat


@pytest.mark.parametrize("width", [1, 7, 8, 9, 152])
def test_eval_at_column_edges(width):
    """one block, a ragged block of seven, exactly one, one and a ragged one, nineteen: against the reference's sums (the matrix need not be an extension: the sums are
    taken whatever it holds), for points with large and with minimal coordinates"""
    from zkir_amd import stark
    cols, mat = _kernel_matrix(width)
    for pts in POINT_SETS:
        got = _u32(stark.eval_at(_ctx(KERNEL_LOG_N, KERNEL_B), mat, pts, width))
        assert got.shape == (len(pts), width, 4)
        assert np.array_equal(got.astype(np.uint64), ev.evaluate(cols, KERNEL_B, pts))


@pytest.mark.parametrize("log_n,b,width", [(3, 3, 9), (12, 1, 9), (8, 2, 17)])
def test_eval_at_row_count_edges(log_n, b, width):
    """eight rows (fewer than the 64 a workgroup takes per iteration) at blow-up 8; 4096 rows at blow-up 2: sixteen chunks, each through the pipelined branch; 256 rows: one
    chunk through the pipelined branch"""
    from zkir_amd import stark
    M = 1 << (log_n + b)
    cols = np.random.default_rng(31 * log_n + b).integers(0, P, (width, M), dtype=np.uint32)
    mat = stark.to_b8(_i32(cols).view(width, M))
    _garbage_in_the_ragged_block(mat, width)
    for pts in POINT_SETS[:2]:
        got = _u32(stark.eval_at(_ctx(log_n, b), mat, pts, width))
        assert np.array_equal(got.astype(np.uint64), ev.evaluate(cols, b, pts))


@pytest.mark.parametrize("width", [152, 512])
def test_constant_p_minus_1_evaluates_to_p_minus_1(width):
    """every term of a 96-bit sum at its largest word; 512 columns = the limit.  A constant column is the constant polynomial: EXACTLY p - 1 at every point — an identity,
    not a comparison.  With these (true) claims a_i = A_i(x) at every row, so the quotient kernel's codeword is zero everywhere."""
    from zkir_amd import stark
    ctx = _ctx(KERNEL_LOG_N, KERNEL_B)
    M = 1 << (KERNEL_LOG_N + KERNEL_B)
    mat = stark.to_b8(_i32(np.full((width, M), P - 1, np.uint32)).view(width, M))
    for pts in POINT_SETS:
        got = _u32(stark.eval_at(ctx, mat, pts, width))
        assert (got[:, :, 0] == P - 1).all() and not got[:, :, 1:].any()
        for gamma in ([P - 1] * 4, [2, 0, 0, 0]):
            assert not _u32(stark.eval_quotient(ctx, mat, gamma, pts, got, width)).any()
    big = _ctx(12, 1)                                                    # 2^12 rows of p - 1: 256 terms a lane
    mat = stark.to_b8(_i32(np.full((9, 1 << 13), P - 1, np.uint32)).view(9, 1 << 13))
    got = _u32(stark.eval_at(big, mat, [BIG, SMALL], 9))
    assert (got[:, :, 0] == P - 1).all() and not got[:, :, 1:].any()


# ---- the quotient kernel alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 7, 8, 9, 152])
def test_quotient_kernel_column_edges(width):
    from zkir_amd import stark
    cols, mat = _kernel_matrix(width)
    M = cols.shape[1]
    rng = np.random.default_rng(width + 40)
    for pts in POINT_SETS[:2]:
        ys = rng.integers(0, P, (len(pts), width, 4), dtype=np.uint32)   # any claims: the kernel subtracts what it is given
        ys[0, 0] = [P - 1] * 4
        for gamma in ([P - 1] * 4, [1, 0, 0, 0], [0, 1, 0, 0]):
            cw = _u32(stark.eval_quotient(_ctx(KERNEL_LOG_N, KERNEL_B), mat, gamma, pts, ys, width))
            assert cw.shape == (4, M)
            assert np.array_equal(cw.T.astype(np.uint64), ev.quotient(cols, KERNEL_B, pts, ys, np.array(gamma, np.uint32)))


@pytest.mark.parametrize("width", [152, 512])
def test_quotient_accumulator_bound_with_every_word_p_minus_1(width):
    from zkir_amd import stark
    M = 1 << (KERNEL_LOG_N + KERNEL_B)
    cols = np.full((width, M), P - 1, np.uint32)
    mat = stark.to_b8(_i32(cols).view(width, M))
    for pts in ([BIG], [SMALL, BIG]):
        ys = np.zeros((len(pts), width, 4), np.uint32)                   # the claim "every column is 0 at z": a_i = 0, the sums at their largest
        for gamma in ([P - 1] * 4, [2, 0, 0, 0]):
            cw = _u32(stark.eval_quotient(_ctx(KERNEL_LOG_N, KERNEL_B), mat, gamma, pts, ys, width))
            assert np.array_equal(cw.T.astype(np.uint64), ev.quotient(cols, KERNEL_B, pts, ys, np.array(gamma, np.uint32)))


# ---- a matrix that is not low-degree ------------------------------------------------------------------------------------------------------------------
def test_a_matrix_that_is_not_low_degree_is_proven_into_a_refused_proof():
    """the device prover follows the honest procedure whatever the matrix holds: one changed value of the extension gives the reference's proof, which both verifiers refuse
    with the same code"""
    from zkir_amd import stark
    shape = SHAPES[2]
    log_n, b, width, n_points, nq, bits = shape
    cols = _shape(shape)[2].copy()
    cols[3, 17] = (int(cols[3, 17]) + 1) % P
    mat, tree = _commit(log_n, b, cols)
    pts = _shape(shape)[3]
    got = stark.eval_prove(_ctx(log_n, b), mat, tree, width, pts, nq, bits)
    assert np.array_equal(got, ev.prove_ref(cols, b, pts, nq, bits))
    code = ev.verify_ref(got)
    assert code != 0 and rt.eval_verify(got) == code


# ---- the C ABI's edges ----------------------------------------------------------------------------------------------------------------------------------
def _last_error() -> str:
    return rt.lib().zkir_last_error().decode()


def _prove_raw(ctx, mat, tree, width, pts, n_points, nq, bits, buf, cap):
    n_words = C.c_uint64(12345)
    pts = None if pts is None else np.ascontiguousarray(pts, dtype=np.uint32)
    rc = rt.lib().zkir_eval_prove(ctx.handle, mat.data_ptr() if mat is not None else None, width, tree.data_ptr() if tree is not None else None,
                                 pts.ctypes.data if pts is not None else None, n_points, nq, bits, buf.ctypes.data if buf is not None else None, cap, C.byref(n_words), None)
    return rc, n_words.value


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[5], SHAPES[7]])
def test_nothing_is_written_past_n_words_and_a_short_buffer_is_refused(shape):
    log_n, b, width, n_points, nq, bits = shape
    mat, tree, h_cols, pts, got, want = _shape(shape)
    total = len(want)
    buf = np.full(total + 64, GUARD, np.uint32)
    rc, n = _prove_raw(_ctx(log_n, b), mat, tree, width, pts, n_points, nq, bits, buf, total + 64)
    assert rc == rt.ZKIR_OK and n == total
    assert np.array_equal(buf[:total], want) and (buf[total:] == GUARD).all(), "words past n_words were written"
    buf = np.full(total + 64, GUARD, np.uint32)
    rc, n = _prove_raw(_ctx(log_n, b), mat, tree, width, pts, n_points, nq, bits, buf, total - 1)
    assert rc == rt.ERR_ARGUMENT and n == 0 and (buf == GUARD).all()
    assert "cap_words" in _last_error()
    rc, n = _prove_raw(_ctx(log_n, b), mat, tree, width, pts, n_points, nq, bits, buf, total)      # exactly enough
    assert rc == rt.ZKIR_OK and n == total and np.array_equal(buf[:total], want) and (buf[total:] == GUARD).all()


def test_argument_edges():
    from zkir_amd import stark
    shape = SHAPES[2]
    log_n, b, width, n_points, nq, bits = shape
    mat, tree, h_cols, pts, got, want = _shape(shape)
    ctx = _ctx(log_n, b)
    buf = np.full(len(want) + 8, GUARD, np.uint32)

    def refused(*args, word):
        rc, n = _prove_raw(*args)
        assert rc == rt.ERR_ARGUMENT and n == 0 and (buf == GUARD).all(), args[3:]
        assert "zkir_eval_prove" in _last_error() and word in _last_error(), _last_error()
    three = np.concatenate([pts, [[1, 2, 3, 4]]]).astype(np.uint32)
    refused(ctx, mat, tree, width, pts, 0, nq, bits, buf, 1 << 30, word="n_points")
    refused(ctx, mat, tree, width, three, 3, nq, bits, buf, 1 << 30, word="n_points")
    refused(ctx, mat, tree, width, [[7, 0, 0, 0], BIG], 2, nq, bits, buf, len(buf), word="points")          # a base-field point
    refused(ctx, mat, tree, width, [BIG, [0, 0, 0, 0]], 2, nq, bits, buf, len(buf), word="points")
    refused(ctx, mat, tree, width, [BIG, BIG], 2, nq, bits, buf, len(buf), word="points")                   # equal points
    refused(ctx, mat, tree, width, [BIG, [1, P, 0, 0]], 2, nq, bits, buf, len(buf), word="points")          # a word that is not canonical
    refused(ctx, mat, tree, width, [[0xFFFFFFFF, 1, 0, 0]], 1, nq, bits, buf, 1 << 30, word="points")
    refused(ctx, mat, tree, width, pts, n_points, 0, bits, buf, len(buf), word="num_queries")
    refused(ctx, mat, tree, width, pts, n_points, 129, bits, buf, 1 << 30, word="num_queries")
    refused(ctx, mat, tree, width, pts, n_points, nq, 25, buf, len(buf), word="pow_bits")
    refused(ctx, mat, tree, 0, pts, n_points, nq, bits, buf, len(buf), word="width")
    refused(ctx, mat, tree, 513, pts, n_points, nq, bits, buf, 1 << 30, word="width")
    refused(ctx, None, tree, width, pts, n_points, nq, bits, buf, len(buf), word="null")
    refused(ctx, mat, None, width, pts, n_points, nq, bits, buf, len(buf), word="null")
    refused(ctx, mat, tree, width, None, n_points, nq, bits, buf, len(buf), word="null")
    refused(ctx, mat, tree, width, pts, n_points, nq, bits, None, len(buf), word="null")
    p32 = np.ascontiguousarray(pts, dtype=np.uint32)
    n_words = C.c_uint64(7)
    assert rt.lib().zkir_eval_prove(None, mat.data_ptr(), width, tree.data_ptr(), p32.ctypes.data, n_points, nq, bits, buf.ctypes.data, len(buf), C.byref(n_words), None) == rt.ERR_ARGUMENT
    assert n_words.value == 0
    assert rt.lib().zkir_eval_prove(ctx.handle, mat.data_ptr(), width, tree.data_ptr(), p32.ctypes.data, n_points, nq, bits, buf.ctypes.data, len(buf), None, None) == rt.ERR_ARGUMENT
    # a context of log_n 2 has no layer to commit (its matrix and tree exist: the context serves the commitment)
    small = _ctx(2, 1)
    cols = np.random.default_rng(2).integers(0, P, (8, 4), dtype=np.uint32)
    m2 = stark.lde(small, stark.to_b8(_i32(cols).view(8, 4)))
    t2 = stark.merkle_commit(small, m2, 8)
    refused(small, m2, t2, 8, pts, n_points, nq, bits, buf, len(buf), word="log_n")
    with pytest.raises(rt.RuntimeError) as e:
        stark.eval_prove(small, m2, t2, 8, pts, nq, bits)
    assert e.value.code == rt.ERR_ARGUMENT
    # a matrix, a tree or points of another size do not reach the library
    other = _ctx(5, 3)
    with pytest.raises(ValueError):
        stark.eval_prove(other, mat, tree, width, pts, nq, bits)
    with pytest.raises(ValueError):
        stark.eval_prove(ctx, mat, tree[4:], width, pts, nq, bits)
    with pytest.raises(ValueError):
        stark.eval_prove(ctx, mat, tree, 8 * mat.shape[0] + 1, pts, nq, bits)
    with pytest.raises(ValueError):
        stark.eval_prove(ctx, mat, tree, width, [1, 2, 3], nq, bits)
    with pytest.raises(ValueError):
        stark.eval_at(other, mat, pts, width)
    with pytest.raises(ValueError):
        stark.eval_quotient(ctx, mat, [1, 0, 0, 0], pts, np.zeros((n_points, width + 1, 4), np.uint32), width)
    # .. and the context still proves
    assert np.array_equal(stark.eval_prove(ctx, mat, tree, width, pts, nq, bits), want)


def test_arena_is_reused_across_the_two_proofs():
    """an evaluation proof, a low-degree proof, an evaluation proof on one context: the first and the last are identical, the one in between is the low-degree reference's"""
    from zkir_amd import stark
    shape = SHAPES[4]
    log_n, b, width, n_points, nq, bits = shape
    mat, tree, h_cols, pts, got, want = _shape(shape)
    ctx = _ctx(log_n, b)
    first = stark.eval_prove(ctx, mat, tree, width, pts, nq, bits)
    low = stark.lowdeg_prove(ctx, mat, tree, width, nq, bits)
    last = stark.eval_prove(ctx, mat, tree, width, pts, nq, bits)
    assert np.array_equal(first, want) and np.array_equal(last, want)
    assert np.array_equal(low, ld.prove_ref(h_cols, b, nq, bits)) and rt.lowdeg_verify(low) == 0
