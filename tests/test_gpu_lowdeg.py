"""zkir_lowdeg_prove on the device: word-for-word parity with tests/lowdeg_ref.prove_ref over the downloaded extension (every schedule class, the three leaf-hash forms,
ragged and wide matrices), the combine kernel alone at its column and accumulator edges, the proof's records as opening records, nothing written past n_words, the
argument edges of the C ABI, and arena reuse.  A shape's matrix, commitment and proofs are computed once and shared."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import lowdeg_ref as ld
from zkir_amd import runtime as rt

pytestmark = pytest.mark.gpu

P = ld.P
GUARD = 0xA5A5A5A5
# (log_n, b, width, num_queries, pow_bits): the CPU test's shapes; 152 columns; M = 2^16 (layer 0 has 2^15 leaves: the one shape that reaches the lane-form leaf hash; the
# quad form from 2^12 leaves); b = 1 with a ragged width and the quad form
SHAPES = [(3, 1, 1, 3, 0), (3, 3, 8, 2, 4), (4, 2, 9, 4, 4), (5, 3, 8, 3, 0), (6, 1, 5, 5, 6), (7, 2, 17, 4, 4), (10, 2, 152, 8, 8), (13, 3, 8, 6, 8), (11, 1, 9, 8, 8)]


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
    """(B8 extension on the device, its tree, the extension downloaded uint32[width][M], the device's proof, the reference's proof)"""
    from zkir_amd import stark
    log_n, b, width, nq, bits = shape
    ctx = _ctx(log_n, b)
    cols = np.random.default_rng(97 * log_n + 7 * b + width).integers(0, P, (width, 1 << log_n), dtype=np.uint32)
    mat = stark.lde(ctx, stark.to_b8(_i32(cols).view(width, 1 << log_n)), clobber=True)
    tree = stark.merkle_commit(ctx, mat, width)
    h_cols = _u32(stark.from_b8(mat, width))
    got = stark.lowdeg_prove(ctx, mat, tree, width, nq, bits)
    want = ld.prove_ref(h_cols, b, nq, bits)
    return mat, tree, h_cols, got, want


@pytest.mark.parametrize("shape", SHAPES)
def test_proof_equals_reference(shape):
    log_n, b, width, nq, bits = shape
    mat, tree, h_cols, got, want = _shape(shape)
    assert len(got) == len(want) == rt.lowdeg_proof_words(log_n, b, width, nq)
    assert np.array_equal(got[:12], want[:12]), "header / root"
    assert np.array_equal(got, want)
    assert np.array_equal(got[8:12], _u32(tree[-4:]))


@pytest.mark.parametrize("shape", SHAPES)
def test_proof_verifies_and_its_records_are_openings(shape):
    from zkir_amd import stark
    log_n, b, width, nq, bits = shape
    mat, tree, h_cols, got, want = _shape(shape)
    assert rt.lowdeg_verify(got) == 0 and rt.lowdeg_verify(got, _u32(tree[-4:])) == 0 and ld.verify_ref(got) == 0
    at = ld.layout(got)
    M = 1 << (log_n + b)
    idx, recs = [], []
    for t in range(nq):
        p0 = at["queries"] + t * at["qsize"]
        q = int(got[p0])
        assert q < M // 2
        idx += [q, q + M // 2]
        recs.append(got[p0 + 1:p0 + 1 + 2 * at["rec"]])
    assert at["rec"] == stark.opening_words(width, M)
    v, s = stark.merkle_verify(_ctx(log_n, b), tree[-4:], width, M, np.array(idx, np.uint64), _i32(np.concatenate(recs)))
    assert not _u32(v).any() and [int(x) for x in _u32(s)] == [0, 0xFFFFFFFF]
    want_recs = _u32(stark.merkle_open(_ctx(log_n, b), mat, tree, np.array(idx, np.uint64), width))
    assert np.array_equal(np.concatenate(recs), want_recs.reshape(-1))


def _last_error() -> str:
    return rt.lib().zkir_last_error().decode()


def _prove_raw(ctx, mat, tree, width, nq, bits, buf, cap):
    n_words = C.c_uint64(12345)
    rc = rt.lib().zkir_lowdeg_prove(ctx.handle, mat.data_ptr() if mat is not None else None, width, tree.data_ptr() if tree is not None else None, nq, bits,
                                   buf.ctypes.data if buf is not None else None, cap, C.byref(n_words), None)
    return rc, n_words.value


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[6], SHAPES[8]])
def test_nothing_is_written_past_n_words_and_a_short_buffer_is_refused(shape):
    log_n, b, width, nq, bits = shape
    mat, tree, h_cols, got, want = _shape(shape)
    total = len(want)
    buf = np.full(total + 64, GUARD, np.uint32)
    rc, n = _prove_raw(_ctx(log_n, b), mat, tree, width, nq, bits, buf, total + 64)
    assert rc == rt.ZKIR_OK and n == total
    assert np.array_equal(buf[:total], want) and (buf[total:] == GUARD).all(), "words past n_words were written"
    buf = np.full(total + 64, GUARD, np.uint32)
    rc, n = _prove_raw(_ctx(log_n, b), mat, tree, width, nq, bits, buf, total - 1)
    assert rc == rt.ERR_ARGUMENT and n == 0 and (buf == GUARD).all()
    assert "cap_words" in _last_error()
    rc, n = _prove_raw(_ctx(log_n, b), mat, tree, width, nq, bits, buf, total)      # exactly enough
    assert rc == rt.ZKIR_OK and n == total and np.array_equal(buf[:total], want) and (buf[total:] == GUARD).all()


def test_two_proofs_in_a_row_on_one_context_are_identical():
    """arena reuse: the second proof runs in the workspace the first left behind; a proof of fewer columns in between moves every offset"""
    from zkir_amd import stark
    shape = SHAPES[5]
    log_n, b, width, nq, bits = shape
    mat, tree, h_cols, got, want = _shape(shape)
    ctx = _ctx(log_n, b)
    again = stark.lowdeg_prove(ctx, mat, tree, width, nq, bits)
    assert np.array_equal(again, want)
    tree9 = stark.merkle_commit(ctx, mat, 9)
    narrow = stark.lowdeg_prove(ctx, mat, tree9, 9, 2, 0)
    assert np.array_equal(narrow, ld.prove_ref(h_cols[:9], b, 2, 0))
    assert np.array_equal(stark.lowdeg_prove(ctx, mat, tree, width, nq, bits), want)


# ---- the combine kernel alone -------------------------------------------------------------------------------------------------------------------------
COMBINE_LOG_N, COMBINE_B = 6, 2


@pytest.mark.parametrize("width", [1, 7, 8, 9, 152])
def test_combine_kernel_column_edges(width):
    """one block, a ragged block of seven, exactly one, one and a ragged one, nineteen: against the reference's sum, for a gamma with large coordinates"""
    from zkir_amd import stark
    ctx = _ctx(COMBINE_LOG_N, COMBINE_B)
    M = 1 << (COMBINE_LOG_N + COMBINE_B)
    cols = np.random.default_rng(width).integers(0, P, (width, M), dtype=np.uint32)
    cols[:, 0], cols[:, M - 1] = P - 1, 0
    mat = stark.to_b8(_i32(cols).view(width, M))
    if width % 8:                                                        # whatever sits in the columns a ragged last block does not have must not count
        mat[-1, :, width % 8:] = 12345
    for gamma in ([P - 1, P - 2, P - 3, P - 4], [1, 0, 0, 0], [0, 1, 0, 0]):
        cw = _u32(stark.lowdeg_combine(ctx, mat, gamma, width))
        assert cw.shape == (4, M)
        assert np.array_equal(cw.T.astype(np.uint64), ld.combine(cols, np.array(gamma, np.uint32)))


@pytest.mark.parametrize("width", [152, 512])
def test_accumulator_bound_with_every_word_p_minus_1(width):
    """every term of a 96-bit sum at its largest word; 512 columns = the limit the bound is stated for.  Alone for a fixed gamma, and through a whole proof with the
    transcript's gamma (a constant column IS low-degree: the proof verifies)."""
    from zkir_amd import stark
    ctx = _ctx(COMBINE_LOG_N, COMBINE_B)
    M = 1 << (COMBINE_LOG_N + COMBINE_B)
    cols = np.full((width, M), P - 1, np.uint32)
    mat, tree = _commit(COMBINE_LOG_N, COMBINE_B, cols)
    for gamma in ([P - 1, P - 1, P - 1, P - 1], [2, 0, 0, 0]):
        cw = _u32(stark.lowdeg_combine(ctx, mat, gamma, width))
        assert np.array_equal(cw.T.astype(np.uint64), ld.combine(cols, np.array(gamma, np.uint32)))
    got = stark.lowdeg_prove(ctx, mat, tree, width, 3, 2)
    assert np.array_equal(got, ld.prove_ref(cols, COMBINE_B, 3, 2)) and rt.lowdeg_verify(got) == 0


def test_a_matrix_that_is_not_low_degree_is_proven_into_a_refused_proof():
    """the device prover follows the honest procedure whatever the matrix holds: one changed value of the extension gives the reference's proof, which both verifiers refuse (4)"""
    from zkir_amd import stark
    shape = SHAPES[2]
    log_n, b, width, nq, bits = shape
    cols = _shape(shape)[2].copy()
    cols[3, 17] = (int(cols[3, 17]) + 1) % P
    mat, tree = _commit(log_n, b, cols)
    got = stark.lowdeg_prove(_ctx(log_n, b), mat, tree, width, nq, bits)
    assert np.array_equal(got, ld.prove_ref(cols, b, nq, bits)) and rt.lowdeg_verify(got) == 4 == ld.verify_ref(got)


# ---- argument edges: ZKIR_ERR_ARGUMENT with a message, before anything is launched ------------------------------------------------------------------------
def test_argument_edges():
    from zkir_amd import stark
    shape = SHAPES[2]
    log_n, b, width, nq, bits = shape
    mat, tree, h_cols, got, want = _shape(shape)
    ctx = _ctx(log_n, b)
    buf = np.full(len(want) + 8, GUARD, np.uint32)

    def refused(*args, word):
        rc, n = _prove_raw(*args)
        assert rc == rt.ERR_ARGUMENT and n == 0 and (buf == GUARD).all(), args[3:]
        assert "zkir_lowdeg_prove" in _last_error() and word in _last_error(), _last_error()
    refused(ctx, mat, tree, width, 0, bits, buf, len(buf), word="num_queries")
    refused(ctx, mat, tree, width, 129, bits, buf, 1 << 30, word="num_queries")
    refused(ctx, mat, tree, width, nq, 25, buf, len(buf), word="pow_bits")
    refused(ctx, mat, tree, 0, nq, bits, buf, len(buf), word="width")
    refused(ctx, mat, tree, 513, nq, bits, buf, 1 << 30, word="width")
    refused(ctx, None, tree, width, nq, bits, buf, len(buf), word="null")
    refused(ctx, mat, None, width, nq, bits, buf, len(buf), word="null")
    refused(ctx, mat, tree, width, nq, bits, None, len(buf), word="null")
    n_words = C.c_uint64(7)
    assert rt.lib().zkir_lowdeg_prove(None, mat.data_ptr(), width, tree.data_ptr(), nq, bits, buf.ctypes.data, len(buf), C.byref(n_words), None) == rt.ERR_ARGUMENT and n_words.value == 0
    assert rt.lib().zkir_lowdeg_prove(ctx.handle, mat.data_ptr(), width, tree.data_ptr(), nq, bits, buf.ctypes.data, len(buf), None, None) == rt.ERR_ARGUMENT
    # a context of log_n 2 has no layer to commit (its matrix and tree exist: the context serves the commitment)
    small = _ctx(2, 1)
    cols = np.random.default_rng(2).integers(0, P, (8, 4), dtype=np.uint32)
    m2 = stark.lde(small, stark.to_b8(_i32(cols).view(8, 4)))
    t2 = stark.merkle_commit(small, m2, 8)
    refused(small, m2, t2, 8, nq, bits, buf, len(buf), word="log_n")
    with pytest.raises(rt.RuntimeError) as e:
        stark.lowdeg_prove(small, m2, t2, 8, nq, bits)
    assert e.value.code == rt.ERR_ARGUMENT
    # a matrix or a tree of another context's size does not reach the library
    other = _ctx(5, 3)
    with pytest.raises(ValueError):
        stark.lowdeg_prove(other, mat, tree, width, nq, bits)
    with pytest.raises(ValueError):
        stark.lowdeg_prove(ctx, mat, tree[4:], width, nq, bits)
    with pytest.raises(ValueError):
        stark.lowdeg_prove(ctx, mat, tree, 8 * mat.shape[0] + 1, nq, bits)
    # .. and the context still proves
    assert np.array_equal(stark.lowdeg_prove(ctx, mat, tree, width, nq, bits), want)
