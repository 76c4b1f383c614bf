"""The leaf sponge's two instances and the compression (stark.hip, round 28) against the oracle, every level of the tree, bit for bit.

A width that is a non-zero multiple of 8 takes leaf_hash_kernel (full blocks: one quad of each permutation's last layer, no per-word width test, constants derived forwards
from the factor the words carry); every other width takes leaf_hash_ragged_kernel (the general sponge).  Widths on both sides of each boundary, leaf counts from one wave's
worth to several workgroups; compress_kernel / subtree_kernel build the levels above, so the whole tree is compared."""
import ctypes as C

import numpy as np
import pytest

from oracle import api as oracle, stark_api as so
from zkir_amd import runtime as rt, spec

pytestmark = pytest.mark.gpu
P = so.P

FULL_WIDTHS = [8, 16, 24, 152, 160]
RAGGED_WIDTHS = [1, 7, 9, 15, 17, 23, 25, 150]
COUNTS = [2, 64, 256, 4096]


@pytest.fixture(scope="module")
def ctx():
    from zkir_amd import stark
    c = stark.StarkContext(4)
    yield c
    c.close()


def _tree(ctx, mat):
    import torch
    from zkir_amd import stark
    return stark.merkle_commit(ctx, stark.to_b8(torch.from_numpy(mat.view(np.int32)).cuda()), mat.shape[0]).cpu().numpy().view(np.uint32)


def _check(ctx, mat):
    root, layers = so.merkle(mat, want_layers=True)
    tree = _tree(ctx, mat)
    n = mat.shape[1]
    assert np.array_equal(tree[:4 * n], layers[:4 * n]), "leaf digests"
    assert np.array_equal(tree, layers), "levels above the leaves"
    assert np.array_equal(tree[-4:], root)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("width", FULL_WIDTHS + RAGGED_WIDTHS)
def test_tree_equals_oracle(ctx, width, n):
    mat = np.random.default_rng(1000 * width + n).integers(0, P, (width, n)).astype(np.uint32)
    _check(ctx, mat)


@pytest.mark.parametrize("width", [152, 150, 16, 9])
@pytest.mark.parametrize("kind", ["zero_blocks", "extremes", "equal_rows", "all_zero", "all_p_minus_1"])
def test_tree_of_special_matrices(ctx, width, kind):
    n = 256
    rng = np.random.default_rng(width)
    mat = rng.integers(0, P, (width, n)).astype(np.uint32)
    if kind == "zero_blocks":                                     # whole blocks of eight columns zero: the first, a middle one and the last (the LDE leaves such blocks)
        mat[:8] = 0
        mat[(width // 16) * 8:(width // 16) * 8 + 8] = 0
        mat[((width - 1) // 8) * 8:] = 0
    elif kind == "extremes":                                      # 0 and p - 1 in every column
        mat[:, 0::7] = 0
        mat[:, 3::7] = P - 1
        mat[::2, 5] = 0; mat[1::2, 5] = P - 1; mat[::2, 6] = P - 1; mat[1::2, 6] = 0
    elif kind == "equal_rows":
        mat[:] = mat[:, :1]
    elif kind == "all_zero":
        mat[:] = 0
    else:
        mat[:] = P - 1
    _check(ctx, mat)


@pytest.mark.parametrize("n", [1, 3, 255, 257, 1000])
@pytest.mark.parametrize("width", [8, 152, 9])
def test_leaf_layer_alone_at_any_leaf_count(ctx, width, n):
    """zkir_merkle_leaves_launch takes any leaf count (the tree entry takes powers of two): the last wave is partly idle"""
    import torch
    from zkir_amd import pipeline as pl, stark
    mat = np.random.default_rng(7 * width + n).integers(0, P, (width, n)).astype(np.uint32)
    dig = torch.zeros(4 * n + 4, dtype=torch.int32, device="cuda")
    b8 = stark.to_b8(torch.from_numpy(mat.view(np.int32)).cuda())
    pl._check(rt.lib().zkir_merkle_leaves_launch(ctx.handle, b8.data_ptr(), width, n, dig.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    got = dig.cpu().numpy().view(np.uint32)
    assert not got[4 * n:].any()                                  # nothing behind the last leaf
    rows = range(n) if n <= 300 else list(range(0, n, 37)) + [n - 1]
    for j in rows:
        assert np.array_equal(got[4 * j:4 * j + 4], so.hash_elems(mat[:, j])), j


def test_montgomery_resting_matrices():
    """The prover's LDE matrices rest in Montgomery form (f0 = R): commit_trace's root of a 2^10-row fib run is the oracle's, and so is the trace root inside a proof,
    whose tree is built from the Montgomery-form matrix."""
    from zkir_amd import pipeline as pl, stark
    n = 1 << 10
    blob = spec.fib_endless_program().to_bytes()
    log = rt.interpret(blob, [], rt.VMConfig(max_cycles=n, enable_execution_trace=True))
    ddl = pl.upload(log)
    tr = pl.DeviceTrace(ddl)
    pl.trace_fill(pl.trace_fill_args(ddl, tr))
    res = oracle.run(blob, max_cycles=n, enable_execution_trace=True)
    want = so.commit_trace(res.rows, 1)
    c = stark.StarkContext(10)
    root, L, tree = stark.commit_trace(c, tr)
    assert np.array_equal(root, want)
    proof = stark.prove(c, tr, rt.public_inputs(log, blob, [], False))
    assert stark.trace_root(proof) == [int(x) for x in want]
    c.close(); log.close()
