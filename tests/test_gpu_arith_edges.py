"""Device code of the field arithmetic and of Poseidon2 at the edges of their documented domains: every bb:: primitive (the inline-asm paths
included) and all three device formulations of the permutation through the probe library, word for word against the big-integer reference
(tests/bigint_ref.py); the production Merkle kernels on crafted digests and rows, and the LDE with chosen values after every inverse stage."""
from __future__ import annotations

import ctypes as C
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import arith_probe as ap
import bigint_ref as ref
from oracle import stark_api as so
from test_arith_edges import ACC96_SHAPES, PRIM_NAMES, _check_cases, acc96_inputs, check_acc96, check_p2, run_ext

pytestmark = pytest.mark.gpu

P = ref.P
N_RANDOM = 1 << 20


@pytest.fixture(scope="module", autouse=True)
def _device_before_probe():
    """the HIP runtime initialised (by torch, on cuda:0) before the probe library is loaded: loaded first, its first launch came back with
    hipErrorNoDevice when no launch of the process had happened yet (seen with the Poseidon2 tests run on their own)"""
    import torch
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def dev_elementwise(name, slots, uarg=0):
    import torch
    d_in = _dev(np.ascontiguousarray(slots, np.uint64))
    d_out = torch.zeros((len(slots), 2), dtype=torch.int64, device="cuda")
    assert ap.lib().zkir_probe_elementwise(0, ap.op_ids()[name], d_in.data_ptr(), len(slots), uarg, d_out.data_ptr(), _stream()) == 0
    return _host(d_out, np.uint64)


def dev_acc96(variant, xs, ys):
    import torch
    n, terms = ys.shape
    d_x, d_y = _dev(np.ascontiguousarray(xs, np.uint32)), _dev(np.ascontiguousarray(ys, np.uint32))
    d_out = torch.zeros((n, 4, 3), dtype=torch.int64, device="cuda")
    assert ap.lib().zkir_probe_acc96(0, variant, d_x.data_ptr(), d_y.data_ptr(), terms, n, d_out.data_ptr(), _stream()) == 0
    return _host(d_out, np.uint64)


_consts = None


def dev_p2(form, raw, states, junk=0xFFFFFFFF):
    import torch
    global _consts
    if _consts is None:
        _consts = torch.from_numpy(ap.consts_bytes()).cuda()
    s = _dev(np.ascontiguousarray(states, np.uint32))
    canon, rawo = torch.zeros_like(s), torch.zeros_like(s)
    assert ap.lib().zkir_probe_p2(0, form, int(raw), _consts.data_ptr(), s.data_ptr(), len(states), junk, canon.data_ptr(), rawo.data_ptr(), _stream()) == 0
    return _host(canon, np.uint32), _host(rawo, np.uint32)


# ---- primitives ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PRIM_NAMES)
def test_device_primitive(name):
    slots = ap.to_slots(name, ref.edge_cases(name))
    _check_cases(name, slots, dev_elementwise(name, slots))
    slots = ap.random_slots(name, N_RANDOM, np.random.default_rng(zlib.crc32(name.encode()) + 11))
    _check_cases(name, slots, dev_elementwise(name, slots), with_contract=False)


def test_device_mulhi_u32():
    a_vals = ref.edge_values("mulhi_u32", 0)
    for b in ref.edge_values("mulhi_u32", 1) + [ref.reduce_wide_m(s) for s in (4, 6, 7)]:
        slots = ap.to_slots("mulhi_u32", [(a, 0) for a in a_vals])
        _check_cases("mulhi_u32", slots, dev_elementwise("mulhi_u32", slots, b), b)
    rng = np.random.default_rng(6)
    for _ in range(4):
        b = int(rng.integers(0, 1 << 32))
        slots = ap.random_slots("mulhi_u32", N_RANDOM // 4, rng)
        _check_cases("mulhi_u32", slots, dev_elementwise("mulhi_u32", slots, b), b, with_contract=False)


@pytest.mark.parametrize("terms,top", ACC96_SHAPES)
def test_device_acc96(terms, top):
    """mad96 / mad96_s / mad96x4_s (v_mad_u64_u32 + v_addc_co_u32) and acc96_div_R at the kernels' term counts"""
    rng = np.random.default_rng(terms + 1)
    xs, xs4, ys = acc96_inputs(terms, top, 64 if terms > 1000 else 128, rng)
    for variant in range(3):
        x = xs if variant == 0 else np.ascontiguousarray(np.broadcast_to(xs[0], (terms,))) if variant == 1 else xs4
        check_acc96(variant, xs, xs4, ys, dev_acc96(variant, x, ys))


def test_device_extension_pow_inv():
    run_ext(dev_elementwise, np.random.default_rng(10), 4000)


# ---- Poseidon2: the three device formulations (and permute()) ---------------------------------------------------------------------------
FORMS = {"permute_scaled": 0, "permute_quad_scaled": 1, "permute_row16_scaled": 2, "permute": 3}


@pytest.mark.parametrize("form", list(FORMS))
def test_device_poseidon2_edges_and_round_targets(form):
    f = FORMS[form]
    sc = ap.scales()
    fo = ap.f_out(sc)
    states = [c[2] for c in ap.round_targeted_inputs()] + ap.edge_states()
    # 30 rounds x 30 targets + the edge states in one launch: far more permutations than a wave holds, so every lane / quad / row position of a wave runs some
    want = [ref.permute(s) for s in states]
    canon, raw = dev_p2(f, False, np.array(states, np.uint32))
    check_p2(states, canon, raw if f != 3 else None, fo, form, want)
    if f != 3:
        rows, canon_in = ap.raw_top_words(sc)
        rows = rows * 8                                     # every lane / quad / row position of a wave
        canon_in = canon_in * 8
        canon, raw = dev_p2(f, True, np.array(rows, np.uint32))
        check_p2(canon_in, canon, raw, fo, form + " (raw words)")


@pytest.mark.parametrize("form", list(FORMS))
def test_device_poseidon2_random(form):
    rng = np.random.default_rng(20 + FORMS[form])
    states = rng.integers(0, P, (1 << 16, 12)).astype(np.uint32)
    canon, raw = dev_p2(FORMS[form], False, states, junk=int(rng.integers(0, 1 << 32)))
    fo = ap.f_out(ap.scales())
    for i in range(len(states)):
        assert np.array_equal(canon[i], so.permute(states[i])), f"{form}: random state {i}"
    if FORMS[form] != 3:
        assert (raw < P + 64).all()
        idx = rng.integers(0, len(states), 64)
        for i in idx:
            want = so.permute(states[i]).tolist()
            assert all((int(raw[i, k]) - fo * want[k]) % P == 0 for k in range(12))


# ---- production Merkle kernels on crafted inputs -------------------------------------------------------------------------------------
EDGE_DIGEST_WORDS = [0, 1, 2, P - 2, P - 1, (P - 1) // 2, ref.R1, 11]


def edge_digests(n, rng):
    out = []
    for i in range(n):
        k = i % 6
        if k == 0:
            out.append([P - 1] * 4)
        elif k == 1:
            out.append([0] * 4)
        elif k == 2:
            out.append([EDGE_DIGEST_WORDS[(i + j) % len(EDGE_DIGEST_WORDS)] for j in range(4)])
        elif k == 3:
            out.append([P - 1, 0, P - 1, 0])
        elif k == 4:
            out.append([1] * 4)
        else:
            out.append(rng.integers(0, P, 4).tolist())
    return out


@pytest.mark.parametrize("n", [2, 64, 128, 256, 2048])
def test_merkle_cap_on_edge_digests(n):
    """subtree_kernel over digests made of edge words: the per-lane branch (> 64 permutations a level) and the row16 branch (<= 64)"""
    import torch
    from zkir_amd import pipeline as pl, runtime as rt, stark
    rng = np.random.default_rng(n)
    digests = edge_digests(n, rng)
    tree = torch.zeros(4 * (2 * n - 1), dtype=torch.int32, device="cuda")
    tree[:4 * n] = torch.from_numpy(np.array(digests, np.uint32).reshape(-1).view(np.int32)).cuda()
    ctx = stark.StarkContext(10)
    pl._check(rt.lib().zkir_merkle_cap_launch(ctx.handle, tree.data_ptr(), n, _stream()))
    got = _host(tree, np.uint32).reshape(-1, 4)
    level, off = [np.array(d, np.uint32) for d in digests], n
    while len(level) > 1:
        level = [so.compress(level[2 * i], level[2 * i + 1]) for i in range(len(level) // 2)]
        for i, d in enumerate(level):
            assert np.array_equal(got[off + i], d), f"node {off + i} of the cap over {n} digests"
        off += len(level)
    ctx.close()


def leaf_rows_with_round0_inputs(targets):
    """rate words x (8) such that the S-box inputs of round 0, (M_ext (x, 0, 0, 0, 0) + ext[0])_i for i = 0..7, are the given targets"""
    A = [row[:8] for row in ref.EXT_M[:8]]
    Ainv = ref.mat_inv(A)
    return [ref.mat_vec(Ainv, [(t - c) % P for t, c in zip(tg, ref.EXT_RC[0][:8])]) for tg in targets]


@pytest.mark.parametrize("width", [8, 13])
def test_merkle_leaves_round0_extremes(width):
    """leaf_hash_kernel on rows whose first S-box layer sees chosen extremes (8 of its 12 inputs set by solving the initial linear layer)"""
    import torch
    from zkir_amd import pipeline as pl, runtime as rt, stark
    targets = []
    for v in (0, 1, P - 1, (P - 1) // 2, P - 2):
        targets.append([v] * 8)
    targets += [[P - 1, 0] * 4, [0, P - 1] * 4]
    for i in range(8):
        t = [0] * 8
        t[i] = P - 1
        targets.append(t)
    rows = leaf_rows_with_round0_inputs(targets)
    for x, tg in zip(rows, targets):                                    # the solved rows do what they are meant to
        y = ref.mat_vec(ref.EXT_M, x + [0] * 4)
        assert [(a + c) % P for a, c in zip(y[:8], ref.EXT_RC[0][:8])] == tg
    n = 256
    rng = np.random.default_rng(width)
    mat = rng.integers(0, P, (width, n)).astype(np.uint32)
    for j in range(n):
        mat[:8, j] = rows[j % len(rows)]
    mat[8:, ::3] = P - 1
    ctx = stark.StarkContext(8)
    b8 = stark.to_b8(torch.from_numpy(mat.view(np.int32)).cuda())
    dig = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    pl._check(rt.lib().zkir_merkle_leaves_launch(ctx.handle, b8.data_ptr(), width, n, dig.data_ptr(), _stream()))
    got = _host(dig, np.uint32)
    _, layers = so.merkle(mat, want_layers=True)
    assert np.array_equal(got.reshape(-1), layers[:4 * n])
    for j in range(len(rows)):                                          # and the reference agrees on the digests
        if width == 8:
            assert got[j].tolist() == ref.permute(rows[j] + [0] * 4)[:4]
    ctx.close()


# ---- the LDE with chosen values after every inverse stage ----------------------------------------------------------------------------
def _pow_table(w, n):
    t = np.ones(n, np.uint64)
    k = 1
    while k < n:
        t[k:2 * k] = t[:k] * np.uint64(ref.fpow(w, k)) % np.uint64(P)
        k *= 2
    return t


def undo_stages(y, s_last, L):
    """inputs x such that inverse DIF stages 0..s_last map x to y (rows of y: columns), vectorized"""
    x = y.astype(np.uint64).copy()
    n = 1 << L
    w = ref.root_of_unity(L)                      # the inverse of the stage twiddle w_N^-j is w_N^j
    pw = _pow_table(w, n // 2)
    half = np.uint64((P + 1) // 2)
    Pu = np.uint64(P)
    for s in range(s_last, -1, -1):
        h = n >> (s + 1)
        v = x.reshape(x.shape[0], 1 << s, 2, h)
        tw = pw[np.arange(h, dtype=np.uint64) << np.uint64(s)]
        a, d = v[:, :, 0, :], v[:, :, 1, :] * tw % Pu
        na = (a + d) % Pu * half % Pu
        nb = (a + Pu - d) % Pu * half % Pu
        v[:, :, 0, :] = na
        v[:, :, 1, :] = nb
    return x


def stage_targets(L):
    """column 2s: all p-1 after inverse stage s; column 2s+1: p-1 / 0 on the pairs of stage s + 1 (the lazy difference of those pairs is 2p - 1)"""
    n = 1 << L

    def one(s):
        h = max(n >> (s + 2), 1)
        alt = np.where((np.arange(n) & h) == 0, P - 1, 0).astype(np.uint64)
        return undo_stages(np.stack([np.full(n, P - 1, np.uint64), alt]), s, L)
    with ThreadPoolExecutor(16) as ex:                                  # (numpy drops the GIL on large arrays)
        return np.concatenate(list(ex.map(one, range(L)))).astype(np.uint32)


def _check_stage_map(L, mat):
    """the crafted columns really reach their targets (checked on the reference's stage map for small sizes)"""
    if L > 8:
        return
    for s in range(L):
        for k, col in enumerate((mat[2 * s], mat[2 * s + 1])):
            y = col.tolist()
            for t in range(s + 1):
                y = ref.dif_stage(y, t)
            assert set(y) == ({P - 1} if k == 0 else {0, P - 1}), f"column {2 * s + k}: stage {s} not reached"



@pytest.mark.parametrize("log_n", [3, 6, 8, 11, 12, 13, 14, 16, 17, 20, 21])
def test_lde_at_targeted_stage_values(log_n):
    import torch
    from zkir_amd import stark
    mat = stage_targets(log_n)
    w = len(mat)
    if w % 8 == 0:                                                      # a ragged last B8 block
        mat = np.concatenate([mat, np.random.default_rng(log_n).integers(0, P, (1, 1 << log_n)).astype(np.uint32)])
        w += 1
    _check_stage_map(log_n, mat)
    ctx = stark.StarkContext(log_n)
    out = stark.lde(ctx, stark.to_b8(torch.from_numpy(mat.view(np.int32)).cuda()))
    got = stark.from_b8(out, w).cpu().numpy().view(np.uint32)
    assert not out[-1, :, w % 8:].any()                                 # the zero columns of the ragged block stay zero
    ctx.close()
    with ThreadPoolExecutor(16) as ex:
        wants = list(ex.map(lambda k: so.lde(mat[k], 1)[1], range(w)))
    for k in range(w):
        assert np.array_equal(got[k], wants[k]), f"column {k} (targets stage {k // 2})"
    if log_n <= 8:                                                      # what "LDE" means, independently of both implementations
        for k in range(0, w, max(w // 6, 1)):
            assert got[k].tolist() == ref.lde_naive(mat[k].tolist()), f"column {k} against the polynomial's values on the coset"
