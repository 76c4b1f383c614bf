"""zkir_merkle_open_launch / zkir_merkle_verify_launch on the device: records against numpy indexing of the downloaded matrix and tree (tests/merkle_open_ref.py), the
device verifier against the host verifier and the oracle-built reference in both kernel forms, the proof's own query records as the bit-for-bit anchor, the other
commitment rates, the sharded composition, 64-bit offsets, and the edges of the C ABI.  The records of one shape are computed once and shared."""
from __future__ import annotations

import ctypes as C
import functools
import types

import numpy as np
import pytest

import merkle_open_ref as mref
from oracle import api as oracle, stark_api as so
from zkir_amd import runtime as rt, spec

pytestmark = pytest.mark.gpu

P = mref.P
FILL = 0xFFFFFFFF
GUARD = 0xA5A5A5A5
ROW16_MAX = 8192                                        # merkle_open.inl: MERKLE_VERIFY_ROW16_MAX — batches up to it take the 16-lanes-a-record kernel, larger ones the lane form
SHAPES = [(n, w) for n in (1, 2, 8, 1024, 2048, 1 << 17) for w in (1, 5, 8, 9, 152) if n < (1 << 17) or w in (8, 152)]


@functools.lru_cache(maxsize=None)
def _ctx():
    from zkir_amd import stark
    return stark.StarkContext(10, 1)                    # the opening calls use nothing of a context that depends on its size or rate


def _i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _indices(n, seed):
    rng = np.random.default_rng(seed)
    fixed = [0, 1 % n, n - 1, max(n // 2 - 1, 0), n // 2 % n]
    rnd = [int(x) for x in rng.integers(0, n, 64)]
    idx = fixed + rnd + [rnd[0], rnd[0]]                # a repeated index; the order is unsorted as it stands
    return np.array(idx, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _shape(n, width):
    """(B8 matrix on the device, tree on the device, column-major host matrix, host tree, indices, device records as numpy, reference records) of one shape"""
    from zkir_amd import stark
    cols = np.random.default_rng(31 * n + width).integers(0, P, (width, n), dtype=np.uint32)
    mat = stark.to_b8(_i32(cols).view(width, n))
    tree = stark.merkle_commit(_ctx(), mat, width)
    h_cols, h_tree = _u32(stark.from_b8(mat, width)), _u32(tree)
    assert np.array_equal(h_cols, cols)
    idx = _indices(n, n + width)
    got = _u32(stark.merkle_open(_ctx(), mat, tree, idx, width))
    want = np.stack([mref.open_ref(h_cols, h_tree, int(j)) for j in idx])
    return mat, tree, h_cols, h_tree, idx, got, want


@pytest.mark.parametrize("n,width", SHAPES)
def test_records_equal_reference(n, width):
    mat, tree, h_cols, h_tree, idx, got, want = _shape(n, width)
    assert got.shape == want.shape == (len(idx), width + 4 * mref.depth_of(n))
    assert np.array_equal(got, want)
    if n <= 2048:
        root, layers = so.merkle(h_cols, want_layers=True)
        assert np.array_equal(h_tree[-4:], root) and np.array_equal(h_tree, layers)


@pytest.mark.parametrize("n_idx", [1, 63, 64, 65, 1000])
def test_launch_geometry_and_untouched_tail(n_idx):
    import torch
    n, width = 2048, 9
    mat, tree, h_cols, h_tree = _shape(n, width)[:4]
    idx = np.random.default_rng(n_idx).integers(0, n, n_idx).astype(np.uint64)
    words = rt.opening_words(width, n)
    out = torch.full((n_idx * words + 64,), GUARD - (1 << 32), dtype=torch.int32, device="cuda")        # oversized and prefilled
    d_idx = _i32(idx.view(np.uint32)).view(torch.int64)
    rc = rt.lib().zkir_merkle_open_launch(_ctx().handle, mat.data_ptr(), width, n, tree.data_ptr(), d_idx.data_ptr(), n_idx, out.data_ptr(), None)
    assert rc == rt.ZKIR_OK
    torch.cuda.synchronize()
    got = _u32(out)
    assert (got[n_idx * words:] == GUARD).all(), "words past n_idx records were written"
    assert np.array_equal(got[:n_idx * words].reshape(n_idx, words), np.stack([mref.open_ref(h_cols, h_tree, int(j)) for j in idx]))


@pytest.mark.parametrize("n,width", [(8, 5), (1024, 152), (2, 8)])
def test_out_of_range_indices_read_nothing(n, width):
    """matrix and tree sit inside larger buffers prefilled with a pattern: an unguarded read shows as wrong words inside allocated memory"""
    import torch
    from zkir_amd import stark
    mat, tree, h_cols, h_tree = _shape(n, width)[:4]
    pad = 4096
    big_m = torch.full((mat.numel() + 2 * pad,), GUARD - (1 << 32), dtype=torch.int32, device="cuda")
    big_t = torch.full((tree.numel() + 2 * pad,), GUARD - (1 << 32), dtype=torch.int32, device="cuda")
    big_m[pad:pad + mat.numel()] = mat.reshape(-1)
    big_t[pad:pad + tree.numel()] = tree
    m2, t2 = big_m[pad:pad + mat.numel()].view(mat.shape), big_t[pad:pad + tree.numel()]
    idx = np.array([0, n, n - 1, n + 7, 1 % n, n, 0], dtype=np.uint64)
    got = _u32(stark.merkle_open(_ctx(), m2, t2, idx, width))
    want = np.stack([mref.open_ref(h_cols, h_tree, int(j)) for j in idx])
    assert np.array_equal(got, want)
    assert (got[[1, 3, 5]] == FILL).all() and not (got[[0, 2, 4, 6]] == FILL).all(axis=1).any()
    v, s = stark.merkle_verify(_ctx(), t2[-4:], width, n, idx, _i32(got).view(got.shape))
    assert [int(x) for x in v.cpu()] == [0, 3, 0, 3, 0, 3, 0] and [int(x) & FILL for x in s.cpu()] == [3, 1]


def _verify_dev(root, width, n, idx, rec, flags=0, summary=True):
    """verdicts / summary through the raw entry point (summary may be NULL there)"""
    import torch
    d_idx = _i32(np.asarray(idx, dtype=np.uint64).view(np.uint32)).view(torch.int64)
    d_rec = _i32(rec.reshape(-1)) if rec.size else torch.zeros(4, dtype=torch.int32, device="cuda")
    d_root = _i32(root)
    v = torch.full((len(idx) + 8,), -7, dtype=torch.int32, device="cuda")
    s = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    rc = rt.lib().zkir_merkle_verify_launch(_ctx().handle, d_root.data_ptr(), width, n, d_idx.data_ptr(), len(idx), d_rec.data_ptr(), flags, v.data_ptr(), s.data_ptr() if summary else None, None)
    assert rc == rt.ZKIR_OK, rt.lib().zkir_last_error().decode()
    torch.cuda.synchronize()
    v = v.cpu().numpy()
    assert (v[len(idx):] == -7).all()
    return v[:len(idx)].view(np.uint32), _u32(s)


@pytest.mark.parametrize("n,width", [(1, 5), (8, 9), (1024, 152), (1 << 17, 152)])
def test_device_verifier_equals_host_verifier_equals_reference(n, width):
    from zkir_amd import stark
    h_tree, idx, got = _shape(n, width)[3:6]
    root = h_tree[-4:]
    i2, r2 = mref.mutations(width, n, np.concatenate([idx, idx[:9]]), np.concatenate([got, got[:9]]), seed=n + width)      # 80 positions: ten rounds of the eight kinds
    i_all, r_all = np.concatenate([idx, i2]), np.concatenate([got, r2])
    want_v, want_s = mref.verify_all_ref(root, width, n, i_all, r_all)
    assert not want_v[:len(idx)].any() and set(int(x) for x in want_v) == ({0, 2, 3} if n == 1 else {0, 1, 2, 3})
    hv, hs = rt.merkle_verify_host(root, width, n, i_all, r_all)
    assert np.array_equal(hv, want_v) and np.array_equal(hs, want_s)
    for flags in (stark.VERIFY_FORM_LANE, stark.VERIFY_FORM_ROW16, 0):                      # both forms by name, then the library's rule
        v, s = _verify_dev(root, width, n, i_all, r_all, flags)
        assert np.array_equal(v, want_v) and np.array_equal(s, want_s), (flags, v, want_v, s, want_s)
        v, s = _verify_dev(root, width, n, i_all, r_all, flags, summary=False)
        assert np.array_equal(v, want_v) and (s.view(np.int32) == -7).all()               # summary = NULL: nothing written there
        v, s = _verify_dev(root, width, n, i_all[len(idx) + 1:len(idx) + 2], r_all[len(idx) + 1:len(idx) + 2], flags)      # n_idx = 1: a word set to p
        assert list(v) == [2] and list(s) == [1, 0]
    v, s = _verify_dev(root, width, n, idx[:1], got[:1])
    assert list(v) == [0] and list(s) == [0, FILL]
    if n == 1 << 17:
        return
    # both sides of the batch threshold: the same batch tiled past it; the untouched records lead, so the first failure keeps its position
    reps = (ROW16_MAX + 1) // len(i_all) + 1
    i_big, r_big, v_big = np.tile(i_all, reps), np.tile(r_all, (reps, 1)), np.tile(want_v, reps)
    for n_idx in (ROW16_MAX, ROW16_MAX + 1, len(i_big)):
        for flags in (0, stark.VERIFY_FORM_LANE, stark.VERIFY_FORM_ROW16):
            v, s = _verify_dev(root, width, n, i_big[:n_idx], r_big[:n_idx], flags)
            assert np.array_equal(v, v_big[:n_idx]) and list(s) == [int(np.count_nonzero(v_big[:n_idx])), int(want_s[1])], (n_idx, flags)


def test_digest_form_verifier_on_the_device():
    from zkir_amd import stark
    n = 8
    h_tree = _shape(n, 9)[3]
    tree = _shape(n, 9)[1]
    idx = np.arange(n, dtype=np.uint64)
    got = _u32(stark.merkle_open(_ctx(), None, tree, idx))
    assert np.array_equal(got, np.stack([mref.open_ref(None, h_tree, int(j)) for j in idx]))
    i2, r2 = mref.mutations(0, n, np.tile(idx, 4), np.tile(got, (4, 1)), flags=mref.LEAF_DIGEST, seed=3)
    want_v, want_s = mref.verify_all_ref(h_tree[-4:], 0, n, i2, r2, mref.LEAF_DIGEST)
    for form in (stark.VERIFY_FORM_LANE, stark.VERIFY_FORM_ROW16):
        v, s = _verify_dev(h_tree[-4:], 0, n, i2, r2, stark.OPEN_LEAF_DIGEST | form)
        assert np.array_equal(v, want_v) and np.array_equal(s, want_s)
    v, s = _verify_dev(h_tree[-4:], 0, 1, [0, 0], np.stack([h_tree[-4:], h_tree[:4]]), stark.OPEN_LEAF_DIGEST)      # depth 0: the leaf is the root
    assert list(v) == [0, 1]


@pytest.mark.parametrize("n", [300, 5000])
def test_proof_records_are_the_openings_of_the_committed_trace(n):
    import torch
    from zkir_amd import stark
    blob = spec.fib_endless_program().to_bytes()
    res = rt.VM(blob, [], rt.VMConfig(max_cycles=n, enable_execution_trace=True)).run()     # zkir_exec
    log_n = stark.padded_log_n(res.cycles)
    ctx = stark.StarkContext(log_n, 1)
    try:
        proof = stark.prove(ctx, res.execution_trace.columns, res.public_inputs())
        assert rt.verify(proof) == 0
        q = mref.proof_queries(proof, log_n)
        tr = types.SimpleNamespace(n_rows=res.execution_trace.n_rows, c=res.execution_trace.columns, cycle=torch.empty(0, device="cuda"))
        root, L, tree = stark.commit_trace(ctx, tr)
        assert np.array_equal(root, q["roots"]["trace"])
        got = _u32(stark.merkle_open(ctx, L, tree, q["indices"]["trace"], stark.W_MAIN))
        assert np.array_equal(got, q["records"]["trace"])                                  # word for word
        v, s = stark.merkle_verify(ctx, tree[-4:], stark.W_MAIN, q["n_leaves"], q["indices"]["trace"], _i32(got).view(got.shape))
        assert not v.cpu().numpy().any() and [int(x) & FILL for x in s.cpu()] == [0, FILL]
        for c in ("aux", "quotient"):
            rec = q["records"][c]
            v, s = stark.merkle_verify(ctx, _i32(q["roots"][c]), q["widths"][c], q["n_leaves"], q["indices"][c], _i32(rec).view(rec.shape))
            assert not v.cpu().numpy().any() and [int(x) & FILL for x in s.cpu()] == [0, FILL], c
    finally:
        ctx.close()
        res.close()


def test_other_rates():
    import torch
    from zkir_amd import stark
    n = 1000
    blob = spec.fib_endless_program().to_bytes()
    res = rt.VM(blob, [], rt.VMConfig(max_cycles=n, enable_execution_trace=True)).run()
    ores = oracle.run(blob, enable_execution_trace=True, max_cycles=n)
    tr = types.SimpleNamespace(n_rows=res.execution_trace.n_rows, c=res.execution_trace.columns, cycle=torch.empty(0, device="cuda"))
    rows = {}
    base = np.random.default_rng(5).integers(0, 1024 << 1, 50).astype(np.uint64)            # 50 seeded rows of the blow-up-2 domain
    try:
        for b in (1, 2, 3):
            ctx = stark.StarkContext(10, b)
            try:
                root, L, tree = stark.commit_trace(ctx, tr)
                m = 1024 << b
                idx = base << np.uint64(b - 1)                                              # row 2j at rate b is row j at rate b - 1
                rec = stark.merkle_open(ctx, L, tree, idx, stark.W_MAIN)
                got = _u32(rec)
                rows[b] = got[:, :stark.W_MAIN]
                v, s = stark.merkle_verify(ctx, tree[-4:], stark.W_MAIN, m, idx, rec)
                assert not v.cpu().numpy().any()
                hv, hs = rt.merkle_verify_host(root, stark.W_MAIN, m, idx, got)
                assert not hv.any() and list(hs) == [0, FILL]
                if b > 1:
                    want_root, want_L = so.commit_trace(ores.rows, b, want_lde=True)
                    assert np.array_equal(root, want_root) and np.array_equal(rows[b], want_L[:, idx.astype(np.int64)].T)
                    assert np.array_equal(rows[b], rows[b - 1])
            finally:
                ctx.close()
    finally:
        res.close()


def test_sharded_commitment_composes():
    import torch
    from zkir_amd import stark
    G, nl, width = 4, 1024, 152
    ctx = _ctx()
    cols = [np.random.default_rng(900 + g).integers(0, P, (width, nl), dtype=np.uint32) for g in range(G)]
    mats = [stark.to_b8(_i32(c).view(width, nl)) for c in cols]
    trees = [stark.merkle_commit(ctx, m, width) for m in mats]
    cap = torch.empty(4 * (2 * G - 1), dtype=torch.int32, device="cuda")
    cap[:4 * G] = torch.cat([t[-4:] for t in trees])
    assert rt.lib().zkir_merkle_cap_launch(ctx.handle, cap.data_ptr(), G, None) == rt.ZKIR_OK
    assert torch.equal(cap[-4:], stark.merkle_cap(ctx, torch.stack([t[-4:] for t in trees])))
    cap_rec = stark.merkle_open(ctx, None, cap, np.arange(G))                               # the digest form
    whole = stark.to_b8(_i32(np.concatenate(cols, axis=1)).view(width, G * nl))
    whole_tree = stark.merkle_commit(ctx, whole, width)
    assert torch.equal(whole_tree[-4:], cap[-4:])
    js = np.array([0, 1, 511, 512, 1023, 700], dtype=np.uint64)
    for g in range(G):
        assert torch.equal(cap_rec[g, :4], trees[g][-4:])                                   # the record's digest is the shard root
        local = stark.merkle_open(ctx, mats[g], trees[g], js, width)
        composed = torch.cat([local, cap_rec[g, 4:].expand(len(js), -1)], dim=1).contiguous()
        gidx = js + np.uint64(g * nl)
        assert torch.equal(composed, stark.merkle_open(ctx, whole, whole_tree, gidx, width))
        v, s = stark.merkle_verify(ctx, cap[-4:], width, G * nl, gidx, composed)
        assert not v.cpu().numpy().any()
    v, s = stark.merkle_verify(ctx, cap[-4:], 0, G, np.arange(G), cap_rec, stark.OPEN_LEAF_DIGEST)
    assert not v.cpu().numpy().any()


def test_offsets_past_32_bits():
    """the smallest shape where (b n + j) 8 passes 2^32: 2^22 leaves x 129 blocks"""
    import torch
    from zkir_amd import stark
    free = torch.cuda.mem_get_info()[0]
    if free < 40 << 30:
        pytest.skip(f"needs 40 GB of free device memory for a 17.3 GB matrix; {free >> 30} GB free")
    n, width = 1 << 22, 1032
    nb = width // 8
    mat = torch.empty((nb, n, 8), dtype=torch.int32, device="cuda")
    ar = torch.arange(n * 8, dtype=torch.int64, device="cuda")
    for b in range(nb):
        mat[b] = ((ar * 2654435761 + b * 40503 + 17) % P).to(torch.int32).view(n, 8)       # a seeded pattern: every block different
    del ar
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    tree = torch.randint(0, P, (4 * (2 * n - 1),), dtype=torch.int32, device="cuda", generator=g)      # a pattern that was not computed: the kernel only reads it
    idx = np.array([0, 1, n - 1, n // 2, n // 2 - 1, 123457, 4000001, n - 2], dtype=np.uint64)
    rec = stark.merkle_open(_ctx(), mat, tree, idx, width)
    torch.cuda.synchronize()
    assert rec.shape == (8, width + 4 * 22)
    for k, j in enumerate(int(x) for x in idx):
        assert ((nb - 1) * n + j) * 8 >= 1 << 32 > ((nb - 2) * n + j) * 8                 # the last block's words sit past 2^32, the one before it just below
        assert torch.equal(rec[k, width - 16:width], mat[nb - 2:, j, :].reshape(-1)), j     # the last two blocks
        assert torch.equal(rec[k, :8], mat[0, j, :])
        for lvl in range(22):
            at = mref.level_start(n, lvl) + 4 * ((j >> lvl) ^ 1)
            assert torch.equal(rec[k, width + 4 * lvl:width + 4 * lvl + 4], tree[at:at + 4]), (j, lvl)
    del mat, tree
    torch.cuda.empty_cache()


def test_error_returns_come_before_any_launch():
    import torch
    L = rt.lib()
    n, width = 8, 9
    mat, tree, _, h_tree, idx, got, _ = _shape(n, width)
    d_idx = _i32(idx.view(np.uint32)).view(torch.int64)
    out = torch.full((got.size,), -7, dtype=torch.int32, device="cuda")
    h, m, t, i, o = _ctx().handle, mat.data_ptr(), tree.data_ptr(), d_idx.data_ptr(), out.data_ptr()
    for args in [(None, m, width, n, t, i, 4, o, None), (h, m, width, n, None, i, 4, o, None), (h, m, width, n, t, None, 4, o, None), (h, m, width, n, t, i, 4, None, None),
                 (h, m, width, 0, t, i, 4, o, None), (h, m, width, 3, t, i, 4, o, None), (h, None, width, n, t, i, 4, o, None)]:
        assert L.zkir_merkle_open_launch(*args) == rt.ERR_ARGUMENT
        assert "zkir_merkle_open_launch" in L.zkir_last_error().decode()
    v = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    r = tree[-4:].contiguous().data_ptr()
    d_rec = _i32(got.reshape(-1))
    for args in [(None, r, width, n, i, 4, d_rec.data_ptr(), 0, v.data_ptr(), None, None), (h, None, width, n, i, 4, d_rec.data_ptr(), 0, v.data_ptr(), None, None),
                 (h, r, width, n, None, 4, d_rec.data_ptr(), 0, v.data_ptr(), None, None), (h, r, width, n, i, 4, None, 0, v.data_ptr(), None, None),
                 (h, r, width, n, i, 4, d_rec.data_ptr(), 0, None, None, None), (h, r, width, 0, i, 4, d_rec.data_ptr(), 0, v.data_ptr(), None, None),
                 (h, r, width, 3, i, 4, d_rec.data_ptr(), 0, v.data_ptr(), None, None)]:
        assert L.zkir_merkle_verify_launch(*args) == rt.ERR_ARGUMENT
        assert "zkir_merkle_verify_launch" in L.zkir_last_error().decode()
    assert L.zkir_merkle_open_launch(h, m, width, n, t, i, 0, o, None) == rt.ZKIR_OK        # n_idx = 0: nothing to do
    torch.cuda.synchronize()
    assert (out == -7).all() and (v == -7).all()                                           # none of the calls above wrote anything


def test_two_streams_interleave_on_one_context():
    import torch
    from zkir_amd import stark
    n, width = 2048, 152
    mat, tree, _, h_tree, idx, got, _ = _shape(n, width)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for k in range(6):
        st = s1 if k % 2 == 0 else s2
        with torch.cuda.stream(st):
            rec = stark.merkle_open(_ctx(), mat, tree, idx, width, stream=st)
            v, s = stark.merkle_verify(_ctx(), tree[-4:], width, n, idx, rec, stark.VERIFY_FORM_ROW16 if k % 3 else stark.VERIFY_FORM_LANE, stream=st)
            outs.append((rec, v, s))
    torch.cuda.synchronize()
    for rec, v, s in outs:
        assert np.array_equal(_u32(rec), got) and not v.cpu().numpy().any() and [int(x) & FILL for x in s.cpu()] == [0, FILL]
