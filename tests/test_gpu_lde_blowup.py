"""Commitments at blow-up 4 and 8 (StarkContext(log_n, log_blowup = 2, 3)): stark.lde against the oracle's so.lde(col, b), byte for byte, over every kernel
combination lde_run can pick — the small kernel (log_n 1, 3, 6, 9), the blow-up middle kernel as the last forward kernel (10), a lone stage (11), register passes
(12, 13), the LDS passes and their splits (14, 15 = 3 + 2, 17 = 4 + 3, 20 = one ten-stage pass); nesting against the shipped blow-up-2 kernels at the workload's own
width; the Merkle tree at the new leaf counts; the commitment of a trace; and the edges of the C ABI.  The reference of one (size, rate) is computed once and shared
by the widths."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bigint_ref as ref
from oracle import api as oracle, stark_api as so
from zkir_amd import runtime as rt, spec

pytestmark = pytest.mark.gpu

P = 0x78000001
BLOWUPS = [2, 3]
LOG_NS = [1, 3, 6, 9, 10, 11, 12, 13, 14, 15, 17, 20]
KINDS = ["all_pm1", "all_zero", "alt_0_pm1", "one_first", "one_middle", "one_last"]


def _widths(log_n):
    """8 and 152, plus the ragged 5 (its block's zero columns stay zero) up to 2^15; 2^20 gets eight columns: the oracle costs 2.9 s a column there at blow-up 8"""
    return [8] if log_n == 20 else ([8, 152, 5] if log_n <= 15 else [8, 152])


def _column(kind, n):
    c = np.zeros(n, np.uint32)
    if kind == "all_pm1":
        c[:] = P - 1
    elif kind == "alt_0_pm1":
        c[1::2] = P - 1
    elif kind == "one_first":
        c[0] = 1
    elif kind == "one_last":
        c[n - 1] = 1
    elif kind == "one_middle":
        c[n // 2] = 1
    else:
        assert kind == "all_zero"
    return c


def _reference(log_n, b):
    """(the fixed columns and their extensions, the seeded random columns and theirs): one pool of 16 threads over all of them (the oracle call releases the GIL)"""
    n, w = 1 << log_n, max(_widths(log_n))
    fixed = [_column(k, n) for k in KINDS]
    rnd = np.random.default_rng(2000 + log_n).integers(0, P, (w, n), dtype=np.uint32)
    cols = fixed + [rnd[k] for k in range(w)]
    so.lib()                                                           # the oracle loads and binds its library on first use, unguarded: on this thread, before the pool
    with ThreadPoolExecutor(16) as ex:
        ext = list(ex.map(lambda c: so.lde(c, b)[1], cols))
    return fixed, ext[:len(KINDS)], rnd, np.stack(ext[len(KINDS):])


def _lde(ctx, mat):
    import torch
    from zkir_amd import stark
    return stark.lde(ctx, stark.to_b8(torch.from_numpy(np.ascontiguousarray(mat).view(np.int32)).cuda()))


@pytest.mark.parametrize("log_n,b", [(l, b) for l in LOG_NS for b in BLOWUPS])
def test_lde_equals_oracle(log_n, b):
    from zkir_amd import stark
    n = 1 << log_n
    fixed, fixed_ext, rnd, rnd_ext = _reference(log_n, b)
    if log_n <= 7:                                                     # the oracle against the extension by definition
        for col, ext in list(zip(fixed, fixed_ext)) + [(rnd[0], rnd_ext[0])]:
            assert ext.tolist() == ref.lde_naive([int(v) for v in col], b)
    ctx = stark.StarkContext(log_n, b)
    try:
        assert ctx.log_blowup == b == rt.lib().zkir_stark_ctx_log_blowup(ctx.handle)
        for width in _widths(log_n):
            for i, kind in enumerate(KINDS + ["random"]):
                if kind == "random":
                    mat, want = rnd[:width], rnd_ext[:width]
                else:
                    mat, want = np.broadcast_to(fixed[i], (width, n)), fixed_ext[i][None, :]
                out = _lde(ctx, mat)
                assert tuple(out.shape) == ((width + 7) // 8, n << b, 8)
                assert not out[-1, :, (width - 1) % 8 + 1:].any(), f"log_n {log_n}, b {b}, width {width}, input {kind}: a zero column of the ragged block is not zero"
                got = stark.from_b8(out, width).cpu().numpy().view(np.uint32)
                del out
                bad = np.flatnonzero((got != want).any(axis=1))
                assert bad.size == 0, f"log_n {log_n}, b {b}, width {width}, input {kind}: columns {bad[:8].tolist()} differ from the oracle"
                assert int(got.max()) < P, f"log_n {log_n}, b {b}, width {width}, input {kind}: a word is not canonical"
    finally:
        ctx.close()


@pytest.mark.parametrize("log_n", [10, 13, 16, 20])
def test_extensions_nest_with_the_shipped_kernels(log_n):
    """rows 0, 2, 4 .. of the extension at b are the extension at b - 1: b = 2 against the blow-up-2 kernels, b = 3 against b = 2; width 152, compared on the device"""
    import torch
    from zkir_amd import stark
    n, width = 1 << log_n, 152
    mat = stark.to_b8(torch.from_numpy(np.random.default_rng(3000 + log_n).integers(0, P, (width, n), dtype=np.uint32).view(np.int32)).cuda())
    prev = None
    for b in (1, 2, 3):
        ctx = stark.StarkContext(log_n, b)
        try:
            cur = stark.lde(ctx, mat)
        finally:
            ctx.close()
        assert tuple(cur.shape) == (width // 8, n << b, 8)
        if prev is not None:
            differ = (cur[:, ::2, :] != prev).any(dim=2).any(dim=0)
            assert not bool(differ.any()), f"log_n {log_n}: rows {(2 * torch.nonzero(differ)[:8, 0]).tolist()} at log_blowup {b} are not the rows of log_blowup {b - 1}"
            assert int(cur.max()) < P and int(cur.min()) >= 0
        prev = cur


@pytest.mark.parametrize("width,log_n", [(152, 8), (17, 10)])
@pytest.mark.parametrize("b", BLOWUPS)
def test_merkle_at_the_new_leaf_counts(width, log_n, b):
    from zkir_amd import stark
    mat = np.random.default_rng(width + b).integers(0, P, (width, 1 << log_n), dtype=np.uint32)
    ctx = stark.StarkContext(log_n, b)
    try:
        L = _lde(ctx, mat)
        tree = stark.merkle_commit(ctx, L, width).cpu().numpy().view(np.uint32)
        ext = stark.from_b8(L, width).cpu().numpy().view(np.uint32)
    finally:
        ctx.close()
    assert ext.shape == (width, (1 << log_n) << b)
    root, layers = so.merkle(ext, want_layers=True)
    assert np.array_equal(tree, layers) and np.array_equal(tree[-4:], root)


PROGRAMS = {"fib": (spec.fib_endless_program, {}), "sha": (spec.sha256_chain_program, {}), "deferred": (spec.fib_endless_program, {"enable_deferred_model": True})}


def _case(name, n):
    """(log, device trace, oracle rows, oracle public inputs, product public inputs) of program `name` run for n cycles"""
    from zkir_amd import pipeline as pl
    mk, cfg = PROGRAMS[name]
    blob = mk().to_bytes()
    log = rt.interpret(blob, [], rt.VMConfig(enable_execution_trace=True, max_cycles=n, **cfg))
    ddl = pl.upload(log)
    tr = pl.DeviceTrace(ddl)
    pl.trace_fill(pl.trace_fill_args(ddl, tr))
    res = oracle.run(blob, enable_execution_trace=True, max_cycles=n, **cfg)
    deferred = bool(cfg.get("enable_deferred_model"))
    opub = so.public_inputs(len(res.rows), blob, [], list(res.outputs), (res.halt_kind, res.halt_code), deferred=deferred)
    return log, tr, res.rows, opub, rt.public_inputs(log, blob, [], deferred)


@pytest.mark.parametrize("name,n", [("fib", 1000), ("fib", 4096), ("sha", 700), ("deferred", 256)])
def test_commit_of_a_trace_matches_oracle(name, n):
    from zkir_amd import stark
    log, tr, rows, opub, pub = _case(name, n)
    deferred = bool(opub.deferred)
    wm = stark.main_width(deferred)
    k = stark.padded_log_n(len(rows))
    for b in BLOWUPS:
        want_root, want_L = so.commit_trace(rows, b, want_lde=True, pub=opub)                 # on the CPU first: existing tests run only its b = 1 form
        assert want_L.shape == (wm, (1 << k) << b)
        ctx = stark.StarkContext(k, b)
        try:
            root, L, tree = stark.commit_trace(ctx, tr, deferred=deferred)
            assert np.array_equal(stark.from_b8(L, wm).cpu().numpy().view(np.uint32), want_L), f"{name} {n}: the extension at log_blowup {b}"
            assert np.array_equal(root, want_root), f"{name} {n}: the root at log_blowup {b}"
            assert tree.numel() == 4 * (2 * ((1 << k) << b) - 1)
        finally:
            ctx.close()
    log.close()


def _create(log_n, b):
    import ctypes as C
    h = C.c_void_p()
    rc = rt.lib().zkir_stark_ctx_create(log_n, b, C.byref(h))
    return rc, h, rt.lib().zkir_last_error().decode()


def test_context_argument_edges():
    import torch
    from zkir_amd import pipeline as pl
    pl._require_gpu()
    torch.cuda.synchronize()
    for log_n, b in [(10, 0), (10, 4), (26, 2), (25, 3), (27, 1), (0, 2)]:
        before = torch.cuda.mem_get_info()[0]
        rc, h, msg = _create(log_n, b)
        assert rc == rt.ERR_ARGUMENT and not h.value, (log_n, b)
        assert "log_n <= 26" in msg and "log_n + log_blowup <= 27" in msg, msg                   # both limits named
        assert torch.cuda.mem_get_info()[0] == before, f"({log_n}, {b}): refused, but device memory was taken"
    for b in (1, 2, 3):
        rc, h, _ = _create(12, b)
        assert rc == rt.ZKIR_OK and rt.lib().zkir_stark_ctx_log_blowup(h) == b
        rt.lib().zkir_stark_ctx_free(h)
    assert rt.lib().zkir_stark_ctx_log_blowup(None) == 0


def test_prover_refuses_a_context_of_another_rate():
    """proofs are blow-up 2: the refusal comes from the library, before any launch, and the same trace then proves on a context of log_blowup 1"""
    import ctypes as C
    import torch
    from zkir_amd import stark
    log, tr, rows, opub, pub = _case("fib", 64)
    ctx2 = stark.StarkContext(6, 2)
    try:
        with pytest.raises(rt.RuntimeError) as e:
            stark.prove(ctx2, tr, pub)
        assert e.value.code == rt.ERR_ARGUMENT and "blow-up 2" in e.value.message and "zkir_prove" in e.value.message
        # the experiments built on the prover's LDE refuse it the same way
        sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        buf = torch.zeros(1 << 12, dtype=torch.int32, device="cuda")
        assert rt.lib().zkir_ntt_strided_variant_launch(ctx2.handle, C.c_void_p(buf.data_ptr()), 8, 0, 0, sp) == rt.ERR_ARGUMENT
        assert "blow-up 2" in rt.lib().zkir_last_error().decode()
        lib = rt.lib()
        n = 64
        m = torch.zeros((stark.W_MAIN // 8, n, 8), dtype=torch.int32, device="cuda")
        L = torch.full((stark.W_MAIN // 8, n << 2, 8), -1, dtype=torch.int32, device="cuda")
        tree = torch.full((4 * (2 * (n << 2) - 1),), -1, dtype=torch.int32, device="cuda")
        V = C.c_void_p
        lib.zkir_commit_fused01_launch.restype = C.c_int
        lib.zkir_commit_fused01_launch.argtypes = [V, V, C.c_uint64, V, C.c_uint32, V, V]
        assert lib.zkir_commit_fused01_launch(ctx2.handle, C.byref(tr.c), n, m.data_ptr(), stark.W_MAIN, L.data_ptr(), sp) == rt.ERR_ARGUMENT
        assert "zkir_commit_fused01_launch" in lib.zkir_last_error().decode() and "blow-up 2" in lib.zkir_last_error().decode()
        lib.zkir_commit_overlapped_launch.restype = C.c_int
        lib.zkir_commit_overlapped_launch.argtypes = [V, V, C.c_uint32, V, V, C.c_uint32, V]
        assert lib.zkir_commit_overlapped_launch(ctx2.handle, m.data_ptr(), stark.W_MAIN, L.data_ptr(), tree.data_ptr(), 4, sp) == rt.ERR_ARGUMENT
        assert "zkir_commit_overlapped_launch" in lib.zkir_last_error().decode() and "blow-up 2" in lib.zkir_last_error().decode()
        torch.cuda.synchronize()
        assert bool((L == -1).all()) and bool((tree == -1).all()) and not bool(m.any())           # refused before any launch: nothing was written
    finally:
        ctx2.close()
    ctx1 = stark.StarkContext(6)
    try:
        proof = stark.prove(ctx1, tr, pub)
        assert rt.verify(proof, pub) == 0 and np.array_equal(proof, so.prove(rows, opub))
    finally:
        ctx1.close()
    log.close()


def test_contexts_of_different_rates_alive_at_once():
    from zkir_amd import stark
    log_n, width = 12, 16
    mat = np.random.default_rng(12).integers(0, P, (width, 1 << log_n), dtype=np.uint32)
    alone = {}
    for b in (1, 2, 3):
        ctx = stark.StarkContext(log_n, b)
        L = _lde(ctx, mat)
        alone[b] = (L.clone(), stark.merkle_commit(ctx, L, width).clone())
        ctx.close()
    ctxs = {b: stark.StarkContext(log_n, b) for b in (3, 1, 2)}
    try:
        for _ in range(2):
            for b in (2, 3, 1):
                L = _lde(ctxs[b], mat)
                tree = stark.merkle_commit(ctxs[b], L, width)
                assert bool((L == alone[b][0]).all()) and bool((tree == alone[b][1]).all()), f"log_blowup {b} next to the other contexts"
    finally:
        for c in ctxs.values():
            c.close()
    want = np.stack([so.lde(mat[k], 3)[1] for k in range(width)])
    assert np.array_equal(stark.from_b8(alone[3][0], width).cpu().numpy().view(np.uint32), want)


def test_service_commits_at_the_context_rate_and_proves_at_blow_up_2_only():
    """service.prove_many(.., commit_only=True, log_blowup=2): per job the root stark.commit_trace gives on a context of that rate (and the oracle's); full proofs at
    another rate are refused before anything runs, with an own context or a given one"""
    from zkir_amd import pipeline as pl, service, stark
    k = 9
    cfg = rt.VMConfig(max_cycles=1 << k, enable_execution_trace=True)
    ragged = rt.VMConfig(max_cycles=(1 << k) - 77, enable_execution_trace=True)
    jobs = [(spec.fib_endless_program().to_bytes(), [], cfg), (spec.sha256_chain_program().to_bytes(), [], ragged)] * 2
    rep = service.prove_many(jobs, k, producers=2, commit_only=True, log_blowup=2)
    assert len(rep.proofs) == 4
    ctx = stark.StarkContext(k, 2)
    try:
        for (blob, inputs, c), root in zip(jobs[:2], rep.proofs[:2]):
            log = rt.interpret(blob, inputs, c)
            ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
            assert np.array_equal(root, stark.commit_trace(ctx, tr)[0])
            res = oracle.run(blob, enable_execution_trace=True, max_cycles=c.max_cycles)
            opub = so.public_inputs(len(res.rows), blob, [], list(res.outputs), (res.halt_kind, res.halt_code))
            assert np.array_equal(root, so.commit_trace(res.rows, 2, pub=opub))
            log.close()
        assert np.array_equal(rep.proofs[0], rep.proofs[2]) and np.array_equal(rep.proofs[1], rep.proofs[3]) and not np.array_equal(rep.proofs[0], rep.proofs[1])
        ctx3 = stark.StarkContext(k, 3)
        rep3 = service.prove_many(jobs[:1], k, producers=1, commit_only=True, ctx=ctx3)       # a given context brings its own rate
        ctx3.close()
        assert not np.array_equal(rep3.proofs[0], rep.proofs[0])
        for kw in ({"log_blowup": 2}, {"ctx": ctx}):
            with pytest.raises(rt.RuntimeError) as e:
                service.prove_many(jobs[:1], k, producers=1, **kw)
            assert e.value.code == rt.ERR_ARGUMENT and "blow-up 2" in e.value.message
    finally:
        ctx.close()
