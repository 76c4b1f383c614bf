"""GPU parity for the self-defined prover stages (stark.hip) against oracle/stark_oracle.cpp, bit-exact.
(The reference has no prover: these stages are 'parity unpinned' vs seceq/zkir; the oracle is pinned by the
algebraic self-checks in tests/test_stark_oracle.py.)"""
import numpy as np
import pytest

from oracle import api as oracle, stark_api as so
from zkir_amd import runtime as rt, spec

import programs

pytestmark = pytest.mark.gpu
P = so.P


def _device_trace(blob, n, inputs=(), **cfg):
    from zkir_amd import pipeline as pl
    log = rt.interpret(blob, inputs, rt.VMConfig(max_cycles=n, enable_execution_trace=True, **cfg))
    assert log.n_rows == n
    ddl = pl.upload(log)
    tr = pl.DeviceTrace(ddl)
    pl.trace_fill(pl.trace_fill_args(ddl, tr))
    return log, tr


@pytest.mark.parametrize("log_n", [3, 6, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23])
def test_lde_matches_oracle(log_n):
    import torch
    from zkir_amd import stark
    # ragged last block; every pass structure of run_strided_stages: log_n - 10 strided stages = a lone stage (11), register passes of 2 / 3 stages
    # (12, 13, 15 = 3 + 2), LDS radix-4 passes of 4 / 6 / 8 / 10 stages (14, 16, 18, 20) and their combinations (17 = 4 + 3, 19 = 6 + 3, 21 = 8 + 3,
    # 22 = 10 + 2, 23 = 10 + 3)
    n, w = 1 << log_n, 5 if log_n < 14 else (11 if log_n < 16 else (4 if log_n < 22 else 2))
    rng = np.random.default_rng(log_n)
    mat = rng.integers(0, P, (w, n)).astype(np.uint32)
    mat[1] = 0
    if w > 3:
        mat[2] = 1; mat[3] = np.arange(n) % P
    ctx = stark.StarkContext(log_n)
    out = stark.lde(ctx, stark.to_b8(torch.from_numpy(mat.view(np.int32)).cuda()))
    got = stark.from_b8(out, w).cpu().numpy().view(np.uint32)
    assert not out[0, :, w:].any()                                 # the zero columns of a ragged block stay zero
    for k in range(w):
        assert np.array_equal(got[k], so.lde(mat[k], 1)[1]), f"column {k}"
    # the extension restricted to even positions of a 2N-NTT of the coefficients is the trace itself on a shifted domain:
    # cheaper size-independent property: constant column stays constant
    assert not got[1].any() and (w < 4 or (got[2] == 1).all())
    ctx.close()


@pytest.mark.parametrize("log_n,width", [(4, 1), (6, 8), (7, 9), (8, 89), (8, 152), (8, 168), (10, 17)])
def test_merkle_matches_oracle(log_n, width):
    import torch
    from zkir_amd import stark
    n = 1 << log_n
    mat = np.random.default_rng(width).integers(0, P, (width, n)).astype(np.uint32)
    ctx = stark.StarkContext(max(log_n - 1, 1))
    tree = stark.merkle_commit(ctx, stark.to_b8(torch.from_numpy(mat.view(np.int32)).cuda()), width).cpu().numpy().view(np.uint32)
    root, layers = so.merkle(mat, want_layers=True)
    assert np.array_equal(tree, layers)
    assert np.array_equal(tree[-4:], root)
    ctx.close()


def test_trees_of_one_context_built_on_two_streams_at_once():
    """subtree_kernel's "who finishes last" counter was one word per context, shared by launches that overlap when a context's trees are built on two
    streams (service.py's commit_only pipeline; any caller of zkir_merkle_commit_launch / zkir_merkle_cap_launch with its own streams).  Now every launch takes its own slot
    of a ring.  Here: trees of 2^13 .. 2^17 leaves (8 .. 128 workgroups per subtree launch; narrow matrices, so the leaf layer is short and the launches of the two
    streams really are in flight together), queued alternately on two streams of ONE context, repeatedly; every tree must equal the one built alone on the default stream."""
    import torch
    from zkir_amd import stark
    ctx = stark.StarkContext(10)
    rng = np.random.default_rng(7)
    mats, want = [], []
    for i, log_n in enumerate([13, 14, 15, 16, 17, 13, 15, 14]):
        m = stark.to_b8(torch.from_numpy(rng.integers(0, P, (8, 1 << log_n)).astype(np.uint32).view(np.int32)).cuda())
        mats.append(m)
        want.append(stark.merkle_commit(ctx, m, 8).cpu().numpy().view(np.uint32))
        if log_n <= 14:
            root, layers = so.merkle(stark.from_b8(m, 8).cpu().numpy().view(np.uint32), want_layers=True)
            assert np.array_equal(want[-1], layers)
    digs = [m[0, :4096, :4].contiguous() for m in mats]
    want_caps = [stark.merkle_cap(ctx, d).clone() for d in digs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for rep in range(20):
        trees = []
        for i, m in enumerate(mats):
            with torch.cuda.stream(streams[i & 1]):
                trees.append(stark.merkle_commit(ctx, m, 8, stream=streams[i & 1]))
        caps = []
        for i in range(8):                                          # the cap launch (zkir_merkle_cap_launch) on the two streams as well: 2^12 digests = 4 workgroups
            with torch.cuda.stream(streams[i & 1]):
                caps.append(stark.merkle_cap(ctx, digs[i], stream=streams[i & 1]).clone())
        torch.cuda.synchronize()
        for i, t in enumerate(trees):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), want[i]), f"rep {rep}, tree {i}"
        for i in range(8):
            assert torch.equal(caps[i], want_caps[i]), f"rep {rep}, cap {i}"
    ctx.close()


@pytest.mark.parametrize("fill", ["p-1", "zero", "one", "alternating"])
def test_merkle_and_lde_extreme_values(fill):
    """Worst cases for the lazy (unreduced) arithmetic of the hash and NTT kernels: every input at the top of the range."""
    import torch
    from zkir_amd import stark
    log_n, width = 9, 168
    n = 1 << log_n
    mat = np.zeros((width, n), dtype=np.uint32)
    if fill == "p-1":
        mat[:] = P - 1
    elif fill == "one":
        mat[:] = 1
    elif fill == "alternating":
        mat[:, ::2] = P - 1; mat[::2, 1::2] = P - 2
    ctx = stark.StarkContext(log_n)
    tree = stark.merkle_commit(ctx, stark.to_b8(torch.from_numpy(mat.view(np.int32)).cuda()), width).cpu().numpy().view(np.uint32)
    root, layers = so.merkle(mat, want_layers=True)
    assert np.array_equal(tree, layers)
    got = stark.from_b8(stark.lde(ctx, stark.to_b8(torch.from_numpy(mat[:3].copy().view(np.int32)).cuda())), 3).cpu().numpy().view(np.uint32)
    for k in range(3):
        assert np.array_equal(got[k], so.lde(mat[k], 1)[1])
    ctx.close()


PROGRAMS = {"fib": (spec.fib_endless_program, {}), "sha": (spec.sha256_chain_program, {}), "deferred": (spec.fib_endless_program, {"enable_deferred_model": True}),
            "cmp": (spec.compare_loop_program, {}), "cmp_deferred": (spec.compare_loop_program, {"enable_deferred_model": True}),
            "call": (spec.call_loop_program, {}), "call_deferred": (spec.call_loop_program, {"enable_deferred_model": True}),
            "sgn": (spec.signed_loop_program, {}), "sgn_deferred": (spec.signed_loop_program, {"enable_deferred_model": True}),
            "cmov": (spec.cmov_loop_program, {}), "cmov_deferred": (spec.cmov_loop_program, {"enable_deferred_model": True}),
            "fib30": (lambda: spec.fib_program(30), {}), "exit42": (lambda: spec.Program.from_code([spec.addi(10, 0, 0), spec.addi(11, 0, 42), spec.ecall()]), {})}


def _case(name, n):
    """(blob, cfg, device trace, oracle rows, oracle public inputs, product public inputs) of program `name` run for at most n cycles."""
    from zkir_amd import pipeline as pl
    mk, cfg = PROGRAMS[name]
    blob = mk().to_bytes()
    kw = dict(max_cycles=n) if n else {}
    log = rt.interpret(blob, [], rt.VMConfig(enable_execution_trace=True, **kw, **cfg))
    ddl = pl.upload(log)
    tr = pl.DeviceTrace(ddl)
    pl.trace_fill(pl.trace_fill_args(ddl, tr))
    res = oracle.run(blob, enable_execution_trace=True, **kw, **cfg)
    deferred = bool(cfg.get("enable_deferred_model"))
    opub = so.public_inputs(len(res.rows), blob, [], list(res.outputs), (res.halt_kind, res.halt_code), deferred=deferred)
    return blob, log, tr, res.rows, opub, rt.public_inputs(log, blob, [], deferred)


@pytest.mark.parametrize("name,n", [("fib", 64), ("fib", 1024), ("fib", 4096), ("fib", 1000), ("fib", 5), ("sha", 512), ("sha", 700), ("deferred", 256),
                                    ("fib30", None), ("exit42", None), ("cmp", 600), ("cmp", 5000), ("cmp_deferred", 300), ("call", 500), ("call", 3000),
                                    ("call_deferred", 250), ("sgn", 700), ("sgn", 5000), ("sgn_deferred", 300), ("cmov", 400), ("cmov", 3000), ("cmov_deferred", 300)])
def test_main_trace_and_commit_match_oracle(name, n):
    """All committed columns of the padded main trace (152 in default mode, 168 deferred: the oracle's 172 logical columns minus the ones
    that are identically zero), the LDE and the commitment root, for power-of-two and ragged row counts and for programs that halt on
    their own (Exit / padding rows)."""
    from zkir_amd import stark
    blob, log, tr, rows, opub, pub = _case(name, n)
    assert pub.n_real == len(rows) == opub.n_real
    deferred = bool(opub.deferred)
    wm = stark.main_width(deferred)
    assert wm == so.committed_width(deferred) == rt.lib().zkir_main_trace_width_for(int(deferred)) and stark.W_MAIN == rt.lib().zkir_main_trace_width()
    want_m = so.to_committed(so.main_trace(rows, opub), deferred)
    got_m = stark.from_b8(stark.main_trace(tr, deferred=deferred), wm).cpu().numpy().view(np.uint32)
    assert got_m.shape == want_m.shape
    for k in range(want_m.shape[0]):
        assert np.array_equal(got_m[k], want_m[k]), f"main-trace column {k}"
    ctx = stark.StarkContext(stark.padded_log_n(len(rows)))
    root, L, tree = stark.commit_trace(ctx, tr, deferred=bool(opub.deferred))
    want_root, want_L = so.commit_trace(rows, 1, want_lde=True, pub=opub)
    assert np.array_equal(stark.from_b8(L, wm).cpu().numpy().view(np.uint32), want_L)
    assert np.array_equal(root, want_root)
    ctx.close(); log.close()


def test_commit_2p16_root_and_properties():
    """A larger size (oracle still finishes in seconds): root equality + Merkle path of a random leaf recomputed with the oracle's hash."""
    from zkir_amd import stark
    log_n = 15
    n = 1 << log_n
    blob, log, tr, rows, opub, pub = _case("fib", n)
    ctx = stark.StarkContext(log_n)
    root, L, tree = stark.commit_trace(ctx, tr)
    assert np.array_equal(root, so.commit_trace(rows, 1, pub=opub))
    Lh = stark.from_b8(L, stark.W_MAIN).cpu().numpy().view(np.uint32)
    t = tree.cpu().numpy().view(np.uint32)
    j, off, mm = 54321, 0, 2 * n
    node = so.hash_elems(Lh[:, j])
    assert np.array_equal(node, t[4 * j:4 * j + 4])
    while mm > 1:
        sib = t[off + 4 * (j ^ 1): off + 4 * (j ^ 1) + 4]
        node = so.compress(node, sib) if j % 2 == 0 else so.compress(sib, node)
        off += 4 * mm; mm //= 2; j //= 2
    assert np.array_equal(node, root)
    ctx.close(); log.close()


@pytest.mark.parametrize("name,n", [("fib", 8), ("fib", 5), ("fib", 32), ("fib", 256), ("fib", 2048), ("fib", 1500), ("sha", 512), ("sha", 300), ("deferred", 1024),
                                    ("fib30", None), ("exit42", None), ("fib", 8192), ("cmp", 600), ("cmp", 4096), ("cmp_deferred", 300), ("call", 500),
                                    ("call", 2048), ("call_deferred", 250), ("sgn", 700), ("sgn", 4096), ("sgn_deferred", 300), ("cmov", 400), ("cmov", 2048), ("cmov_deferred", 300)])
def test_proof_bytes_match_oracle_and_verify(name, n):
    """End-to-end proof (quotient over the v1 AIR, openings, DEEP, FRI, grinding, queries): GPU proof words == oracle proof words,
    and both verifiers accept them.  The GPU evaluates openings barycentrically on the LDE coset, the oracle by Horner on
    coefficients; the GPU's constraint list is air.h, the oracle's its own."""
    from zkir_amd import stark
    blob, log, tr, rows, opub, pub = _case(name, n)
    ctx = stark.StarkContext(stark.padded_log_n(len(rows)))
    proof, ms = stark.prove(ctx, tr, pub, want_stage_ms=True)
    assert so.verify(proof, opub) == 0 and rt.verify(proof, pub) == 0
    want = so.prove(rows, opub)
    assert len(proof) == len(want)
    if not np.array_equal(proof, want):
        bad = np.nonzero(proof != want)[0]
        raise AssertionError(f"proof differs at word {bad[0]} of {len(want)} ({len(bad)} words differ)")
    # tampering is rejected
    for pos in (8, 30, len(proof) // 2, len(proof) - 1):
        t = proof.copy()
        t[pos] = (int(t[pos]) + 1) % P
        assert so.verify(t) != 0 and rt.verify(t) == so.verify(t)
    assert np.array_equal(stark.prove(ctx, tr, pub), proof)                                 # deterministic
    ctx.close(); log.close()


@pytest.mark.parametrize("n", [16, 64, 128])
def test_proof_bytes_match_oracle_at_the_smallest_fri_schedules(n):
    """zkir_prove runs the commitment layer's FRI at b = 1.  With test_proof_bytes_match_oracle_and_verify's fib at 8 and 32 rows, these sizes give every short schedule:
    log_n = 3 .. 7 -> [1], [1, 1], [1, 2], [1, 3], [1, 3, 1] — a single layer, each fri_fold_k_kernel<K>, a short last layer.  Mode 0, word for word, accepted."""
    from zkir_amd import stark
    blob, log, tr, rows, opub, pub = _case("fib", n)
    assert len(rows) == n
    ctx = stark.StarkContext(stark.padded_log_n(n))
    proof = stark.prove(ctx, tr, pub)
    assert np.array_equal(proof, so.prove(rows, opub))
    assert rt.verify(proof, pub) == 0
    ctx.close(); log.close()


def test_wrong_execution_is_rejected_on_the_gpu_path():
    """The GPU prover on a device trace whose values do not follow the program (patched in HBM): the proof it emits is rejected by
    both verifiers at the constraint check — a wrong ADD result, a wrong branch target."""
    import torch
    from zkir_amd import stark
    blob, log, tr, rows, opub, pub = _case("fib", 256)
    ctx = stark.StarkContext(8)
    ops = rows["instruction"] & 0x7F
    k = int(np.nonzero(ops == 0x00)[0][5])
    nxt = k + 1 + int(np.nonzero(ops[k + 1:] == 0x00)[0][0])
    saved = tr.registers[4, k + 1:nxt + 1].clone()
    tr.registers[4, k + 1:nxt + 1] += 1                                                     # the ADD's result, consistently off by one until r4 is rewritten
    bad = stark.prove(ctx, tr, pub)
    assert so.verify(bad, opub) == 10 and rt.verify(bad, pub) == 10
    tr.registers[4, k + 1:nxt + 1] = saved
    # AIR v3: the comparison families, on a run of spec.compare_loop_program — an SLTU written the wrong way round, a SUB off by one
    blob3, log3, tr3, rows3, opub3, pub3 = _case("cmp", 600)
    ctx3 = stark.StarkContext(10)
    ops3 = rows3["instruction"] & 0x7F
    for op, rd, edit in ((0x20, 6, lambda v: v ^ 1), (0x01, 4, lambda v: v + 1)):
        ks = np.nonzero((ops3 == op) & (((rows3["instruction"] >> 7) & 0xF) == rd))[0]
        k3, nx3 = int(ks[4]), int(ks[5])
        saved3 = tr3.registers[rd, k3 + 1:nx3 + 1].clone()
        tr3.registers[rd, k3 + 1:nx3 + 1] = edit(saved3)
        bad3 = stark.prove(ctx3, tr3, pub3)
        assert so.verify(bad3, opub3) == 10 and rt.verify(bad3, pub3) == 10, hex(op)
        tr3.registers[rd, k3 + 1:nx3 + 1] = saved3
    assert np.array_equal(stark.prove(ctx3, tr3, pub3), so.prove(rows3, opub3))
    ctx3.close(); log3.close()
    # AIR v4: a JALR's link off by 4, a register written "by" a signed branch — on a run of spec.call_loop_program
    blob4, log4, tr4, rows4, opub4, pub4 = _case("call", 500)
    ctx4 = stark.StarkContext(9)
    ops4 = rows4["instruction"] & 0x7F
    kj = int(np.nonzero((ops4 == 0x49) & (((rows4["instruction"] >> 7) & 0xF) == 13))[0][0]); kb = int(np.nonzero(ops4 == 0x42)[0][3])
    for reg, lo, edit in ((13, kj + 1, lambda v: v + 4), (9, kb + 1, lambda v: v + 7)):
        saved4 = tr4.registers[reg, lo:len(rows4)].clone()
        tr4.registers[reg, lo:len(rows4)] = edit(saved4)
        bad4 = stark.prove(ctx4, tr4, pub4)
        assert so.verify(bad4, opub4) == 10 and rt.verify(bad4, pub4) == 10, reg
        tr4.registers[reg, lo:len(rows4)] = saved4
    assert np.array_equal(stark.prove(ctx4, tr4, pub4), so.prove(rows4, opub4))
    ctx4.close(); log4.close()
    # AIR v5: a signed comparison written the wrong way round, a register that follows a signed branch going the other way — on a run of
    # spec.signed_loop_program (the r4 += 16 after "blt r1, r0" executed although the branch was taken)
    blob5, log5, tr5, rows5, opub5, pub5 = _case("sgn", 700)
    ctx5 = stark.StarkContext(10)
    ops5 = rows5["instruction"] & 0x7F
    ks5 = np.nonzero((ops5 == 0x22) & (((rows5["instruction"] >> 7) & 0xF) == 4))[0]
    k5 = int(ks5[3])
    nx5 = k5 + 1 + int(np.nonzero(((rows5["instruction"][k5 + 1:] >> 7) & 0xF) == 4)[0][0])
    saved5 = tr5.registers[4, k5 + 1:nx5 + 1].clone()
    tr5.registers[4, k5 + 1:nx5 + 1] = saved5 ^ 1
    bad5 = stark.prove(ctx5, tr5, pub5)
    assert so.verify(bad5, opub5) == 10 and rt.verify(bad5, pub5) == 10
    tr5.registers[4, k5 + 1:nx5 + 1] = saved5
    assert np.array_equal(stark.prove(ctx5, tr5, pub5), so.prove(rows5, opub5))
    ctx5.close(); log5.close()
    # A row whose (pc, instruction word) is not in the program's code table has NO proof in AIR v2 (instruction-ROM lookup): the honest
    # prover refuses it instead of emitting a proof the verifier would reject — a BNE's fall-through claimed where the run branched
    # (the word at the claimed pc is another one), an instruction word patched in HBM (ADD -> SUB: the forgery AIR v1 accepted)
    kb = int(np.nonzero(ops == 0x41)[0][3])
    saved_pc = tr.pc[kb + 1].clone()
    tr.pc[kb + 1] = tr.pc[kb] + 4
    with pytest.raises(rt.RuntimeError) as e:
        stark.prove(ctx, tr, pub)
    assert e.value.code == rt.ERR_ARGUMENT and f"row {kb + 1} " in e.value.message and "code table" in e.value.message
    tr.pc[kb + 1] = saved_pc
    saved_w = tr.instruction[k].clone()
    tr.instruction[k] = (int(saved_w) & ~0x7F) | 0x01
    with pytest.raises(rt.RuntimeError) as e:
        stark.prove(ctx, tr, pub)
    assert e.value.code == rt.ERR_ARGUMENT and f"row {k} " in e.value.message
    tr.instruction[k] = saved_w
    # ... and so has a run of a program that rewrites its own code: the executed word is not the program's
    from zkir_amd import pipeline as pl
    import programs
    sm_blob, sm_in, sm_cfg = programs.ALL["self_modifying"]()
    sm_log = rt.interpret(sm_blob, sm_in, rt.VMConfig(enable_execution_trace=True, **sm_cfg))
    sm_ddl = pl.upload(sm_log); sm_tr = pl.DeviceTrace(sm_ddl); pl.trace_fill(pl.trace_fill_args(sm_ddl, sm_tr))
    sm_ctx = stark.StarkContext(stark.padded_log_n(sm_log.n_rows))
    with pytest.raises(rt.RuntimeError) as e:
        stark.prove(sm_ctx, sm_tr, rt.public_inputs(sm_log, sm_blob, sm_in))
    assert "code table" in e.value.message
    sm_ctx.close(); sm_log.close()
    good = stark.prove(ctx, tr, pub)
    assert rt.verify(good, pub) == 0 and np.array_equal(good, so.prove(rows, opub))
    ctx.close(); log.close()


def test_two_contexts_prove_concurrently():
    """No process-wide prover state: two threads, two contexts, two streams, different runs — proofs identical to the sequential ones."""
    import threading
    import torch
    from zkir_amd import stark
    cases = [_case("fib", 4096), _case("sha", 3000)]
    ctxs = [stark.StarkContext(12), stark.StarkContext(12)]
    want = [stark.prove(c, cs[2], cs[5]) for c, cs in zip(ctxs, cases)]
    got = [[None] * 6 for _ in cases]
    errs = []

    def work(i):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            for r in range(6):
                with torch.cuda.stream(s):
                    got[i][r] = stark.prove(ctxs[i], cases[i][2], cases[i][5], stream=s)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    torch.cuda.synchronize()
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        for r in range(6):
            assert np.array_equal(got[i][r], want[i]), (i, r)
        assert rt.verify(want[i], cases[i][5]) == 0
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("G", [2, 4, 8])
def test_row_sharded_commitment_matches_oracle(G):
    """BASELINE configs[3] shape on one device: each row shard is filled and committed on its own (own register snapshot, own
    LDE + Merkle subtree); the shard roots are the leaves of the top log2(G) levels (zkir_merkle_cap_launch).  G = 8: the three-level cap of the 8-GPU run
    (VERDICT r4 weak #2).  Oracle: same thing on the CPU."""
    import torch
    from zkir_amd import pipeline as pl, stark
    log_n = 9
    n = 1 << log_n
    blob = spec.sha256_chain_program().to_bytes()
    log = rt.interpret(blob, config=rt.VMConfig(max_cycles=n * G, enable_execution_trace=True), tile_rows=256)
    rows = oracle.run(blob, max_cycles=n * G, enable_execution_trace=True).rows
    ctx = stark.StarkContext(log_n)
    roots, want_roots = [], []
    for g in range(G):
        sh = log.shard(g * n, (g + 1) * n)
        ddl = pl.upload(sh)
        tr = pl.DeviceTrace(ddl)
        pl.trace_fill(pl.trace_fill_args(ddl, tr))
        root, _, tree = stark.commit_trace(ctx, tr)
        roots.append(tree[-4:].clone())
        want_roots.append(so.commit_trace(rows[g * n:(g + 1) * n], 1))
        assert np.array_equal(root, want_roots[-1]), f"shard {g}"
        sh.close()
    top = stark.merkle_cap(ctx, torch.stack(roots)).cpu().numpy().view(np.uint32)
    level = list(want_roots)
    while len(level) > 1:
        level = [so.compress(level[i], level[i + 1]) for i in range(0, len(level), 2)]
    assert np.array_equal(top, level[0])
    ctx.close(); log.close()


@pytest.mark.parametrize("log_n", [16, 18])
def test_proof_large_verifies(log_n):
    """Larger than the oracle prover comfortably handles: both VERIFIERS (cheap) accept the GPU proof.  2^18 rows is the
    smallest size whose FRI schedule has an 8-to-1 layer hashed by the one-permutation-per-lane kernel (> 2^14 leaves), and whose
    Merkle trees use the per-level kernel, both subtree modes and the quad-lane permutation.  One row short of the power of two:
    the last row is padding."""
    from zkir_amd import stark
    blob, log, tr, rows, opub, pub = _case("fib", (1 << log_n) - 1)
    ctx = stark.StarkContext(log_n)
    proof = stark.prove(ctx, tr, pub)
    assert so.verify(proof, opub) == 0 and rt.verify(proof, pub) == 0
    assert proof[2] == log_n and proof[3] == 152 and proof[7] == (1 << log_n) - 1
    ctx.close(); log.close()


def _fpow(a, e):
    """Vectorised a^e mod p on uint64 arrays (products of two 31-bit values fit 62 bits)."""
    a = a.astype(np.uint64) % np.uint64(P)
    r = np.ones_like(a)
    while e:
        if e & 1:
            r = r * a % np.uint64(P)
        a = a * a % np.uint64(P)
        e >>= 1
    return r


def _bary_eval(values, log_size, shift, z):
    """f(z) for the polynomial of degree < 2^log_size with f(shift * w^j) = values[j], base-field z outside the domain:
    f(z) = ((z/shift)^n - 1)/n * sum_j values[j] * x_j / (z - x_j)."""
    n = 1 << log_size
    w = pow(31, (P - 1) >> log_size, P)                           # primitive 2^log_size-th root: 31 generates F_p^*, p - 1 = 15 * 2^27
    x = np.empty(n, dtype=np.uint64)                              # x_j = shift * w^j by doubling
    x[0] = shift
    filled, wp = 1, w
    while filled < n:
        x[filled:2 * filled] = x[:filled] * np.uint64(wp) % np.uint64(P)
        wp = wp * wp % P
        filled *= 2
    d = (np.uint64(z) + np.uint64(P) - x) % np.uint64(P)
    terms = values.astype(np.uint64) * (x * _fpow(d, P - 2) % np.uint64(P)) % np.uint64(P)
    s = int(terms.sum(dtype=np.uint64)) % P                       # at most 2^21 terms below 2^31
    zs = z * pow(shift, P - 2, P) % P
    return (pow(zs, n, P) - 1) * pow(n, P - 2, P) % P * s % P


def test_full_size_2p20_properties():
    """BASELINE configs[1] size (2^20 rows), where the oracle's O(N log N) scalar code takes minutes: size-independent properties.
    * LDE: the column interpolant evaluated at a random point from the N trace values on H equals the one evaluated from the
      2N LDE values on the coset g<w_2N> (both by the barycentric formula, numpy on the host);
    * Merkle: random leaves re-hashed with the oracle's sponge and walked up their paths with the oracle's compression reach the root;
    * proof: both verifiers accept the GPU proof."""
    from zkir_amd import pipeline as pl, stark
    log_n = 20
    n = 1 << log_n
    blob = spec.fib_endless_program().to_bytes()
    log = rt.interpret(blob, [], rt.VMConfig(max_cycles=n, enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    pub = rt.public_inputs(log, blob)
    ctx = stark.StarkContext(log_n)
    m = stark.from_b8(stark.main_trace(tr), stark.W_MAIN).cpu().numpy().view(np.uint32)
    root, L, tree = stark.commit_trace(ctx, tr)
    Lh, t = stark.from_b8(L, stark.W_MAIN).cpu().numpy().view(np.uint32), tree.cpu().numpy().view(np.uint32)
    rng = np.random.default_rng(20)
    for col in (0, 1, 9, 18, 57, 105, 111):                         # committed columns: cycle, pc limb, r1 limb, r4 limb, a write selector, y limb, a class flag
        z = int(rng.integers(2, P))
        assert _bary_eval(m[col], log_n, 1, z) == _bary_eval(Lh[col], log_n + 1, 31, z), col
    for j in rng.integers(0, 2 * n, 6):
        j = int(j)
        node, off, mm = so.hash_elems(Lh[:, j]), 0, 2 * n
        assert np.array_equal(node, t[4 * j:4 * j + 4])
        while mm > 1:
            sib = t[off + 4 * (j ^ 1): off + 4 * (j ^ 1) + 4]
            node = so.compress(node, sib) if j % 2 == 0 else so.compress(sib, node)
            off += 4 * mm; mm //= 2; j //= 2
        assert np.array_equal(node, root)
    del L, tree, Lh, t
    proof = stark.prove(ctx, tr, pub)
    assert rt.verify(proof, pub) == 0 and so.verify(proof) == 0
    assert stark.trace_root(proof) == [int(x) for x in root]
    ctx.close(); log.close()


@pytest.mark.parametrize("name,n_total,seg", [("fib", 1000, 300), ("sha", 700, 256), ("fib", 4096, 1025), ("deferred", 500, 200)])
def test_a_run_proven_in_segments_on_the_gpu(name, n_total, seg):
    """Multi-GPU proving, executed here shard after shard on one device: every row shard of the delta log (plus the first row of the
    next one) goes through K1 and zkir_prove on its own; each segment proof is the oracle's word for word, and the chain verifies as
    ONE run in both verifiers.  Nothing but 16-byte-aligned row ranges of the host log is shared between the segments."""
    from zkir_amd import pipeline as pl, stark
    mk, cfg = PROGRAMS[name]
    blob = mk().to_bytes()
    deferred = bool(cfg.get("enable_deferred_model"))
    log = rt.interpret(blob, [], rt.VMConfig(enable_execution_trace=True, max_cycles=n_total, **cfg))
    res = oracle.run(blob, enable_execution_trace=True, max_cycles=n_total, **cfg)
    run_pub = rt.public_inputs(log, blob, [], deferred)
    run_opub = so.public_inputs(len(res.rows), blob, [], list(res.outputs), (res.halt_kind, res.halt_code), deferred=deferred)
    cuts, a = [], 0
    while a < log.n_rows - 1:
        b = min(a + seg, log.n_rows)
        cuts.append((a, b)); a = b - 1
    proofs = []
    for a, b in cuts:
        sh = log.shard(a, b)
        ddl = pl.upload(sh); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
        pub = rt.PublicInputsC.from_buffer_copy(run_pub); pub.n_real = b - a
        ctx = stark.StarkContext(stark.padded_log_n(b - a))
        proof = stark.prove(ctx, tr, pub)
        ctx.close(); sh.close()
        opub = so.PublicC.from_buffer_copy(run_opub); opub.n_real = b - a
        want = so.prove(res.rows[a:b], opub)
        assert np.array_equal(proof, want), f"segment rows [{a}, {b})"
        proofs.append(proof)
    assert len(proofs) >= 3
    assert rt.verify_chain(proofs, run_pub) == 0 and so.verify_chain(proofs, run_opub) == 0
    assert rt.verify(proofs[1]) == 7 and rt.verify_chain(proofs[1:]) == 41 and rt.verify_chain([proofs[0]] + proofs[2:]) == 42
    log.close()


# ---- MODE 2 (round 4): the default VM mode with the I/O argument -----------------------------------------------------------------------------------------
def _io_program():
    """READ, READ, WRITE their 40-bit sum, READ on the exhausted tape, WRITE that 0, EXIT(3) (syscall.rs:101-121)."""
    code = [spec.addi(10, 0, 1), spec.ecall(), spec.addi(5, 10, 0), spec.addi(10, 0, 1), spec.ecall(), spec.add(6, 5, 10), spec.addi(11, 6, 0), spec.addi(10, 0, 2), spec.ecall(),
            spec.addi(10, 0, 1), spec.ecall(), spec.addi(11, 10, 0), spec.addi(10, 0, 2), spec.ecall(), spec.addi(10, 0, 0), spec.addi(11, 0, 3), spec.ecall()]
    return spec.Program.from_code(code).to_bytes(), [1000, (1 << 45) + 77]


def _mode2_case(which):
    from zkir_amd import pipeline as pl
    if which == "io":
        blob, ins = _io_program(); n = None
    elif which == "fib30":
        blob, ins, n = spec.fib_program(30).to_bytes(), [], None
    elif which == "sha":
        blob, ins, n = spec.sha256_chain_program().to_bytes(), [], 700
    else:                                                                   # a long loop that WRITEs every iteration and exits: 400 outputs
        code = [spec.addi(1, 0, 0), spec.addi(3, 0, 400), spec.addi(1, 1, 3), spec.addi(11, 1, 0), spec.addi(10, 0, 2), spec.ecall(), spec.addi(3, 3, -1), spec.bne(3, 0, -20),
                spec.addi(10, 0, 0), spec.addi(11, 0, 7), spec.ecall()]
        blob, ins, n = spec.Program.from_code(code).to_bytes(), [], None
    cfg = dict(max_cycles=n) if n else {}
    ores = oracle.run(blob, ins, enable_execution_trace=True, **cfg)
    log = rt.interpret(blob, ins, rt.VMConfig(enable_execution_trace=True, **cfg))
    assert log.n_rows == len(ores.rows)
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    opub = so.public_inputs(len(ores.rows), blob, ins, list(ores.outputs), (ores.halt_kind, ores.halt_code), io_mode=True)
    pub = rt.public_inputs(log, blob, ins, io_mode=True)
    assert pub.deferred == 2 and list(pub.io_digest) == list(opub.io)
    return blob, ins, ores, log, tr, opub, pub


@pytest.mark.parametrize("which", ["io", "fib30", "sha", "writes"])
def test_mode2_proof_bytes_match_oracle_and_verify(which):
    """A proof in mode 2 — ECALL rows dispatched on R10, WRITE / READ rows tied to the tapes the proof carries — from the GPU prover equals the oracle's word for word;
    both verifiers accept it (their zkir_verify now also checks the io digest against the carried tapes and the halt row), zkir_verify_io agrees with the claim."""
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = _mode2_case(which)
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)))
    proof = stark.prove(ctx, tr, pub)
    want = so.prove(ores.rows, opub)
    assert proof[3] == 160 and proof[9] == 2 and len(proof) == len(want)
    if not np.array_equal(proof, want):
        bad = np.nonzero(proof != want)[0]
        raise AssertionError(f"mode-2 proof differs at word {bad[0]} of {len(want)} ({len(bad)} words differ)")
    assert so.verify(proof, opub) == 0 and rt.verify(proof, pub) == 0 and rt.verify(proof) == 0
    assert rt.verify_io(proof, pub, ins, list(ores.outputs), (ores.halt_kind, ores.halt_code)) == 0
    for pos in (8, 30, 158, 160, len(proof) // 2, len(proof) - 1):
        t = proof.copy()
        t[pos] = (int(t[pos]) + 1) % P
        assert so.verify(t) != 0 and rt.verify(t) == so.verify(t), pos
    ctx.close(); log.close()


def test_mode2_forged_outputs_are_rejected_on_the_gpu_path():
    """The GPU prover given public inputs that CLAIM other outputs than the trace writes (digest recomputed for the claim): the table side of the tape lookup is formed from the
    claim, the row side from the trace — the proof it emits fails the constraint check in both verifiers (10); a claim with too few / too many outputs is refused by
    the prover or fails the counters' check (51)."""
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = _mode2_case("fib30")
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)))
    assert list(ores.outputs) == [832040]
    fake = so.public_inputs(len(ores.rows), blob, ins, [832041], (ores.halt_kind, ores.halt_code), io_mode=True)
    fpub = pub.copy(); fpub.with_io(ins, [832041]); fpub.io_digest[:] = list(fake.io)
    proof = stark.prove(ctx, tr, fpub)
    assert so.verify(proof, fake) == rt.verify(proof, fpub) == 10
    assert np.array_equal(proof, so.prove(ores.rows, fake))                    # the same (worthless) proof the oracle's prover makes of that claim
    # the honest claim still verifies, and mode 0 of the same run is what it was (no I/O statement)
    assert rt.verify(stark.prove(ctx, tr, pub), pub) == 0
    pub0 = rt.public_inputs(log, blob, ins)
    assert pub0.deferred == 0 and rt.verify(stark.prove(ctx, tr, pub0), pub0) == 0
    ctx.close(); log.close()


# ---- MODE 3 (round 4): mode 2 + the memory argument ------------------------------------------------------------------------------------------------------------
def _mode3_case(which, witness="device", wide=False):
    from zkir_amd import pipeline as pl
    import programs as pg
    cfg = {}
    if which.startswith("random"):
        blob, ins = pg.random_program(int(which[6:]), hashes=False)
    elif which == "signed_division_loop":                                 # (mode 4) both routes of the wide class: sign-extended bytes (the tape) and small ones (the chunk relation)
        blob, ins, cfg = spec.signed_division_loop_program().to_bytes(), [], dict(max_cycles=3000)
    elif which == "memloop":                                              # a loop that walks an array: store i * 3 at A + 8 i, load it back as bytes / halfwords / words, sum, WRITE the sum
        blob, ins = spec.memory_loop_program(200).to_bytes(), []
    elif which.endswith("_on_code"):                                      # the reference's test as written: its data at 0x1000, the first code word
        blob, ins, cfg = getattr(pg, which[:-8])()
    else:
        blob, ins, cfg = pg.off_code(which)                               # (timestamps: the data moved off the code segment — format v11, check 55)
        cfg = {k: v for k, v in cfg.items() if k == "max_cycles"}
    ores = oracle.run(blob, list(ins), enable_execution_trace=True, **cfg)
    log = rt.interpret(blob, list(ins), rt.VMConfig(enable_execution_trace=True, **cfg))
    assert log.n_rows == len(ores.rows)
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    opub = so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code), mem_mode=not wide, wide_mode=wide)
    pub = rt.public_inputs(log, blob, list(ins), mem_mode=not wide, wide_mode=wide, mem_witness=witness)
    assert pub.deferred == (4 if wide else 3) and list(pub.io_digest) == list(opub.io)
    return blob, list(ins), ores, log, tr, opub, pub


@pytest.mark.parametrize("witness", ["device", "host"])
@pytest.mark.parametrize("which", ["timestamps", "loads_stores", "alu_all", "mul_grid", "echo5", "fib30", "random3", "random5", "memloop", "mem_sw_lw", "rc_doubling"])
def test_mode3_proof_bytes_match_oracle_and_verify(which, witness):
    """A proof in mode 3 — loads and stores constrained, every access one step of the offline memory check, the touched cells carried — from the GPU prover equals the
    oracle's word for word; both verifiers accept it and give the same verdict on tampered copies.  The memory witness comes from the device (memcheck.hip: address-major
    sort + segmented scan) or from the host's sequential replay: the same proof either way."""
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = _mode3_case(which, witness)
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)))
    proof = stark.prove(ctx, tr, pub)
    want = so.prove(ores.rows, opub)
    assert proof[3] == 264 and proof[9] == 3 and len(proof) == len(want)
    if not np.array_equal(proof, want):
        bad = np.nonzero(proof != want)[0]
        raise AssertionError(f"mode-3 proof differs at word {bad[0]} of {len(want)} ({len(bad)} words differ)")
    assert so.verify(proof, opub) == 0 and rt.verify(proof, pub) == 0 and rt.verify(proof) == 0
    assert rt.verify_io(proof, pub, ins, list(ores.outputs), (ores.halt_kind, ores.halt_code)) == 0
    for pos in (8, 30, 158, 160, len(proof) // 2, len(proof) - 1):
        t = proof.copy()
        t[pos] = (int(t[pos]) + 1) % P
        assert so.verify(t) != 0 and rt.verify(t) == so.verify(t), pos
    ctx.close(); log.close()


# ---- MODE 4 (round 6): mode 3 + MULH / DIVU / REMU / DIV / REM (chunk relation below 2^40, the wide tape above), hash syscalls as a tape, the boundary cell -----------------------------------------------------------------------
@pytest.mark.parametrize("witness", ["device", "host"])
@pytest.mark.parametrize("which", ["wide_grid", "alu_all", "timestamps", "mul_grid", "random3", "random5", "memloop", "fib30", "sha_chain_small", "sha256_hello", "hashes_all",
                                   "blake3_multi_chunk", "loads_stores", "signed_division_loop"])
def test_mode4_proof_bytes_match_oracle_and_verify(which, witness):
    """A proof in mode 4 (format v12: 288 + 128 columns, 712 constraints) — the five wide opcodes constrained as F1 F2 + ADD = LO + 2^40 HI over 10-bit chunks, hash syscalls as
    a tape whose digests the verifier computes (configs[4]'s SHA-256 chain, the reference's SHA-256 / Keccak-256 / BLAKE3 tests: proven from the host witness — a "device"
    request is switched over), the boundary cell (the chain program reads its seed from it), everything of mode 3 beside them — from the GPU prover equals the oracle's word
    for word; both verifiers accept it and give the same verdict on tampered copies."""
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = _mode3_case(which, witness, wide=True)
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)))
    proof = stark.prove(ctx, tr, pub)
    want = so.prove(ores.rows, opub)
    assert proof[1] == 12 and proof[3] == 288 and proof[9] == 4 and len(proof) == len(want)
    if not np.array_equal(proof, want):
        bad = np.nonzero(proof != want)[0]
        raise AssertionError(f"mode-4 proof differs at word {bad[0]} of {len(want)} ({len(bad)} words differ)")
    assert so.verify(proof, opub) == 0 and rt.verify(proof, pub) == 0 and rt.verify(proof) == 0
    assert rt.verify_io(proof, pub, ins, list(ores.outputs), (ores.halt_kind, ores.halt_code)) == 0
    for pos in (8, 30, 158, 160, len(proof) // 2, len(proof) - 1):
        t = proof.copy()
        t[pos] = (int(t[pos]) + 1) % P
        assert so.verify(t) != 0 and rt.verify(t) == so.verify(t), pos
    ctx.close(); log.close()


@pytest.mark.parametrize("which", ["wide_grid", "loads_stores", "random3", "signed_division_loop", "sha256_hello"])
def test_mode4_device_main_trace_equals_the_oracles(which):
    """main_trace_kernel<4> + wide_tape_fix_kernel against the oracle's main trace, every committed column of every row.  The row kernel sits at 256 registers with spilled
    SGPRs; in round 6 a variant of it with 64-bit division inlined read four registers from wrong addresses on gfx950 — the proofs differed, but this comparison names the column."""
    import ctypes as C
    import torch
    blob, ins, ores, log, tr, opub, pub = _mode3_case(which, "host", wide=True)
    nr = len(ores.rows)
    N = 1 << so.padded_log_n(nr); wm = so.committed_width(4)
    out = torch.zeros((wm // 8, N, 8), dtype=torch.int32, device="cuda")
    scratch = torch.zeros(2 * N + 2 * (N // 1024 + 2) + 64, dtype=torch.int32, device="cuda")
    tape = torch.tensor([int(x) - (1 << 64) if int(x) >> 63 else int(x) for x in ins] if len(ins) else [0], dtype=torch.int64, device="cuda")

    class IoArgs(C.Structure):
        _fields_ = [("inputs", C.c_void_p), ("n_inputs", C.c_uint64), ("writes_before", C.c_uint64), ("reads_before", C.c_uint64)]
    io = IoArgs(tape.data_ptr(), len(ins), 0, 0)
    mo = torch.from_numpy(np.ctypeslib.as_array(C.cast(pub.mem_old, C.POINTER(C.c_uint64)), (nr,)).astype(np.int64)).cuda()
    mt = torch.from_numpy(np.ctypeslib.as_array(C.cast(pub.mem_told, C.POINTER(C.c_uint32)), (nr,)).astype(np.int32)).cuda()
    L = rt.lib()
    L.zkir_main_trace_wide_launch.restype = C.c_int
    L.zkir_main_trace_wide_launch.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.zkir_main_trace_wide_launch(C.byref(tr.c), nr, C.byref(io), mo.data_ptr(), mt.data_ptr(), int.from_bytes(blob[16:20], "little"), scratch.data_ptr(), out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32).transpose(0, 2, 1).reshape(wm, N)
    want = so.to_committed(so.main_trace(ores.rows, opub), 4)
    for k in range(wm):
        assert np.array_equal(got[k], want[k]), f"committed column {k}: first difference at row {int(np.nonzero(got[k] != want[k])[0][0])}"
    log.close()


def test_mode4_wide_tape_raw_64_bit_operands():
    """The wide tape on the GPU: a run that divides and multiplies RAW 64-bit registers — a byte sign-extended by LB (0xFFFF...FF80), 64-bit inputs that arrive by READ, i64::MIN
    / -1 — has a mode-4 proof, equal to the oracle's word for word: the row builder marks the rows (ot), lookup_index_kernel appends their records, the host sorts them by
    cycle, computes the reference's results (air::wide_result) for the table side and scatters the helpers WW.  The tape the proof carries holds exactly those rows; a tampered
    record is rejected by both verifiers alike."""
    from zkir_amd import pipeline as pl, stark
    import programs as pg
    O, E = spec.Opcode, spec.encode
    vals = [0xFFFFFFFFFFFFFF80, 0x8000000000000000, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF, 0x0000010000000000, 0x123456789ABCDEF0, 0xFF, 3]
    regs = [1, 2, 3, 4, 9, 14, 15, 7]
    code = [pg.A(5, 0, 1)]
    for r in regs:
        code += [pg.A(10, 0, 1), pg.EC, E(O.CMOV, r, 10, 5)]                                       # READ leaves the raw 64 bits in r10; CMOV copies them
    body = [E(op, 8, regs[a], regs[b]) for a in range(8) for b in range(8) for op in (O.MULH, O.DIVU, O.REMU, O.DIV, O.REM)]
    blob = pg._p(code + body + [pg.EB])
    ores = oracle.run(blob, vals, enable_execution_trace=True)
    log = rt.interpret(blob, vals, rt.VMConfig(enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    opub = so.public_inputs(len(ores.rows), blob, vals, list(ores.outputs), (ores.halt_kind, ores.halt_code), wide_mode=True)
    pub = rt.public_inputs(log, blob, vals, wide_mode=True)
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)))
    proof = stark.prove(ctx, tr, pub)
    want = so.prove(ores.rows, opub)
    assert np.array_equal(proof, want)
    assert so.verify(proof, opub) == 0 and rt.verify(proof, pub) == 0
    lay = stark.proof_layout(proof)
    w0 = lay["wide_section"]
    n = int(proof[w0])
    assert n >= 5 * 60 and all(int(proof[w0 + 1 + 8 * k]) < int(proof[w0 + 1 + 8 * (k + 1)]) for k in range(n - 1))      # nearly the whole grid, in cycle order
    t = proof.copy(); t[w0 + 1 + 8 * (n // 2) + 2] ^= 1
    assert so.verify(t) != 0 and rt.verify(t) == so.verify(t)
    ctx.close(); log.close()


@pytest.mark.parametrize("witness", ["device", "host"])
@pytest.mark.parametrize("which", ["timestamps_on_code", "mem_sw_lw_on_code", "q9_access_at_own_pc"])
def test_mode3_refuses_accesses_to_the_code_segment(which, witness):
    """(format v11) Instruction fetch is tied to the program's words, so a store into the code segment would change what the VM executes (strict protection is off,
    vm.rs:175) but not what the AIR lets through: the GPU prover refuses a run whose touched cells overlap [0x1000, 0x1000 + code_size) — the reference's own memory tests as
    written (they store at 0x1000), the Q9 program (an access at its own pc) — and both verifiers reject the oracle's proof of it with check 55."""
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = _mode3_case(which, witness)
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)))
    with pytest.raises(rt.RuntimeError) as e:
        stark.prove(ctx, tr, pub)
    assert e.value.code == rt.ERR_ARGUMENT and "overlaps the code segment" in e.value.message
    want = so.prove(ores.rows, opub)
    assert so.verify(want, opub) == 55 and rt.verify(want) == 55
    ctx.close(); log.close()


def test_mode3_forged_memory_is_rejected_on_the_gpu_path():
    """The GPU prover fed a memory witness in which one load reads a STALE cell (the bytes and time of an earlier access): every row is locally consistent with its witness —
    the main trace kernel just builds what it is given — but the multiset equation does not close, and both verifiers reject the proof (10).  A forged final cell likewise."""
    import ctypes as C
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = _mode3_case("timestamps", "host")  # sw [A] <- 0x100; sw [A + 4] <- 0x200; lw A; lw A + 4: one cell, four accesses (rows 2, 4, 5, 6)
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)))
    assert rt.verify(stark.prove(ctx, tr, pub), pub) == 0
    with pytest.raises(Exception, match="hash syscall"):                       # the device witness refuses what the host replay refuses
        b2, i2, o2, l2, t2, op2, p2 = _mode3_case("sha256_hello")
        stark.prove(stark.StarkContext(stark.padded_log_n(len(o2.rows))), t2, p2)
    n = len(ores.rows)
    old = np.ctypeslib.as_array(C.cast(pub.mem_old, C.POINTER(C.c_uint64)), (n,)).copy()
    told = np.ctypeslib.as_array(C.cast(pub.mem_told, C.POINTER(C.c_uint32)), (n,)).copy()
    assert told[5] == 5 and old[5] == 0x0000020000000100
    old[5], told[5] = old[4], told[4]                                          # the first load sees the cell as the SECOND store found it (before 0x200 was written)
    f = pub.copy(); f._old, f._told = old, told
    f.mem_old, f.mem_told = old.ctypes.data, told.ctypes.data
    try:
        proof = stark.prove(ctx, tr, f)
    except Exception:
        proof = None                                                           # (the loaded register no longer matches the trace's next row: the prover may refuse the row outright)
    if proof is not None:
        assert so.verify(proof) != 0 and rt.verify(proof) != 0
    g = pub.copy()
    cb = np.ctypeslib.as_array(C.cast(pub.cell_bytes, C.POINTER(C.c_uint64)), (pub.n_cells,)).copy()
    cb[0] ^= 1
    g._cb = cb; g.cell_bytes = cb.ctypes.data
    proof = stark.prove(ctx, tr, g)
    assert so.verify(proof) == rt.verify(proof) == 10
    ctx.close(); log.close()


def test_mode3_at_scale():
    """2^18 rows of the array loop (4 of 13 rows are loads / stores, ~20 Ki cells): accepted by both verifiers; proving time reported."""
    import time
    from zkir_amd import pipeline as pl, stark
    blob = spec.memory_loop_program(1 << 15).to_bytes()
    log = rt.interpret(blob, [], rt.VMConfig(max_cycles=1 << 18, enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    t0 = time.perf_counter(); hpub = rt.public_inputs(log, blob, [], mem_mode=True, mem_witness="host"); t_wit = time.perf_counter() - t0
    pub = rt.public_inputs(log, blob, [], mem_mode=True)
    ctx = stark.StarkContext(stark.padded_log_n(log.n_rows))
    stark.prove(ctx, tr, pub)
    t0 = time.perf_counter(); proof = stark.prove(ctx, tr, pub); t_prove = time.perf_counter() - t0
    t0 = time.perf_counter(); hproof = stark.prove(ctx, tr, hpub); t_hprove = time.perf_counter() - t0
    print(f"mode 3, {log.n_rows} rows, {hpub.n_cells} cells: prove {t_prove * 1e3:.1f} ms with the memory witness made on the device; host replay {t_wit * 1e3:.1f} ms + prove {t_hprove * 1e3:.1f} ms; "
          f"proof {len(proof) * 4 / 1024:.0f} KiB")
    assert np.array_equal(proof, hproof)
    assert rt.verify(proof, pub) == 0 and so.verify(proof) == 0
    ctx.close(); log.close()


def test_mode3_prove_wall_time_is_the_stages():
    """A mode-3 proof's wall time is the sum of its device stages (+ host transcript work), call after call.  Round 4 measured 49 ms of wall for 25 ms of stages from the third
    call of a process on: the memory section (1.8 MB) crossed as a PAGEABLE copy, the runtime pinned it in place, and free() handing the block back to the kernel evicted the
    process's queues (host.h: HostPin; profiles/r04w_pageable_copy_stall.txt).  Every block of unbounded size now crosses through the context's pinned staging."""
    import time
    from zkir_amd import pipeline as pl, stark
    blob = spec.memory_loop_program(65535).to_bytes()
    log = rt.interpret(blob, [], rt.VMConfig(max_cycles=1 << 20, enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    pub = rt.public_inputs(log, blob, [], mem_mode=True)
    ctx = stark.StarkContext(stark.padded_log_n(log.n_rows))
    stark.prove(ctx, tr, pub)
    gaps = []
    for _ in range(6):
        t0 = time.perf_counter(); _, ms = stark.prove(ctx, tr, pub, want_stage_ms=True); wall = (time.perf_counter() - t0) * 1e3
        gaps.append(wall - float(sum(ms)))
    print("mode 3, 2^20 rows: wall - stages per call (ms):", [round(g, 2) for g in gaps])
    assert min(gaps[2:]) < 5.0, gaps                            # (the stall added 17-25 ms to EVERY call from the third on)
    ctx.close(); log.close()


@pytest.mark.parametrize("k,log2_cells", [(12, 4), (16, 13), (18, 13), (18, 10), (20, 13)])
def test_memcheck_witness_device_equals_host_replay(k, log2_cells):
    """zkir_memcheck_witness_device (memcheck.hip: the accesses sorted by (cell, row), a segmented scan per cell) against zkir_memcheck_witness_of (the host's sequential replay)
    on spec.memory_ring_program — every cell is RE-VISITED after 2^log2_cells iterations, so each cell's accesses are far apart in time and the sort has real work to do (sizes on
    both sides of rocPRIM's merge-sort / onesweep switch: sorting on the cell bits alone went wrong in between, scripts/dbg/sort_test.hip): old bytes and old time of every row,
    and the touched cells, entry for entry."""
    import ctypes as C
    import torch
    from zkir_amd import pipeline as pl
    n = 1 << k
    blob = spec.memory_ring_program(log2_cells).to_bytes()
    log = rt.interpret(blob, [], rt.VMConfig(max_cycles=n, enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr)); torch.cuda.synchronize()
    hw = rt.MemcheckWitness(log, blob)
    pub = rt.PublicInputsC(); pub.with_memory(hw)
    nc = hw.n_cells
    assert nc == min(1 << log2_cells, (n - 6) // 16 + 1)
    host = [np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), (m,)).copy() for p, t, m in
            ((pub.mem_old, C.c_uint64, n), (pub.mem_told, C.c_uint32, n), (pub.cell_addr, C.c_uint64, nc), (pub.cell_bytes, C.c_uint64, nc), (pub.cell_time, C.c_uint32, nc))]
    d_old, d_told = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    d_ca, d_cb, d_ct, dn = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint32), C.c_uint64(0)
    L = rt.lib()
    L.zkir_memcheck_witness_device.restype = C.c_int
    L.zkir_memcheck_witness_device.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t] + [C.c_void_p] * 5 + [C.c_uint64, C.c_void_p, C.c_void_p]
    assert L.zkir_memcheck_witness_device(C.byref(tr.c), n, blob, len(blob), d_old.ctypes.data, d_told.ctypes.data, d_ca.ctypes.data, d_cb.ctypes.data, d_ct.ctypes.data, n, C.byref(dn), None) == 0
    assert dn.value == nc
    for got, want, name in zip((d_old, d_told, d_ca[:nc], d_cb[:nc], d_ct[:nc]), host, ("old bytes", "old time", "cell address", "cell bytes", "cell time")):
        assert np.array_equal(got, want), f"{name}: first difference at {int(np.nonzero(got != want)[0][0])}"
    log.close()


def test_mode3_wrong_execution_is_rejected_on_the_gpu_path():
    """Mode 3 on a device trace whose values do not follow the program (patched in HBM, consistently until the register is rewritten): a load that returns another value than
    the cell holds, an XOR off by a bit, a shift off by a bit, a product off by one, an ANDI with the wrong immediate — each proof the GPU prover emits is rejected by both verifiers; in mode 0 the very
    same forged traces are ACCEPTED (those opcodes are class "other" there: y is a free witness) — the difference the mode makes."""
    from zkir_amd import stark
    blob = spec.memory_ring_program(4).to_bytes()
    n = 700
    ores = oracle.run(blob, [], max_cycles=n, enable_execution_trace=True)
    rows = ores.rows
    ops, rds = rows["instruction"] & 0x7F, (rows["instruction"] >> 7) & 0xF
    ctx = stark.StarkContext(stark.padded_log_n(n))

    def fresh():
        from zkir_amd import pipeline as pl
        log = rt.interpret(blob, [], rt.VMConfig(max_cycles=n, enable_execution_trace=True))
        ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
        return log, tr
    log, tr = fresh()
    pub3, pub0 = rt.public_inputs(log, blob, [], mem_mode=True), rt.public_inputs(log, blob, [])
    assert rt.verify(stark.prove(ctx, tr, pub3), pub3) == 0
    for op, rd, what in ((0x34, 8, "LW"), (0x12, 2, "XOR"), (0x13, 5, "ANDI"), (0x11, 12, "OR"), (0x33, 9, "LHU"), (0x30, 10, "LB")):
        ks = np.nonzero((ops == op) & (rds == rd))[0]
        k = int(ks[3])
        later = np.nonzero(rds[k + 1:] == rd)[0]                                            # rows until rd is written again
        hi = k + 1 + (int(later[0]) if len(later) else n - k - 2)
        saved = tr.registers[rd, k + 1:hi + 1].clone()
        tr.registers[rd, k + 1:hi + 1] = saved ^ 2
        bad3 = stark.prove(ctx, tr, pub3)
        assert rt.verify(bad3, pub3) != 0 and so.verify(bad3) != 0, what
        if op in (0x12, 0x11):                                                              # the forged register feeds only rows that are class "other" in mode 0: there the forged trace passes
            assert rt.verify(stark.prove(ctx, tr, pub0), pub0) == 0, what
        tr.registers[rd, k + 1:hi + 1] = saved
    assert rt.verify(stark.prove(ctx, tr, pub3), pub3) == 0
    ctx.close(); log.close()
    # the shifts and MUL, on tests/programs.py: alu_all
    import programs as pg
    blob2, ins2, _ = pg.alu_all()
    ores2 = oracle.run(blob2, list(ins2), enable_execution_trace=True)
    from zkir_amd import pipeline as pl
    log2 = rt.interpret(blob2, list(ins2), rt.VMConfig(enable_execution_trace=True))
    ddl2 = pl.upload(log2); tr2 = pl.DeviceTrace(ddl2); pl.trace_fill(pl.trace_fill_args(ddl2, tr2))
    pub2 = rt.public_inputs(log2, blob2, list(ins2), mem_mode=True)
    ctx2 = stark.StarkContext(stark.padded_log_n(len(ores2.rows)))
    assert rt.verify(stark.prove(ctx2, tr2, pub2), pub2) == 0
    ops2, rds2, n2 = ores2.rows["instruction"] & 0x7F, (ores2.rows["instruction"] >> 7) & 0xF, len(ores2.rows)
    for op in (0x18, 0x19, 0x1A, 0x1B, 0x1C, 0x1D, 0x02):                                  # .. and MUL
        ks = np.nonzero((ops2 == op) & (rds2 != 0))[0]
        k = int(ks[len(ks) // 2]); rd = int(rds2[k])
        later = np.nonzero(rds2[k + 1:] == rd)[0]
        hi = k + 1 + (int(later[0]) if len(later) else n2 - k - 2)
        saved = tr2.registers[rd, k + 1:hi + 1].clone()
        tr2.registers[rd, k + 1:hi + 1] = saved ^ 1
        bad = stark.prove(ctx2, tr2, pub2)
        assert rt.verify(bad, pub2) != 0 and so.verify(bad) != 0, hex(op)
        tr2.registers[rd, k + 1:hi + 1] = saved
    ctx2.close(); log2.close()


# ---- modes 3 / 4 at the address and hash-call edges (tests/test_memory_edges.py: the same programs against a Python model and the oracle on the CPU) -----------------------
_EDGE_CASES = [(n, m) for n in sorted(programs.MEM_EDGES) for m in (3, 4) if not (n == "edge_bc_alias_ok" and m == 3)] + [(n, 4) for n in sorted(programs.HASH_EDGES)]


def _edge_main_trace(which, mode):
    """The device main trace of an edge run (main_trace_kernel<3> / <4> + wide_tape_fix_kernel, host witness) and the oracle's, both as committed columns."""
    import ctypes as C
    import torch
    blob, ins, ores, log, tr, opub, pub = _mode3_case(which, "host", wide=mode == 4)
    nr = len(ores.rows)
    N = 1 << so.padded_log_n(nr); wm = so.committed_width(mode)
    out = torch.zeros((wm // 8, N, 8), dtype=torch.int32, device="cuda")
    scratch = torch.zeros(2 * N + 2 * (N // 1024 + 2) + 64, dtype=torch.int32, device="cuda")
    tape = torch.tensor([int(x) - (1 << 64) if int(x) >> 63 else int(x) for x in ins] if len(ins) else [0], dtype=torch.int64, device="cuda")

    class IoArgs(C.Structure):
        _fields_ = [("inputs", C.c_void_p), ("n_inputs", C.c_uint64), ("writes_before", C.c_uint64), ("reads_before", C.c_uint64)]
    io = IoArgs(tape.data_ptr(), len(ins), 0, 0)
    mo = torch.from_numpy(np.ctypeslib.as_array(C.cast(pub.mem_old, C.POINTER(C.c_uint64)), (nr,)).astype(np.int64)).cuda()
    mt = torch.from_numpy(np.ctypeslib.as_array(C.cast(pub.mem_told, C.POINTER(C.c_uint32)), (nr,)).astype(np.int32)).cuda()
    L = rt.lib()
    if mode == 4:
        L.zkir_main_trace_wide_launch.restype = C.c_int
        L.zkir_main_trace_wide_launch.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = L.zkir_main_trace_wide_launch(C.byref(tr.c), nr, C.byref(io), mo.data_ptr(), mt.data_ptr(), int.from_bytes(blob[16:20], "little"), scratch.data_ptr(), out.data_ptr(), None)
    else:
        L.zkir_main_trace_mem_launch.restype = C.c_int
        L.zkir_main_trace_mem_launch.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = L.zkir_main_trace_mem_launch(C.byref(tr.c), nr, C.byref(io), mo.data_ptr(), mt.data_ptr(), scratch.data_ptr(), out.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32).transpose(0, 2, 1).reshape(wm, N)
    want = so.to_committed(so.main_trace(ores.rows, opub), mode)
    log.close()
    return got, want


@pytest.mark.parametrize("which,mode", [c for c in _EDGE_CASES if c[0] != "hash_edge_max_len"])
def test_edge_device_main_trace_equals_the_oracles(which, mode):
    """Every committed column of every row at the address edges — limb-0 carries and borrows (c0, c1, C_CM2), limb 1 at 0xFFFFF / 0x80000 / 0x55555, the top cell, wrapped
    64-bit bases, cells 8 p apart, the boundary cell's neighbours and odd hash-output pointers: the failure names the column and the first row."""
    got, want = _edge_main_trace(which, mode)
    for k in range(len(want)):
        assert np.array_equal(got[k], want[k]), f"committed column {k}: first difference at row {int(np.nonzero(got[k] != want[k])[0][0])}"


@pytest.mark.parametrize("which", sorted(programs.MEM_EDGES))
def test_edge_memory_witness_device_equals_host_replay(which):
    """memcheck.hip (its sort key packs (ea >> 3) << 26: the top cell 2^40 - 8 is its largest key; cells 8 p apart must stay apart) against the host's replay: old bytes and old
    time of every row, the touched cells with their final bytes and times."""
    import ctypes as C
    import torch
    from zkir_amd import pipeline as pl
    blob, ins, cfg = programs.ALL[which]()
    log = rt.interpret(blob, ins, rt.VMConfig(enable_execution_trace=True))
    n = log.n_rows
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr)); torch.cuda.synchronize()
    hw = rt.MemcheckWitness(log, blob)
    pub = rt.PublicInputsC(); pub.with_memory(hw)
    nc = hw.n_cells
    host = [np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), (m,)).copy() for p, t, m in
            ((pub.mem_old, C.c_uint64, n), (pub.mem_told, C.c_uint32, n), (pub.cell_addr, C.c_uint64, nc), (pub.cell_bytes, C.c_uint64, nc), (pub.cell_time, C.c_uint32, nc))]
    d_old, d_told = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    d_ca, d_cb, d_ct, dn = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint32), C.c_uint64(0)
    L = rt.lib()
    L.zkir_memcheck_witness_device.restype = C.c_int
    L.zkir_memcheck_witness_device.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t] + [C.c_void_p] * 5 + [C.c_uint64, C.c_void_p, C.c_void_p]
    assert L.zkir_memcheck_witness_device(C.byref(tr.c), n, blob, len(blob), d_old.ctypes.data, d_told.ctypes.data, d_ca.ctypes.data, d_cb.ctypes.data, d_ct.ctypes.data, n, C.byref(dn), None) == 0
    assert dn.value == nc and nc >= 3
    for got, want, name in zip((d_old, d_told, d_ca[:nc], d_cb[:nc], d_ct[:nc]), host, ("old bytes", "old time", "cell address", "cell bytes", "cell time")):
        assert np.array_equal(got, want), f"{name}: first difference at {int(np.nonzero(got != want)[0][0])}"
    log.close()


@pytest.mark.parametrize("witness", ["device", "host"])
@pytest.mark.parametrize("which,mode", _EDGE_CASES)
def test_edge_proof_bytes_match_oracle_and_verify(which, mode, witness):
    """The whole proof at the edges, from either memory witness: equal to the oracle's word for word, accepted by both verifiers, tampered copies rejected alike."""
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = _mode3_case(which, witness, wide=mode == 4)
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)))
    proof = stark.prove(ctx, tr, pub)
    want = so.prove(ores.rows, opub)
    assert proof[9] == mode and len(proof) == len(want)
    if not np.array_equal(proof, want):
        bad = np.nonzero(proof != want)[0]
        raise AssertionError(f"mode-{mode} proof differs at word {bad[0]} of {len(want)} ({len(bad)} words differ)")
    assert so.verify(proof, opub) == 0 and rt.verify(proof, pub) == 0 and rt.verify(proof) == 0
    for pos in (8, 30, 160, len(proof) // 2, len(proof) - 1):
        t = proof.copy()
        t[pos] = (int(t[pos]) + 1) % P
        assert so.verify(t) != 0 and rt.verify(t) == so.verify(t), pos
    ctx.close(); log.close()


def _refused(which, mode, witness):
    from zkir_amd import pipeline as pl, stark
    blob, ins, cfg = getattr(programs, which)()
    log = rt.interpret(blob, ins, rt.VMConfig(enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    ctx = stark.StarkContext(stark.padded_log_n(log.n_rows))
    try:
        with pytest.raises(rt.RuntimeError) as e:
            pub = rt.public_inputs(log, blob, ins, mem_mode=mode == 3, wide_mode=mode == 4, mem_witness=witness)
            stark.prove(ctx, tr, pub)
    finally:
        ctx.close(); log.close()
    assert e.value.code == rt.ERR_ARGUMENT
    return e.value.message


@pytest.mark.parametrize("witness", ["device", "host"])
@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("which", ["edge_at_2p40", "edge_above_2p40"])
def test_accesses_at_or_above_2p40_are_refused(which, mode, witness):
    """No proof states an address of 2^40 or more: the prover refuses — memcheck.hip on the device path, the host's replay on the other — naming why."""
    msg = _refused(which, mode, witness)
    assert ("accesses an address of 2^40 or more" in msg) if witness == "device" else ("is not below 2^40" in msg), msg


@pytest.mark.parametrize("witness", ["device", "host"])
@pytest.mark.parametrize("which", ["edge_bc_alias_low_1", "edge_bc_alias_low_68"])
def test_a_boundary_cell_alias_store_is_refused(which, witness):
    """a store into the low half of B + 8 p j has delta = 0 in I_BC, so its row violates I_BC + 1 — the oracle's proof of it is rejected (10,
    tests/test_memory_edges.py).  The GPU prover refuses the run (lookup_index_kernel reports the row) instead of emitting a proof that does not verify."""
    msg = _refused(which, 4, witness)
    assert "has no proof in this AIR" in msg and "B + 8 p j" in msg, msg


@pytest.mark.parametrize("which,needle", [("hash_edge_len_over", "is outside what a proof states"), ("hash_edge_out_over_2p40", "is outside what a proof states"),
                                          ("hash_edge_in_over_code", "overlaps the code segment"), ("hash_edge_out_over_code", "overlaps the code segment")])
def test_hash_calls_without_a_proof_are_refused(which, needle):
    """Hash calls a mode-4 proof cannot state (more than 1 MiB of input, an output past 2^40, a buffer over the code): the prover refuses with a message; both verifiers reject
    the oracle's proof of the run with the same code (tests/test_memory_edges.py)."""
    msg = _refused(which, 4, "device")
    assert needle in msg, msg
