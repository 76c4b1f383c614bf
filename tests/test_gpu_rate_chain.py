"""A run proven in segments at blow-up 2, 4 and 8 on the GPU (stark.prove_rate_segment) and verified as one run (rt.verify_rate_chain, host and device), and the batched
query stage behind the device entries (rt.verify_rate_segment / verify_rate_chain with device=True, rt.verify_rate_many, rt.pcs_verify_many).  Segment proofs are held word
for word against tests/prove_rate_ref.py on the oracle's rows; every device verdict is held against the host entry's, which tests/test_rate_chain_host.py holds against the
reference.  No test provokes a device fault: equal verdicts on mutants are what shows that the kernels read what the checked headers state and nothing else."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import prove_rate_ref as pr
import rate_chain_ref as rc
import test_gpu_pcs_verify_device as tp
import test_gpu_stark as gs
from oracle import api as oracle, stark_api as so
from zkir_amd import runtime as rt

pytestmark = pytest.mark.gpu
P = so.P
N_RUN, NQ = 64, 3
CUTS = {"A": [(0, 9), (8, 40), (39, 64)], "B": [(0, 33), (32, 64), (63, 64)]}       # log_n 4, 5, 5; 6, 5 and the one-row tail at log_n 3
BITS = {"A": 0, "B": 4}


@functools.lru_cache(maxsize=None)
def run_case(name):
    """(blob, host log, oracle rows, oracle public inputs, product public inputs) of a 64-cycle run"""
    mk, cfg = gs.PROGRAMS[name]
    blob = mk().to_bytes()
    deferred = bool(cfg.get("enable_deferred_model"))
    log = rt.interpret(blob, [], rt.VMConfig(enable_execution_trace=True, max_cycles=N_RUN, **cfg))
    res = oracle.run(blob, enable_execution_trace=True, max_cycles=N_RUN, **cfg)
    assert log.n_rows == len(res.rows) == N_RUN
    opub = so.public_inputs(N_RUN, blob, [], list(res.outputs), (res.halt_kind, res.halt_code), deferred=deferred)
    return blob, log, res.rows, opub, rt.public_inputs(log, blob, [], deferred)


def shard_proof(log, run_pub, a, e, b, nq, bits, **io):
    """rows [a, e) of `log` through K1 and stark.prove_rate_segment on their own"""
    from zkir_amd import pipeline as pl, stark
    sh = log.shard(a, e)
    ddl = pl.upload(sh); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    pub = rt.PublicInputsC.from_buffer_copy(run_pub); pub.n_real = e - a
    for k, v in io.items():
        setattr(pub, k, v)
    ctx = stark.StarkContext(stark.padded_log_n(e - a), b)
    proof = stark.prove_rate_segment(ctx, tr, pub, nq, bits)
    return proof, ctx, sh


@functools.lru_cache(maxsize=None)
def gpu_segment(name, a, e, b, nq, bits):
    _, log, _, _, run_pub = run_case(name)
    proof, ctx, sh = shard_proof(log, run_pub, a, e, b, nq, bits)
    ctx.close(); sh.close()
    proof.setflags(write=False)
    return proof


def gpu_chain(name, cuts, b):
    return [gpu_segment(name, a, e, b, NQ, BITS[cuts]) for a, e in CUTS[cuts]]


def jobs_of(proofs):
    """(hash jobs, value jobs) of the embedded proofs of 'ZKSR' proofs: sum nq (2 n_mats + n_layers), sum nq (2 + n_layers)"""
    from zkir_amd import stark
    h = v = 0
    for p in proofs:
        e = p[stark.rate_proof_layout(p)["eval_proof"]:]
        n_mats, nq, n_layers = int(e[4]), int(e[6]), int(e[8])
        h += nq * (2 * n_mats + n_layers); v += nq * (2 + n_layers)
    return h, v


@pytest.mark.parametrize("b", [1, 2, 3])
@pytest.mark.parametrize("cuts", ["A", "B"])
@pytest.mark.parametrize("name", ["fib", "deferred"])
def test_segment_proofs_equal_the_reference_word_for_word(name, cuts, b):
    _, _, rows, opub, run_pub = run_case(name)
    proofs = gpu_chain(name, cuts, b)
    for (a, e), proof in zip(CUTS[cuts], proofs):
        want = pr.prove_ref(rows[a:e], rc.segment_pub(opub, a, e), b, NQ, BITS[cuts])
        assert len(proof) == len(want)
        if not np.array_equal(proof, want):
            bad = np.nonzero(proof != want)[0]
            raise AssertionError(f"rows [{a}, {e}): the proof differs from the reference at word {bad[0]} of {len(want)} ({len(bad)} words differ)")
    assert [int(p[2]) for p in proofs] == ([4, 5, 5] if cuts == "A" else [6, 5, 3])
    for device in (False, True):
        assert rt.verify_rate_chain(proofs, run_pub, NQ, BITS[cuts], device=device) == 0 and rt.verify_rate_chain(proofs, None, device=device) == 0
        for i, p in enumerate(proofs):
            code, first, last = rt.verify_rate_segment(p, None, NQ, BITS[cuts], device=device)
            assert code == 0 and np.array_equal(first, p[21:21 + 68]) and np.array_equal(last, p[21 + 68:21 + 136])
            assert rt.verify_rate(p, None, 1, 0, device=device) == (0 if i == 0 else 7)


@pytest.mark.parametrize("name,b", [("fib", 1), ("deferred", 2), ("fib", 3)])
def test_a_whole_run_gets_prove_rates_words(name, b):
    from zkir_amd import stark
    blob, log, tr, rows, opub, pub = gs._case(name, N_RUN)
    ctx = stark.StarkContext(6, b)
    whole = stark.prove_rate_segment(ctx, tr, pub, 4, 4)
    assert np.array_equal(whole, stark.prove_rate(ctx, tr, pub, 4, 4))
    assert rt.verify_rate(whole, pub, 4, 4) == 0 and rt.verify_rate_chain([whole], pub, 4, 4) == 0 and rt.verify_rate_chain([whole], pub, 4, 4, device=True) == 0
    ctx.close(); log.close()


def same(proofs, expect=None, min_q=1, min_bits=0):
    """the chain verdict host and device give"""
    host, device = rt.verify_rate_chain(proofs, expect, min_q, min_bits), rt.verify_rate_chain(proofs, expect, min_q, min_bits, device=True)
    assert host == device, f"host {host}, device {device}"
    return host


@pytest.mark.parametrize("name,cuts,b", [("fib", "A", 2), ("deferred", "B", 3)])
def test_wrong_chains_get_the_host_code_on_the_device(name, cuts, b):
    s = gpu_chain(name, cuts, b)
    run_pub = run_case(name)[4]
    (a1, e1), bits = CUTS[cuts][1], BITS[cuts]
    assert same(s, run_pub) == 0 and same([]) == 40 and same(s[1:]) == 41 and same([s[0], s[2]]) == 42 and same([s[0], s[1], s[1]]) == 42
    other_name = "deferred" if name == "fib" else "fib"
    for other in (gpu_segment(name, a1, e1, b % 3 + 1, NQ, bits), gpu_segment(name, a1, e1, b, NQ + 1, bits), gpu_segment(other_name, a1, e1, b, NQ, bits)):
        assert same([s[0], other, s[2]], run_pub) == 43
    o = rt.PublicInputsC.from_buffer_copy(run_pub); o.n_real = N_RUN + 1
    assert same(s, o) == 44
    assert same(s, run_pub, NQ + 1, 0) == 1002
    for i in range(3):
        t = [p.copy() for p in s]
        t[i][-1] = (int(t[i][-1]) + 1) % P                                      # the last word of the last query
        chain_code = same(t, run_pub)
        code, first, _ = rt.verify_rate_segment(t[i], None, device=True)
        assert code == rt.verify_rate_segment(t[i])[0] and 106 < code < 112 and chain_code == 1000 * (i + 1) + code and not first.any()


@pytest.mark.parametrize("name,cuts,b", [("fib", "A", 2), ("deferred", "B", 1)])
def test_single_word_mutants_get_the_host_code_on_the_device(name, cuts, b):
    """about 150 mutants across the chain: word `pos` of segment k becomes (w + 1 + r) mod p"""
    s = gpu_chain(name, cuts, b)
    run_pub = run_case(name)[4]
    rng = np.random.default_rng(77 + b)
    codes = set()
    for it in range(150):
        k = it % 3
        lo = len(s[k]) // 2 if it % 2 else 0                                    # half of them inside the embedded proof's query section
        pos = int(rng.integers(lo, len(s[k])))
        t = [p.copy() for p in s]
        t[k][pos] = (int(t[k][pos]) + 1 + int(rng.integers(0, 1000))) % P
        code = same(t, run_pub)
        assert code != 0 and code // 1000 == k + 1, (k, pos, code)
        codes.add(code % 1000)
    assert any(c > 105 for c in codes) and any(c < 100 for c in codes), sorted(codes)


def test_the_stage_reports_what_it_ran():
    s = gpu_chain("fib", "A", 2)
    assert rt.verify_rate_chain(s, None, device=True) == 0
    last = rt.verify_queries_last()
    h, v = jobs_of(s)
    assert (last["hash_jobs"], last["value_jobs"], last["launches"]) == (h, v, 2) and last["uploaded_words"] > sum(len(p) - pr.layout(p)["eval_proof"] for p in s)
    # segment 1 fails its front: segment 0 alone reaches the stage; segment 0 fails its front: nothing is launched
    t = [p.copy() for p in s]; t[1][2] = 9
    assert rt.verify_rate_chain(t, None, device=True) == 2002
    last = rt.verify_queries_last()
    assert (last["hash_jobs"], last["value_jobs"], last["launches"]) == (*jobs_of(s[:1]), 2)
    t = [p.copy() for p in s]; t[0][2] = 9
    assert rt.verify_rate_chain(t, None, device=True) == 1002
    last = rt.verify_queries_last()
    assert (last["hash_jobs"], last["value_jobs"], last["launches"], last["uploaded_words"]) == (0, 0, 0, 0)
    assert rt.verify_rate_segment(s[1], None, device=True)[0] == 0
    last = rt.verify_queries_last()
    assert (last["hash_jobs"], last["value_jobs"], last["launches"]) == (*jobs_of(s[1:2]), 2)
    assert rt.verify_rate_chain(s, None) == 0 and rt.verify_queries_last()["launches"] == 0      # a host entry


# ---- mode 2: the 400-output loop in three segments -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mode2_chain():
    import torch
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = gs._mode2_case("writes")
    rows, n = ores.rows, len(ores.rows)
    cuts = [(0, n // 3), (n // 3 - 1, 2 * n // 3), (2 * n // 3 - 1, n)]

    def ecalls(a, num):
        return sum(1 for r in rows[:a] if (int(r["instruction"]) & 0x7F) == 0x50 and int(r["registers"][10]) == num)
    proofs = []
    for a, e in cuts:
        proof, ctx, sh = shard_proof(log, pub, a, e, 2, 5, 4, writes_before=ecalls(a, 2), reads_before=ecalls(a, 1))
        # the embedded proof is stark.batch_eval_prove's on the matrices the segment's proof left in the workspace
        at = stark.rate_proof_layout(proof)
        inner = proof[at["eval_proof"]:]
        ia = stark.batch_eval_layout(inner)
        widths = [int(proof[3]), so.aux_width(2), 4]
        assert ia["widths"] == widths and ia["masks"] == [3, 3, 1]
        dev = [torch.from_numpy(m.view(np.int32)).cuda() for m in stark.rate_last_matrices(ctx)]
        trees = [stark.merkle_commit(ctx, d, w) for d, w in zip(dev, widths)]
        assert np.array_equal(stark.batch_eval_prove(ctx, dev, trees, widths, [3, 3, 1], inner[ia["points"]:ia["evals"]].reshape(2, 4), 5, 4), inner)
        ctx.close(); sh.close()
        proofs.append(proof)
    return proofs, cuts, ecalls, log, pub, ores


def test_mode2_chain_is_accepted_and_its_counters_link():
    from zkir_amd import stark
    proofs, cuts, ecalls, log, pub, ores = mode2_chain()
    assert all(int(p[9]) == 2 and int(p[3]) == 160 for p in proofs) and len(ores.outputs) == 400
    assert [int(p[157]) for p in proofs] == [ecalls(a, 2) for a, _ in cuts] and int(proofs[2][159]) == 400 and int(proofs[1][157]) > 0
    assert same(proofs, pub, 5, 4) == 0 and same(proofs) == 0
    assert same(proofs[:2]) == 51 and same(proofs[1:]) == 41 and same([proofs[0], proofs[2]]) == 42
    # a segment proven with writes_before off by one: the prover refuses nothing it cannot see, the chain is refused with one code on host and device
    a, e = cuts[1]
    bad, ctx, sh = shard_proof(log, pub, a, e, 2, 5, 4, writes_before=ecalls(a, 2) + 1)
    ctx.close(); sh.close()
    assert same([proofs[0], bad, proofs[2]], pub) != 0
    # a forged output word in a segment's I/O section
    at = stark.rate_proof_layout(proofs[1])
    out0 = at["io_section"] + 1 + 4 * int(proofs[1][at["io_section"]]) + 1
    t = [p.copy() for p in proofs]; t[1][out0] ^= 1
    code = same(t, pub)
    assert code // 1000 == 2 and code % 1000 in (50, 51, 10)
    host, device = rt.verify_rate_segment(t[1])[0], rt.verify_rate_segment(t[1], device=True)[0]
    assert host == device and host in (50, 51, 10)
    t = [p.copy() for p in proofs]
    for p in t:
        p[out0] ^= 1
    assert same(t, pub) % 1000 in (50, 51, 10)


def test_refusals_come_before_any_launch_with_a_message():
    from zkir_amd import stark
    blob, log, tr, rows, opub, pub = gs._case("fib", N_RUN)
    ctx = stark.StarkContext(6, 2)
    for mode in (3, 4):
        p = rt.PublicInputsC.from_buffer_copy(pub); p.deferred = mode
        with pytest.raises(rt.RuntimeError) as e:
            stark.prove_rate_segment(ctx, tr, p, 5, 4)
        assert e.value.code == rt.ERR_ARGUMENT and "zkir_prove_rate_segment" in e.value.message and "mode" in e.value.message
    for nq, bits, word in ((0, 4, "num_queries"), (129, 4, "num_queries"), (5, 25, "pow_bits")):
        with pytest.raises(rt.RuntimeError) as e:
            stark.prove_rate_segment(ctx, tr, pub, nq, bits)
        assert e.value.code == rt.ERR_ARGUMENT and "zkir_prove_rate_segment" in e.value.message and word in e.value.message
    seg = rt.PublicInputsC.from_buffer_copy(pub); seg.writes_before = 1
    for fn in (stark.prove_rate, stark.prove_rate_modes):                       # the whole-run entries keep their refusal
        with pytest.raises(rt.RuntimeError) as e:
            fn(ctx, tr, seg, 5, 4)
        assert e.value.code == rt.ERR_ARGUMENT and "segment" in e.value.message
    ctx.close(); log.close()


# ---- many independent proofs in one stage run ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def whole_proofs():
    """[(proof, public inputs)]: b = 1, 2, 3; modes 0, 1, 2; 3 and 5 queries; log_n 3 and 6"""
    from zkir_amd import stark
    out = []
    for name, n, b, nq, bits in (("fib", 5, 1, 3, 0), ("deferred", 64, 2, 5, 4), ("fib", 64, 3, 3, 0), ("deferred", 5, 3, 5, 0)):
        blob, log, tr, rows, opub, pub = gs._case(name, n)
        ctx = stark.StarkContext(stark.padded_log_n(n), b)
        out.append((stark.prove_rate(ctx, tr, pub, nq, bits), pub))
        ctx.close()
    blob, ins, ores, log, tr, opub, pub = gs._mode2_case("io")
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)), 2)
    out.append((stark.prove_rate(ctx, tr, pub, 5, 4), pub))
    ctx.close()
    return out


def test_verify_rate_many_gives_every_proofs_own_verdict():
    import torch
    good = whole_proofs()
    proofs, pubs = [p for p, _ in good], [q for _, q in good]
    assert {int(p[5]) for p in proofs} == {1, 2, 3} and {int(p[9]) for p in proofs} == {0, 1, 2} and {int(p[4]) for p in proofs} == {3, 5} and {int(p[2]) for p in proofs} >= {3, 6}
    assert rt.verify_rate_many(proofs, pubs) == [0] * 5
    last = rt.verify_queries_last()
    assert (last["hash_jobs"], last["value_jobs"], last["launches"]) == (*jobs_of(proofs), 2)
    assert [rt.verify_rate(p, q) for p, q in good] == [0] * 5
    header = proofs[1].copy(); header[2] = 9                                     # no jobs
    in_query = [proofs[2].copy(), proofs[4].copy()]
    in_query[0][-5] = (int(in_query[0][-5]) + 1) % P
    in_query[1][-40] = (int(in_query[1][-40]) + 1) % P
    for where in (0, 3, 7):
        batch = [(p, q) for p, q in good] + [(in_query[0], pubs[2]), (in_query[1], None)]
        batch.insert(where, (header, pubs[1]))
        ps, qs = [p for p, _ in batch], [q for _, q in batch]
        want = [rt.verify_rate(p, q) for p, q in batch]
        assert rt.verify_rate_many(ps, qs) == want and want[where] == 2 and sum(1 for c in want if c > 105) == 2 and want.count(0) == 5
        last = rt.verify_queries_last()
        assert (last["hash_jobs"], last["launches"]) == (jobs_of([p for k, p in enumerate(ps) if k != where])[0], 2)
    # per-proof floors, one proof, a batch in which nothing reaches its queries, another stream
    mq, mb = [int(p[4]) + (k == 1) for k, p in enumerate(proofs)], [int(p[6]) + (k == 3) for k, p in enumerate(proofs)]
    assert rt.verify_rate_many(proofs, None, mq, mb) == [0, 2, 0, 2, 0] == [rt.verify_rate(p, None, a, c) for p, a, c in zip(proofs, mq, mb)]
    assert rt.verify_rate_many([proofs[3]]) == [0] and rt.verify_rate_many([in_query[0]], [None]) == [rt.verify_rate(in_query[0])]
    short = proofs[0][:100].copy()
    want_short = rt.verify_rate(short)
    assert rt.verify_rate_many([header, short]) == [2, want_short] and want_short != 0 and rt.verify_queries_last()["launches"] == 0
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        from zkir_amd import stark
        assert stark.verify_rate_many(proofs + [in_query[1]], stream=side) == [0] * 5 + [rt.verify_rate(in_query[1])]
    side.synchronize()
    # n = 0 and n = 1025: an argument error, nothing written
    L = rt.lib()
    sentinel = (C.c_int32 * 4)(-7, -7, -7, -7)
    ptrs, lens = (C.c_void_p * 1)(proofs[0].ctypes.data), (C.c_uint64 * 1)(len(proofs[0]))
    for n in (0, 1025):
        assert L.zkir_verify_rate_many_device(ptrs, lens, None, None, None, n, sentinel, None) == rt.ERR_ARGUMENT and list(sentinel) == [-7] * 4
    assert L.zkir_verify_rate_many_device(None, lens, None, None, None, 1, sentinel, None) == rt.ERR_ARGUMENT and list(sentinel) == [-7] * 4
    with pytest.raises(rt.RuntimeError):
        rt.verify_rate_many([])


def test_verify_rate_many_takes_modes_3_and_4():
    """the frozen mode-3 and mode-4 proofs beside a small one: a mode-4 proof's tape stages run on the device before the shared query stage"""
    from test_prove_rate_modes_verify import golden
    g3, g4 = golden("mode3")[0], golden("mode4")[0]
    small = whole_proofs()[0][0]
    bad4 = g4.copy(); bad4[-1] = (int(bad4[-1]) + 1) % P
    batch = [g3, small, g4, bad4]
    want = [rt.verify_rate(p) for p in batch]
    assert want[:3] == [0, 0, 0] and want[3] > 100
    assert rt.verify_rate_many(batch) == want == [rt.verify_rate(p, device=True) for p in batch]


def test_pcs_verify_many_gives_the_host_entries_verdicts():
    """a 'ZKLD', a 'ZKEV' at one point, a 'ZKBE' of four matrices at two points and one of two matrices with masks {1, 2}; log_n 3 and 8, b 1 and 3; honest and damaged"""
    shapes = [("ld", (3, 1, 7, 3, 0)), ("ld", (8, 3, 5, 3, 2)), ("ev", (8, 1, 9, 1, 3, 2)), ("ev", (3, 3, 3, 1, 3, 0)), ("be", (3, 1, ((1, 1), (1, 2), (1, 3), (1, 3)), 2, 3, 3)),
              ("be", (8, 3, ((9, 3), (5, 1), (3, 2), (8, 3)), 2, 3, 2)), ("be", (3, 3, ((8, 1), (5, 2)), 2, 4, 0)), ("be", (8, 1, ((4, 1), (6, 2)), 2, 3, 2))]
    kind_no = {"ld": 0, "ev": 1, "be": 2}
    rng = np.random.default_rng(5)
    items = []                                                                  # (kind, words, (roots, points, evals))
    for kind, shape in shapes:
        p = tp.PROOF[kind](shape)
        exp = tuple(tp.expectations(kind, p, p)) + (None,) * (3 - len(tp.expectations(kind, p, p)))
        items.append((kind, p, (None, None, None)))
        items.append((kind, p, exp))
        at, q0, end = tp.query_section(kind, p)
        for pos in (q0, q0 + 1, q0 + at["layers"][0][0], int(rng.integers(q0, end)), end - 1):
            items.append((kind, tp.bump(p, pos), exp))
        items.append((kind, tp.bump(p, 2), (None, None, None)))                 # a header that states another length: no jobs
        items.append((kind, p[:-1].copy(), (None, None, None)))
    order = rng.permutation(len(items))
    items = [items[i] for i in order]
    want = [tp.HOST[k](t, *[x for x in exp[:1 if k == "ld" else 3]]) for k, t, exp in items]
    got = rt.pcs_verify_many([kind_no[k] for k, _, _ in items], [t for _, t, _ in items], [e[0] for _, _, e in items], [e[1] for _, _, e in items], [e[2] for _, _, e in items])
    assert got == want and want.count(0) == 16 and {1, 6, 7, 8} <= set(want), sorted(set(want))
    last = rt.verify_queries_last()
    reached = [tp.jobs_of(k, t) for (k, t, _), c in zip(items, want) if c == 0 or 6 <= c <= 11]
    assert (last["hash_jobs"], last["value_jobs"], last["launches"]) == (sum(h for h, _ in reached), sum(v for _, v in reached), 2)
    assert rt.pcs_verify_many(["eval"], [tp.PROOF["ev"](shapes[2][1])]) == [0]
    with pytest.raises(rt.RuntimeError):
        rt.pcs_verify_many([3], [tp.PROOF["ld"](shapes[0][1])])
    with pytest.raises(rt.RuntimeError):
        rt.pcs_verify_many([], [])
