"""zkir_lowdeg_verify_device / zkir_eval_verify_device / zkir_batch_eval_verify_device: the commitment layer's verifiers with checks 7 - 11 of all queries on the GPU.
Every comparison is three-way and exact: device verdict == host entry's verdict == the reference's verify_ref (lowdeg_ref, eval_ref, batch_eval_ref).  Proofs come from the
CPU references unless a test says otherwise.  No test provokes a device fault: the equal verdicts on mutants are what shows that the kernels read what the checked header
states and nothing else."""
from __future__ import annotations

import functools
import threading

import numpy as np
import pytest

import batch_eval_ref as be
import eval_ref as ev
import lowdeg_ref as ld
import test_batch_eval_verify as tb
import test_eval_verify as te
import test_lowdeg_verify as tl
from zkir_amd import runtime as rt

pytestmark = pytest.mark.gpu

P = ld.P
REF = {"ld": ld.verify_ref, "ev": ev.verify_ref, "be": be.verify_ref}
HOST = {"ld": rt.lowdeg_verify, "ev": rt.eval_verify, "be": rt.batch_eval_verify}
LAYOUT = {"ld": ld.layout, "ev": ev.layout, "be": be.layout}
NO_LAUNCH = (1, 2, 3, 4, 5, 12, 13)                               # verdicts reached before the query stage


def device_verdict(kind, t, *exp, stream=None) -> int:
    return HOST[kind](t, *exp, device=True, stream=stream)


def jobs_of(kind, t):
    """(hash_jobs, value_jobs) the header of `t` (one that passed check 1) asks for"""
    if kind == "ld":
        n_mats, nq, n_layers = 1, int(t[5]), int(t[7])
    else:
        n_mats, nq, n_layers = (int(t[4]) if kind == "be" else 1), int(t[6]), int(t[8])
    return nq * (2 * n_mats + n_layers), nq * (2 + n_layers)


def three(kind, t, *exp, stream=None) -> int:
    """the verdict all three give; the device entry's job counts are what the verdict says they must be"""
    host, ref = HOST[kind](t, *exp), REF[kind](t, *exp)
    dev = device_verdict(kind, t, *exp, stream=stream)
    jobs = rt.pcs_verify_last_jobs()
    assert dev == host == ref, f"{kind}: device {dev}, host {host}, reference {ref}"
    assert jobs == ((0, 0) if dev in NO_LAUNCH else jobs_of(kind, t)), (kind, dev, jobs)
    return dev


def bump(pr, *positions):
    t = pr.copy()
    for at in positions:
        t[at] = (int(t[at]) + 1) % P
    return t


# ---- shapes --------------------------------------------------------------------------------------------------------------------------------------------------------------
# 'ZKLD' (log_n, b, width, num_queries, pow_bits): the CPU suite's (every schedule class: [1], [1], [1,1], [1,2], [1,3], [1,3,1]; b = 1, 2, 3; pow_bits 0), then the kernel
# edges at log_n 3, b 1: one word, a ragged block, one block, one block and a word, three ragged blocks, 19 blocks, 64 blocks (every lane of the value kernel takes eight
# columns); one query; 128 queries
LD_SHAPES = list(tl.SHAPES) + [(3, 1, w, 2, 2) for w in (1, 7, 8, 9, 17, 152, 512)] + [(4, 1, 3, 1, 0), (3, 1, 5, 128, 3)]
# 'ZKEV' (log_n, b, width, n_points, num_queries, pow_bits)
EV_SHAPES = list(te.SHAPES) + [(3, 1, 17, 2, 128, 0), (4, 3, 152, 1, 1, 2)]
# 'ZKBE' (log_n, b, ((width, mask), ..), n_points, num_queries, pow_bits): the CPU suite's, four matrices with every mask, the shape a STARK would use
BE_SHAPES = list(tb.SHAPES) + [(3, 1, ((1, 1), (1, 2), (1, 3), (1, 3)), 2, 3, 3), (5, 2, ((152, 3), (40, 3), (8, 1)), 2, 4, 3), (3, 1, ((9, 3), (8, 2)), 2, 128, 0)]


@functools.lru_cache(maxsize=None)
def ld_proof(shape):
    log_n, b, width, nq, bits = shape
    pr = ld.prove_ref(tl._matrix(log_n, b, width), b, nq, bits)
    pr.setflags(write=False)
    return pr


@functools.lru_cache(maxsize=None)
def ev_proof(shape):
    log_n, b, width, n_points, nq, bits = shape
    pr = ev.prove_ref(te.matrix(log_n, b, width), b, te.points_for(log_n, n_points), nq, bits)
    pr.setflags(write=False)
    return pr


PROOF = {"ld": ld_proof, "ev": ev_proof, "be": tb.proof}
ALL = [("ld", s) for s in LD_SHAPES] + [("ev", s) for s in EV_SHAPES] + [("be", s) for s in BE_SHAPES]
CPU_SHAPES = [("ld", s) for s in tl.SHAPES] + [("ev", s) for s in te.SHAPES] + [("be", s) for s in tb.SHAPES]


def expectations(kind, t, pr):
    """what a holder of the honest proof `pr` expects, as far as it can be held against `t`"""
    if kind == "ld":
        return (pr[8:12],)
    return te.expectations(t, pr) if kind == "ev" else tb.expectations(t, pr)


def query_section(kind, pr):
    at = LAYOUT[kind](pr)
    return at, at["queries"], len(pr)


# ---- 1: honest proofs ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", ALL)
def test_honest_proofs_are_accepted_by_both(kind, shape):
    pr = PROOF[kind](shape)
    assert three(kind, pr) == 0
    assert three(kind, pr, *expectations(kind, pr, pr)) == 0
    at = LAYOUT[kind](pr)
    if at["num_queries"] == 128:                                     # log_n 3, b 1: M / 2 = 8 rows and 128 samples — every row is opened, the first and the last among them
        assert (at["log_n"], at["b"]) == (3, 1)
        rows = {int(pr[at["queries"] + t * at["qsize"]]) for t in range(128)}
        assert rows == set(range(8)), rows


def test_the_shapes_cover_the_schedule_classes():
    ks = [tuple(ld.schedule(s[0], s[1])) for s in LD_SHAPES]
    assert {k[-1] for k in ks if len(k) > 1} == {1, 2, 3} and (1,) in ks
    assert {s[1] for s in LD_SHAPES} == {1, 2, 3} and {s[3] for s in LD_SHAPES} >= {1, 128} and 0 in {s[4] for s in LD_SHAPES}
    assert {s[2] for s in LD_SHAPES if s[:2] == (3, 1)} >= {1, 7, 8, 9, 17, 152, 512}


# ---- 2: mutants ----------------------------------------------------------------------------------------------------------------------------------------------------------
def lowdeg_mutants(pr, rng):
    """[(label, words)] of a 'ZKLD' proof, of the kinds of test_eval_verify.eval_mutants: header words at edges, the root, layer roots, final words, the nonce, the query
    index words, a record's row and path at both rows, every layer's values and path, cuts at every section boundary, extensions, bumps, words >= p, swaps, zeroed runs"""
    at = ld.layout(pr)
    n = len(pr)
    out = []

    def put(label, pos, val):
        t = pr.copy(); t[pos] = val & 0xFFFFFFFF
        out.append((label, t))
    for pos in range(8):                                             # magic, version, log_n, b, width, num_queries, pow_bits, n_layers
        for v in te.EDGES + [int(pr[pos]) + 1, max(int(pr[pos]) - 1, 0), 2, 3, 4, 24, 25, 26, 27, 128, 129, 512, 513]:
            put(f"header{pos}={v}", pos, v)
    for pos in (8, 11):
        put(f"root@{pos}+1", pos, (int(pr[pos]) + 1) % P)
    put("root>=p", 9, P)
    for j in range(len(at["ks"])):
        put("layer root+1", 12 + 4 * j + j % 4, (int(pr[12 + 4 * j + j % 4]) + 1) % P)
    for pos in (at["final"], at["final"] + 5, at["nonce"] - 1):
        put("final+1", pos, (int(pr[pos]) + 1) % P)
    for v in (0, int(pr[at["nonce"]]) + 1, P - 1, P):
        put(f"nonce={v}", at["nonce"], v)
    starts = [at["queries"] + t * at["qsize"] for t in range(at["num_queries"])]
    for s in starts:
        for v in te.EDGES + [int(pr[s]) ^ 1, int(pr[s]) + (1 << (at["log_n"] + at["b"] - 1))]:
            put(f"query@{s}={v}", s, v)
    width, rec = at["width"], at["rec"]
    for s in (starts[0], starts[-1]):
        for r0 in (s + 1, s + 1 + rec):                              # record(q), record(q + M/2): first and last row word, first and last path word
            for pos in (r0, r0 + width - 1, r0 + width, r0 + rec - 1):
                put(f"record@{pos}+1", pos, (int(pr[pos]) + 1) % P)
        for v_at, p_at, depth in at["layers"]:
            for pos in (s + v_at, s + v_at + 7):
                put(f"layer value@{pos}+1", pos, (int(pr[pos]) + 1) % P)
            if depth:
                for pos in (s + p_at, s + p_at + 4 * depth - 1):
                    put(f"layer path@{pos}+1", pos, (int(pr[pos]) + 1) % P)
    bounds = [8, 12, at["final"], at["nonce"], at["queries"]] + starts + [starts[0] + 1 + rec, starts[0] + at["layers"][0][0], starts[0] + at["layers"][0][1], n]
    for b in bounds:
        for cut in (b - 1, b, b + 1):
            if 0 <= cut <= n:
                out.append((f"cut{cut}", pr[:cut].copy()))
    for cut in rng.integers(0, n, 8):
        out.append((f"cut{cut}", pr[:int(cut)].copy()))
    for extra in (1, 3, 32):
        out.append((f"extend{extra}", np.concatenate([pr, rng.integers(0, P, extra).astype(np.uint32)])))
    for pos in rng.integers(8, n, 20):
        put(f"word{pos}+1", int(pos), (int(pr[pos]) + 1) % P)
    for pos in rng.integers(0, n, 8):
        put(f"word{pos}>=p", int(pos), [P, P + 1, 0xFFFFFFFF][int(pos) % 3])
    for _ in range(8):
        a, b = (int(x) for x in rng.integers(8, n, 2))
        t = pr.copy(); t[a], t[b] = t[b], t[a]
        out.append((f"swap{a},{b}", t))
        a = int(rng.integers(8, n))
        t = pr.copy(); t[a:a + int(rng.integers(1, 40))] = 0
        out.append((f"zero{a}", t))
    return [(label, t) for label, t in out if not (len(t) == n and np.array_equal(t, pr))]


def extra_query_mutants(kind, pr):
    """a 7, an 8 and a 9 in the LAST query, for a generator that does not make each of them: a record's first row word, layer 0's second value, layer 0's (or, where layer 0's
    tree is a single leaf, the deepest layer's) last path word"""
    at = LAYOUT[kind](pr)
    s = at["queries"] + (at["num_queries"] - 1) * at["qsize"]
    v0, p0, d0 = at["layers"][0]
    out = [("last query: record row", bump(pr, s + 1)), ("last query: layer-0 value", bump(pr, s + v0 + 4))]
    v_at, p_at, depth = max(at["layers"], key=lambda x: x[2])
    if depth:
        out.append(("last query: layer path", bump(pr, s + p_at + 4 * depth - 1)))
    return out


MUTANTS = {"ld": lowdeg_mutants, "ev": te.eval_mutants, "be": tb.batch_mutants}


@pytest.mark.parametrize("kind,shape", CPU_SHAPES)
def test_mutants_get_the_same_code(kind, shape):
    pr = PROOF[kind](shape)
    rng = np.random.default_rng(177 + shape[0])
    plain = {}
    for label, t in MUTANTS[kind](pr, rng) + extra_query_mutants(kind, pr):
        code = three(kind, t)
        assert code != 0, f"a mutant is accepted: {label}"
        plain[code] = plain.get(code, 0) + 1
        with_exp = three(kind, t, *expectations(kind, t, pr))
        assert with_exp != 0 and (with_exp == code or with_exp in (2, 13)), (label, code, with_exp)
    print(kind, shape, dict(sorted(plain.items())))
    assert {6, 7, 8, 9} <= set(plain), plain                         # (against a vacuous pass: the device stage decided mutants of each of its checks)


# ---- 3: codes 10 and 11 --------------------------------------------------------------------------------------------------------------------------------------------------
def plus_one(which):
    def hook(j, layer):
        if j != which:
            return layer
        out = layer.copy(); out[:, 0] = (out[:, 0] + np.uint64(1)) % np.uint64(P)
        return out
    return hook


@pytest.mark.parametrize("shape", tl.SHAPES)
def test_layers_that_are_not_the_fold(shape):
    """a layer committed honestly that is NOT the fold of the one before: 10 at every middle layer, 11 at the final one"""
    log_n, b, width, nq, bits = shape
    n_layers = len(ld.schedule(log_n, b))
    m = tl._matrix(log_n, b, width)
    for j in range(1, n_layers):
        assert three("ld", ld.prove_ref(m, b, nq, bits, layer_hook=plus_one(j))) == 10, j
    assert three("ld", ld.prove_ref(m, b, nq, bits, layer_hook=plus_one(n_layers))) == 11


# ---- 4: layer-0 values that are not what the rows give --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 2, 9, 4, 4), (6, 1, 5, 5, 6), (5, 3, 8, 3, 0)])
def test_a_codeword_for_another_gamma_is_an_8(shape):
    log_n, b, width, nq, bits = shape
    m = tl._matrix(log_n, b, width)
    assert three("ld", ld.prove_ref(m, b, nq, bits, codeword=ld.combine(m, np.array([1, 2, 3, 4], np.uint32)))) == 8


@pytest.mark.parametrize("shape", [tb.SHAPES[0], tb.SHAPES[2]])
def test_a_false_claim_is_refused_alike(shape):
    """evaluations with one word off by one, the honest procedure from there (one matrix; one of three, each in turn): refused by all three with one code — the reference's"""
    log_n, b, wm, n_points, nq, bits = shape
    mats, masks, pts = tb.matrices(shape), [k for _, k in wm], tb.points_for(log_n, n_points)
    y = be.evaluate(mats, b, masks, pts)
    at = be.layout(tb.proof(shape))
    for (i, m), pos in at["evals_of"].items():
        off = y.copy()
        e = (pos - at["evals"]) // 4 + wm[m][0] - 1
        off[e, 3] = (off[e, 3] + np.uint64(1)) % np.uint64(P)
        assert three("be", be.prove_ref(mats, b, masks, pts, nq, bits, evals=off)) != 0, (i, m)


# ---- 5: the order of the checks -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", CPU_SHAPES)
def test_pairs_of_bumps_in_the_query_section(kind, shape):
    pr = PROOF[kind](shape)
    at, lo, hi = query_section(kind, pr)
    rng = np.random.default_rng(500 + shape[0] + 10 * shape[1])
    seen = set()
    for a, b in rng.integers(lo, hi, (200, 2)):
        seen.add(three(kind, bump(pr, int(a), int(b)) if a != b else bump(pr, int(a))))
    assert 0 not in seen and len(seen) >= 3, seen


@pytest.mark.parametrize("kind,shape", [("ld", (7, 2, 17, 4, 4)), ("ev", (6, 3, 9, 2, 3, 4)), ("be", tb.SHAPES[2])])
def test_named_pairs(kind, shape):
    pr = PROOF[kind](shape)
    at = LAYOUT[kind](pr)
    q0, qsize, nq = at["queries"], at["qsize"], at["num_queries"]
    last = q0 + (nq - 1) * qsize
    v0, p0, d0 = at["layers"][0]
    # lowest query first: query 0's layer-0 path (9) wins over the last query's index word (6)
    assert three(kind, bump(pr, last, q0 + p0)) == 9
    # a record word and a layer-0 value in one query: the record is checked first
    assert three(kind, bump(pr, q0 + 1, q0 + v0)) == 7
    assert three(kind, bump(pr, q0 + qsize + 1, q0 + v0)) == 8       # .. but query 0's layer-0 value (8) before query 1's record (7)
    if kind == "be":                                                 # matrix 1's record in query 0 with matrix 0's in query 1
        assert three(kind, bump(pr, q0 + at["records"][1][0], q0 + qsize + at["records"][0][0])) == 7
        assert three(kind, bump(pr, q0 + at["records"][2][1] + at["widths"][2], last)) == 7      # the last matrix's second record, its path; a later 6
    if len(at["layers"]) >= 3:                                       # layer 1's path (9) before layer 2's carried value (10 or 9: its leaf no longer hashes either way)
        v1, p1, d1 = at["layers"][1]
        v2, p2, d2 = at["layers"][2]
        assert d1 and three(kind, bump(pr, q0 + p1, q0 + v2)) == 9
    # the index word alone, in a middle query: a 6, the device's flags of the queries before it all clear
    assert three(kind, bump(pr, q0 + (nq // 2) * qsize)) == 6


# ---- 6: state and streams ------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_stream_of_the_callers():
    import torch
    from zkir_amd import stark
    s = torch.cuda.Stream()
    pr = ld_proof((6, 1, 5, 5, 6))
    at = ld.layout(pr)
    bad = bump(pr, at["queries"] + 1)
    assert stark.lowdeg_verify(pr, device=True, stream=s) == 0 and stark.lowdeg_verify(bad, device=True, stream=s) == 7 == rt.lowdeg_verify(bad)
    pe = ev_proof((5, 2, 5, 2, 4, 3))
    assert stark.eval_verify(pe, device=True, stream=s) == 0 and stark.eval_verify(pe, *te.expectations(pe, pe), device=True, stream=s) == 0
    pb = tb.proof(tb.SHAPES[2])
    assert stark.batch_eval_verify(pb, device=True, stream=s) == 0 and stark.batch_eval_verify(pb, *tb.expectations(pb, pb), device=True, stream=s) == 0
    with torch.cuda.stream(s):                                       # the current stream is the default
        assert stark.batch_eval_verify(pb, device=True) == 0
    s.synchronize()


def test_small_large_small():
    """the device block grows for the large proof and is reused by the small one after it"""
    small, large = ld_proof((3, 1, 1, 3, 0)), ld_proof((3, 1, 512, 2, 2))
    mid = tb.proof((5, 2, ((152, 3), (40, 3), (8, 1)), 2, 4, 3))
    assert len(small) < len(mid) and len(small) < len(large)
    for _ in range(2):
        for kind, pr in (("ld", small), ("ld", large), ("ld", small), ("be", mid), ("ld", small), ("ev", ev_proof(te.SHAPES[0]))):
            assert three(kind, pr) == 0
            at = LAYOUT[kind](pr)
            assert three(kind, bump(pr, at["queries"] + at["layers"][0][0])) == 8


def test_four_threads():
    cases = []
    for kind, shape in (("ld", (6, 1, 5, 5, 6)), ("ev", (5, 2, 5, 2, 4, 3)), ("be", tb.SHAPES[2]), ("ld", (3, 3, 8, 2, 4))):
        pr = PROOF[kind](shape)
        at = LAYOUT[kind](pr)
        q0 = at["queries"]
        for t in (pr, bump(pr, q0), bump(pr, q0 + 1), bump(pr, q0 + at["layers"][0][0]), bump(pr, q0 + at["qsize"] + at["layers"][-1][1]), pr[:-1], bump(pr, at["final"])):
            cases.append((kind, t, HOST[kind](t)))
    assert {c[2] for c in cases} >= {0, 1, 4, 6, 7, 8, 9}
    errors = []

    def work(k):
        try:
            for i in range(50):
                kind, t, want = cases[(7 * k + 3 * i) % len(cases)]
                got = device_verdict(kind, t)
                jobs = rt.pcs_verify_last_jobs()                     # (per thread)
                if got != want or jobs != ((0, 0) if want in NO_LAUNCH else jobs_of(kind, t)):
                    errors.append((k, i, kind, got, want, jobs))
        except Exception as e:                                       # noqa: BLE001 — a worker's failure is the test's
            errors.append((k, repr(e)))
    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors[:5]


def test_no_proof_is_malformed_and_launches_nothing():
    lib = rt.lib()
    assert three("ld", ld_proof((6, 1, 5, 5, 6))) == 0 and rt.pcs_verify_last_jobs() != (0, 0)
    empty = np.zeros(0, np.uint32)
    for kind in ("ld", "ev", "be"):
        assert three(kind, empty) == 1 and rt.pcs_verify_last_jobs() == (0, 0)
    pr = ld_proof((3, 1, 1, 3, 0))
    assert lib.zkir_lowdeg_verify_device(None, len(pr), None, None) == 1 and lib.zkir_lowdeg_verify_device(pr.ctypes.data, 0, None, None) == 1
    assert lib.zkir_eval_verify_device(None, 100, None, None, None, None) == 1 and lib.zkir_batch_eval_verify_device(None, 100, None, None, None, None) == 1
    assert rt.pcs_verify_last_jobs() == (0, 0)


# ---- 7: proofs the device made --------------------------------------------------------------------------------------------------------------------------------------------
def _query_bumps(kind, pr, seed, n):
    at, lo, hi = query_section(kind, pr)
    assert three(kind, pr) == 0
    codes = set()
    for pos in np.random.default_rng(seed).integers(lo, hi, n):
        codes.add(three(kind, bump(pr, int(pos))))
    assert 0 not in codes and len(codes) >= 2, codes


def test_a_batch_proof_of_the_device():
    import test_gpu_batch_eval as g
    from zkir_amd import stark
    log_n, b, widths, masks, nq, bits = 12, 3, [152, 40, 8], [3, 3, 1], 17, 8
    ctx = g._ctx(log_n, b)
    mats, trees = [], []
    for m, width in enumerate(widths):
        cols = np.random.default_rng(900 + m).integers(0, P, (width, 1 << log_n), dtype=np.uint32)
        mat = stark.lde(ctx, stark.to_b8(g._i32(cols).view(width, 1 << log_n)), clobber=True)
        mats.append(mat); trees.append(stark.merkle_commit(ctx, mat, width))
    pr = stark.batch_eval_prove(ctx, mats, trees, widths, masks, g._points(log_n, 2), nq, bits)
    _query_bumps("be", pr, 12, 60)


def test_a_lowdeg_proof_of_the_device():
    import test_gpu_batch_eval as g
    from zkir_amd import stark
    log_n, b, width, nq, bits = 14, 1, 24, 50, 8
    ctx = g._ctx(log_n, b)
    cols = np.random.default_rng(914).integers(0, P, (width, 1 << log_n), dtype=np.uint32)
    mat = stark.lde(ctx, stark.to_b8(g._i32(cols).view(width, 1 << log_n)), clobber=True)
    pr = stark.lowdeg_prove(ctx, mat, stark.merkle_commit(ctx, mat, width), width, nq, bits)
    _query_bumps("ld", pr, 14, 60)
