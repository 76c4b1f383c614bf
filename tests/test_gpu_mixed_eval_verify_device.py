"""zkir_mixed_eval_verify_device: the mixed-height verifier ('ZKMH') with checks 7 - 11 of all queries on the GPU.  Every comparison is three-way and exact: device verdict ==
rt.mixed_eval_verify == mixed_eval_ref.verify_ref, and after each device call the job counts are the header's, or (0, 0) when the verdict was reached before the query
stage.  Proofs come from mx.prove_ref on the CPU unless a test says otherwise.  No test provokes a device fault: the equal verdicts on mutants are what shows that the
kernels read what the checked header states and nothing else."""
from __future__ import annotations

import threading

import numpy as np
import pytest

import lowdeg_ref as ld
import mixed_eval_ref as mx
import test_batch_eval_verify as tb
import test_mixed_eval_stage as ts
from test_mixed_eval_verify import SHAPES, expectations, groups_of, mixed_mutants, proof
from zkir_amd import runtime as rt

pytestmark = pytest.mark.gpu

P = ld.P
NO_LAUNCH = (1, 2, 3, 4, 5, 12, 13)                               # verdicts reached before the query stage
# Two more shapes.  WIDE: a group-0 matrix of 130 columns (the value wave's column loop: two full passes of 64 lanes and a tail of 2; 17 sponge blocks, the last of 2
# words) and a lower matrix of 70 (a pass and a tail of 6; 70 = 8 * 8 + 6).  FOUR: four matrices in the lower group, every mask — 2 + 4 + 3 hash slots a query.
WIDE = ((5, 3), 1, ((((130, 1),), 1), (((70, 0b11),), 2)), 2, 2)
FOUR = ((4, 3), 1, ((((2, 0b11),), 2), (((1, 1), (2, 2), (1, 3), (3, 3)), 2)), 3, 2)
ALL = list(SHAPES) + [WIDE, FOUR]
ids = lambda s: f"{s[0]}/{s[1]}/{sum(len(wm) for wm, _ in s[2])}m"


def jobs_of(t):
    """(hash_jobs, value_jobs) the header of `t` (one that passed check 1) asks for"""
    groups = rt.mixed_eval_groups(t)[0]
    nq, n_layers = int(t[4]), int(t[6])
    n_mats = [len(g["widths"]) for g in groups]
    return nq * (2 * n_mats[0] + sum(n_mats[1:]) + n_layers), nq * (2 + (len(groups) - 1) + n_layers)


def three(t, *exp, stream=None) -> int:
    """the verdict all three give; the device entry's job counts are what the verdict says they must be"""
    host, ref = rt.mixed_eval_verify(t, *exp), mx.verify_ref(t, *exp)
    dev = rt.mixed_eval_verify(t, *exp, device=True, stream=stream)
    jobs = rt.pcs_verify_last_jobs()
    assert dev == host == ref, f"device {dev}, host {host}, reference {ref}"
    assert jobs == ((0, 0) if dev in NO_LAUNCH else jobs_of(t)), (dev, jobs)
    return dev


def bump(pr, *positions):
    t = pr.copy()
    for at in positions:
        t[at] = (int(t[at]) + 1) % P
    return t


# ---- 1: honest proofs ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ALL, ids=ids)
def test_honest_proofs_are_accepted_by_all_three(shape):
    pr = proof(shape)
    assert three(pr) == 0 and rt.pcs_verify_last_jobs() == jobs_of(pr)
    assert three(pr, *expectations(pr, pr)) == 0


def test_the_shapes_cover_the_paths():
    ks = {(s[0], s[1]): mx.schedule(s[0], s[1]) for s in ALL}
    assert {len(s[0]) for s in ALL} == {2, 3} and {s[1] for s in ALL} == {1, 2, 3}
    assert ks[((8, 4), 1)] == [1, 3, 2] and ks[((7, 5, 3), 1)] == [1, 1, 2, 1]      # a k = 3 step into a lower layer; k = 1 steps
    assert {n for s in ALL for _, n in s[2][1:]} == {1, 2}                          # one and two points in a lower group
    assert any(k != (1 << n) - 1 for s in ALL for wm, n in s[2] for _, k in wm)      # masks that skip a point
    assert WIDE[2][0][0][0][0] == 130 and WIDE[2][1][0][0][0] == 70 and len(FOUR[2][1][0]) == 4
    assert jobs_of(proof(FOUR))[0] == 3 * (2 + 4 + len(ks[((4, 3), 1)]))


# ---- 2: mutants ----------------------------------------------------------------------------------------------------------------------------------------------------------
STAGE_CODES = {}


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_mutants_get_the_same_code_three_ways(shape):
    pr = proof(shape)
    rng = np.random.default_rng(277 + sum(shape[0]))
    codes = {}
    for i, (label, t) in enumerate(mixed_mutants(pr, rng)):
        roots, pts, ys = expectations(t, pr)
        code = three(t, *[(None, None, None), (roots, None, None), (roots, pts, ys), (None, pts, ys)][i % 4])
        assert code != 0, f"a mutant is accepted: {label}"
        codes[code] = codes.get(code, 0) + 1
    print(shape[:2], dict(sorted(codes.items())))
    assert {1, 2, 3, 5, 6, 7, 8, 9, 12, 13} <= set(codes), codes
    STAGE_CODES[shape] = set(codes) - set(NO_LAUNCH)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[4]], ids=ids)
def test_a_false_evaluation_over_the_true_codewords(shape):
    """8 in group 0 and 10 in a lower group: the fold lane's + F_h"""
    log_ns, b, _, nq, bits = shape
    groups = groups_of(shape)
    y = mx.evaluate(groups, b)
    for h, g in enumerate(mx.layout(proof(shape))["groups"]):
        off = y.copy()
        off[g["first_e"], 0] = (off[g["first_e"], 0] + np.uint64(1)) % np.uint64(P)
        assert three(mx.prove_ref(groups, b, nq, bits, evals=off, quotient_evals=y)) == (8 if h == 0 else 10), h


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[4]], ids=ids)
def test_a_lower_record_opened_at_another_row_than_q_mod_m_is_a_7(shape):
    M0 = 1 << (shape[0][0] + shape[1])
    pr = mx.prove_ref(groups_of(shape), shape[1], shape[3], shape[4], low_q=lambda q, Mh: q * Mh // (M0 // 2))
    at = mx.layout(pr)
    qs = ts.samples(pr)
    assert any(q * (1 << g["log_M"]) // (M0 // 2) != q % (1 << g["log_M"]) for q in qs for g in at["groups"][1:])
    assert three(pr) == 7


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4], SHAPES[5]], ids=ids)
def test_a_final_layer_the_last_fold_does_not_give_is_an_11(shape):
    assert three(mx.prove_ref(groups_of(shape), shape[1], shape[3], shape[4], final_add=[1, 0, 2, P - 1])) == 11


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4], WIDE, FOUR], ids=ids)
def test_the_order_of_the_checks(shape):
    pr = proof(shape)
    at = mx.layout(pr)
    q0, qsize, nq, G = at["queries"], at["qsize"], at["num_queries"], at["groups"]
    # one word of a lower group's record: its leaf no longer hashes (7) — and the F_h formed from it is another too, which a 10 would show: 7 stands first
    for h in range(1, len(G)):
        for m in range(len(G[h]["widths"])):
            r0 = G[h]["records"][m][0]
            assert three(bump(pr, q0 + r0)) == 7 and three(bump(pr, q0 + r0 + G[h]["widths"][m] - 1)) == 7, (h, m)
    v0, p0, _ = at["layers"][0]
    last_rec = G[-1]["records"][-1][0]
    assert three(bump(pr, q0 + last_rec, q0 + v0)) == 7             # the last record of the query before its layer-0 values
    assert nq >= 2
    assert three(bump(pr, q0 + qsize + 1, q0 + v0)) == 8            # query 0's 8 before query 1's 7
    assert three(bump(pr, q0 + (nq - 1) * qsize, q0 + p0)) == 9     # lowest query first: query 0's layer-0 path before the last query's index word
    # an index word bumped in a middle query: a 6, every earlier query's flags clear
    assert three(bump(pr, q0 + (nq // 2) * qsize)) == 6


def test_the_device_stage_decided_every_one_of_its_codes():
    """a guard against a vacuous pass: over the mutants and the named cases the stage's flags gave 6, 7, 8, 9, 10 and 11"""
    seen = set().union(*STAGE_CODES.values()) if STAGE_CODES else set()
    if not seen >= {6, 7, 8, 9}:                                     # (run alone: the mutants of one shape)
        pr = proof(SHAPES[1])
        seen |= {three(t) for _, t in mixed_mutants(pr, np.random.default_rng(281))} - set(NO_LAUNCH)
    shape = SHAPES[1]
    groups, y = groups_of(shape), mx.evaluate(groups_of(shape), shape[1])
    off = y.copy()
    e = mx.layout(proof(shape))["groups"][1]["first_e"]
    off[e, 0] = (off[e, 0] + np.uint64(1)) % np.uint64(P)
    seen.add(three(mx.prove_ref(groups, shape[1], shape[3], shape[4], evals=off, quotient_evals=y)))
    seen.add(three(mx.prove_ref(groups, shape[1], shape[3], shape[4], final_add=[1, 0, 2, P - 1])))
    assert seen >= {6, 7, 8, 9, 10, 11}, seen


# ---- 3: the maximal layer table ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [1, 2], ids=["pair", "triple"])
def test_hollow_ten_layer_proofs(which):
    best, _, triple = ts.longest_schedules()
    assert best == ts.MAX_LAYERS == 10                               # no pair or triple has more
    log_ns, b = ts.LONG_PAIR if which == 1 else triple
    pr = ts.hollow(log_ns, b)
    assert int(pr[6]) == 10 and jobs_of(pr) == (2 * (2 + (len(log_ns) - 1) + 10), 2 * (2 + (len(log_ns) - 1) + 10))
    assert three(pr) in (6, 7) and rt.pcs_verify_last_jobs() == jobs_of(pr)
    assert three(ts.with_index_words(pr)) == 7 and rt.pcs_verify_last_jobs() == jobs_of(pr)


# ---- 4: proofs the device made ---------------------------------------------------------------------------------------------------------------------------------------------
def test_a_mixed_proof_of_the_device():
    import test_gpu_mixed_eval as g
    from zkir_amd import stark
    shape = g.SHAPES[4]                                              # (7, 5, 3) at b = 1
    dev, ref, got, want = g._shape(shape)
    assert np.array_equal(got, want)
    assert stark.mixed_eval_verify(got, device=True) == 0 == three(got) and three(got, *expectations(got, got)) == 0
    at = mx.layout(got)
    codes = {three(bump(got, int(pos))) for pos in np.random.default_rng(19).integers(at["queries"], len(got), 12)}
    assert 0 not in codes and len(codes) >= 2, codes


# ---- 5: state and streams --------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_stream_of_the_callers():
    import torch
    from zkir_amd import stark
    s = torch.cuda.Stream()
    pr = proof(SHAPES[4])
    bad = bump(pr, mx.layout(pr)["queries"] + 1)
    assert stark.mixed_eval_verify(pr, device=True, stream=s) == 0 and stark.mixed_eval_verify(bad, device=True, stream=s) == 7 == rt.mixed_eval_verify(bad)
    assert stark.mixed_eval_verify(pr, *expectations(pr, pr), device=True, stream=s) == 0 and stark.mixed_eval_verify(pr) == 0
    with torch.cuda.stream(s):                                       # the current stream is the default
        assert stark.mixed_eval_verify(pr, device=True) == 0
    s.synchronize()


def test_small_large_small_and_the_batch_entry_between():
    """the device block grows for the large proof and is reused by the small one after it; zkir_batch_eval_verify_device shares the block and the job counts"""
    small, large, pb = proof(SHAPES[0]), proof(WIDE), tb.proof(tb.SHAPES[2])
    assert len(small) < len(large)
    for _ in range(2):
        for pr in (small, large, small):
            assert three(pr) == 0
            assert three(bump(pr, mx.layout(pr)["queries"] + mx.layout(pr)["layers"][0][0])) == 8
            assert rt.batch_eval_verify(pb, device=True) == 0 == rt.batch_eval_verify(pb)
            assert rt.pcs_verify_last_jobs() == (int(pb[6]) * (2 * int(pb[4]) + int(pb[8])), int(pb[6]) * (2 + int(pb[8])))
            assert three(pr) == 0


def test_four_threads():
    cases = []
    for shape in (SHAPES[1], SHAPES[4], WIDE, FOUR):
        pr = proof(shape)
        at = mx.layout(pr)
        q0 = at["queries"]
        for t in (pr, bump(pr, q0), bump(pr, q0 + 1), bump(pr, q0 + at["layers"][0][0]), bump(pr, q0 + at["qsize"] + at["layers"][-1][1]), pr[:-1], bump(pr, at["final"])):
            want = rt.mixed_eval_verify(t)
            assert want == mx.verify_ref(t)
            cases.append((t, want))
    assert {c[1] for c in cases} >= {0, 1, 4, 6, 7, 8, 9}
    errors = []

    def work(k):
        try:
            for i in range(40):
                t, want = cases[(7 * k + 3 * i) % len(cases)]
                got = rt.mixed_eval_verify(t, device=True)
                jobs = rt.pcs_verify_last_jobs()                     # (per thread)
                if got != want or jobs != ((0, 0) if want in NO_LAUNCH else jobs_of(t)):
                    errors.append((k, i, got, want, jobs))
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
    pr = proof(SHAPES[0])
    assert three(pr) == 0 and rt.pcs_verify_last_jobs() != (0, 0)
    assert three(np.zeros(0, np.uint32)) == 1 and rt.pcs_verify_last_jobs() == (0, 0)
    assert three(pr) == 0
    assert lib.zkir_mixed_eval_verify_device(None, len(pr), None, None, None, None) == 1 and rt.pcs_verify_last_jobs() == (0, 0)
    assert lib.zkir_mixed_eval_verify_device(pr.ctypes.data, 0, None, None, None, None) == 1 and rt.pcs_verify_last_jobs() == (0, 0)
