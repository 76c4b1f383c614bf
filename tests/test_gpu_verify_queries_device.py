"""zkir_verify_on_device, zkir_verify_many_on_device, zkir_verify_chain_on_device: the STARK verifier with the query stage of one proof, of many proofs or of a chain's
segments as ONE batch on the GPU (stark_verify.inl: two launches).  The reference for every verdict is the host entry on the same words.

Shapes: runs whose padded log_n is 3, 4, 5, 6 and 7 — the FRI schedules [1], [1, 1], [1, 2], [1, 3], [1, 3, 1]: one layer only, every last-step width, a middle 8-to-1
layer — in every mode (the widths), with 50 and 84 queries.  No test here provokes a device fault: a kernel's extents come from header words the host has checked, and a
query the proof's end cuts never reaches the device, which is what equal verdicts on the cuts show."""
import functools
import threading

import numpy as np
import pytest

import stark_query_cases as sq
import tape_side_ref as R
from zkir_amd import runtime as rt, stark

pytestmark = pytest.mark.gpu

ZERO = {"hash_jobs": 0, "value_jobs": 0, "launches": 0, "uploaded_words": 0}


def on_device(proof, expect=None, stream=None):
    return rt.verify(proof, expect, device=True, stream=stream, queries=True)


def jobs_of(proof):
    """(hash jobs, value jobs) of a proof that reaches its queries whole"""
    nq, nl = int(proof[4]), len(sq.SCHEDULES[int(proof[2])])
    return nq * (6 + nl), nq * (2 + nl)


def both(t, expect=None):
    """the host's verdict, which the device entry must give too"""
    host = rt.verify(t, expect)
    dev = on_device(t, expect)
    assert dev == host, ("the device form disagrees", dev, host)
    return host


@functools.lru_cache(maxsize=None)
def gpu_proof(mode):
    """(proof, public inputs) of sha256_hello from the GPU prover: mode 0, or mode 4 with the witness and the tape built on the device"""
    from zkir_amd import pipeline as pl
    blob, ins, cfg = R.real_program("sha256_hello")
    log = rt.interpret(blob, list(ins), rt.VMConfig(enable_execution_trace=True, **cfg))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    pub = rt.public_inputs(log, blob, list(ins), wide_mode=True, hash_witness="device") if mode == 4 else rt.public_inputs(log, blob, list(ins))
    ctx = stark.StarkContext(stark.padded_log_n(log.n_rows))
    proof = stark.prove(ctx, tr, pub)
    ctx.close()
    assert int(proof[9]) == mode
    return proof, pub


# ---- 1: honest proofs ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [3, 4, 5, 6, 7])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_honest_oracle_proofs_are_accepted_by_both(mode, log_n):
    proof, pub = sq.oracle_proof(mode, log_n)
    assert int(proof[2]) == log_n and len(sq.SCHEDULES[log_n]) == sq.query_layout(proof)["n_layers"]
    assert on_device(proof, pub) == rt.verify(proof, pub) == 0
    assert rt.verify_queries_last() == ZERO                        # (the last call was the host's)
    assert on_device(proof) == 0
    d = rt.verify_queries_last()
    assert (d["hash_jobs"], d["value_jobs"]) == jobs_of(proof) and d["launches"] == 2
    q = sq.query_layout(proof)
    assert d["uploaded_words"] <= len(proof) - q["trace_root"] + q["tables_words"] + 512      # (+ the shape record, the prefix tables and four 256-byte alignments)
    assert rt.verify(proof) == 0 and rt.verify_queries_last() == ZERO
    assert rt.verify(proof, device=True) == 0 and rt.verify_queries_last() == ZERO and rt.verify_last_stages()["device_stages"] == 0


@pytest.mark.parametrize("mode", [0, 4])
def test_honest_proofs_of_the_gpu_prover(mode, monkeypatch):
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_RECORDS", "0")      # (whatever the default routing of short tapes is)
    proof, pub = gpu_proof(mode)
    assert on_device(proof, pub) == rt.verify(proof, pub) == 0
    assert on_device(proof) == rt.verify(proof) == 0
    assert on_device(proof) == 0
    d = rt.verify_queries_last()
    nq, log_n = int(proof[4]), int(proof[2])
    nl = len(stark_schedule(log_n))
    assert (d["hash_jobs"], d["value_jobs"], d["launches"]) == (nq * (6 + nl), nq * (2 + nl), 2)
    if mode == 4:
        lay = stark.proof_layout(proof)
        assert int(proof[lay["hash_section"]]) > 0 and rt.verify_last_stages()["device_stages"] >= 3
        WM = int(proof[3])
        # the stage's own tables: the samples, the gamma table (8 (WM + WA) + 16 words, WA < WM), betas and the layer table, the shape record, alignments
        assert d["uploaded_words"] < len(proof) - lay["trace_root"] + nq + 16 * WM + 16 + 16 * nl + 512
        assert d["uploaded_words"] < len(proof)                    # (never the program, the multiplicities or the tapes in front of the trace root)
    assert rt.verify(proof) == 0 and rt.verify_queries_last() == ZERO
    assert rt.verify(proof, device=True) == 0 and rt.verify_queries_last() == ZERO


def stark_schedule(log_n):
    """fri_shape.h's fri_schedule(log_n, 1)"""
    ks, log_m = [], log_n + 1
    while log_m > 3:
        k = 1 if not ks else min(3, log_m - 3)
        ks.append(k); log_m -= k
    return ks


def test_the_shapes_cover_the_schedule_classes():
    assert {n: stark_schedule(n) for n in sq.SCHEDULES} == sq.SCHEDULES


# ---- 2: mutants get the host's code --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", range(sq.BUMP_CHUNKS))
@pytest.mark.parametrize("t", [0, -1])
@pytest.mark.parametrize("mode,log_n", sq.MUTANT_PROOFS)
def test_bumped_query_words_get_the_hosts_code(mode, log_n, t, chunk):
    proof, _ = sq.oracle_proof(mode, log_n)
    for what, m in sq.query_bumps(proof, t, chunk):
        assert both(m) != 0, what


@pytest.mark.parametrize("mode,log_n", sq.MUTANT_PROOFS)
def test_roots_cuts_and_a_trailing_word_get_the_hosts_code(mode, log_n):
    proof, pub = sq.oracle_proof(mode, log_n)
    assert both(proof, pub) == 0
    codes = set()
    for what, m in sq.record_bumps(proof, 0) + sq.record_bumps(proof, -1) + sq.other_mutants(proof):
        host = both(m)
        assert host != 0, what
        codes.add(host)
    assert sq.WANTED_CODES <= codes, codes                        # (a condition on the inputs: the lists reach every check of a query)


# ---- 3: checks 24, 25, 26 through the verifier's draws -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,log_n", [(0, 3), (0, 7), (4, 3), (4, 7), (2, 5), (3, 6), (1, 4)])
def test_perturbed_draws_get_the_host_stages_code(mode, log_n):
    proof, _ = sq.oracle_proof(mode, log_n)
    nl, nq = len(sq.SCHEDULES[log_n]), int(proof[4])
    cases = [(0, 0, 0), (1, 0, 24), (2, 0, 24), (3, 0, 24)] + [(4, j, 25 if j < nl - 1 else 26) for j in range(nl)] + [(5, t, 20) for t in (0, nq // 2, nq - 1)]
    for what, index, want in cases:
        host = rt.stark_query_stage_probe(proof, what, index, device=False)
        dev = rt.stark_query_stage_probe(proof, what, index, device=True)
        assert dev == host == want, (what, index, dev, host, want)


# ---- 4: many -------------------------------------------------------------------------------------------------------------------------------------------------------------
def mixed_list():
    """[(proof, expect, the honest proof it was made of)]: modes 0 - 4, log_n 3 - 7, 50 and 84 queries, honest beside bumped, cut and trailing-word proofs, bad magic, no
    words; expectations partly None, one naming another run"""
    out = []
    for mode, log_n in ((0, 3), (1, 4), (2, 5), (3, 6), (4, 7), (0, 7), (4, 3)):
        p, pub = sq.oracle_proof(mode, log_n)
        out.append((p, pub if (mode + log_n) % 2 else None, p))
    p84, pub84 = sq.oracle_proof(0, 6, 84, 16)
    assert int(p84[4]) == 84 and int(p84[6]) == 16
    out += [(p84, pub84, p84), (p84, None, p84)]
    p, pub = sq.oracle_proof(0, 5)
    q = sq.query_layout(p)
    other = sq.oracle_proof(0, 6)[1]
    out += [(sq.bump(p, q["at_queries"] + 7 * q["qsize"] + q["records"][2] + 1), pub, p), (sq.bump(p, q["at_queries"] + q["records"][8] + 4), None, p), (p[:len(p) - 9], pub, p),
            (p[:q["at_queries"] + 3 * q["qsize"] + q["records"][5]], None, p), (np.concatenate([p, np.zeros(1, np.uint32)]), pub, p), (p, other, p), (sq.bump(p, 0), pub, p),
            (np.zeros(0, np.uint32), None, p), (sq.bump(p, q["trace_root"]), None, p)]
    p4, _ = sq.oracle_proof(4, 4)
    q4 = sq.query_layout(p4)
    out += [(sq.bump(p4, q4["at_queries"] + 49 * q4["qsize"] + q4["records"][3]), None, p4), (p4, None, p4)]
    return out


def test_many_proofs_in_one_call():
    cases = mixed_list()
    proofs, expects = [c[0] for c in cases], [c[1] for c in cases]
    want = [rt.verify(p, e) for p, e in zip(proofs, expects)]
    assert {0, 1, 4, 6, 21, 23, 27, 30} <= set(want), want
    assert rt.verify_many(proofs, expects) == want
    d = rt.verify_queries_last()
    # the proofs that reached their queries: every code of the query stage (the cuts of this list lie in the queries: their 4 / 20 is the cut query's) and check 30 behind
    # it; a cut proof sends its whole queries only
    n_hash = 0
    for (p, _, honest), code in zip(cases, want):
        if code in (0, 4, 30) or 20 <= code <= 27:
            q = sq.query_layout(honest)
            n_hash += min(q["num_queries"], (len(p) - q["at_queries"]) // q["qsize"]) * (6 + q["n_layers"])
    assert d["launches"] == 2 and d["hash_jobs"] == n_hash
    assert rt.verify_many(proofs) == [rt.verify(p) for p in proofs]      # (no expectations at all)


def test_many_of_one_of_none_and_of_refused_proofs():
    p, pub = sq.oracle_proof(0, 4)
    assert rt.verify_many([p], [pub]) == [0] and rt.verify_queries_last()["launches"] == 2
    refused = [sq.bump(p, 0), p[:50], np.zeros(0, np.uint32), sq.bump(p, 9)]
    assert rt.verify_many(refused) == [rt.verify(t) for t in refused]
    assert rt.verify_queries_last() == ZERO                        # every proof refused before its queries: nothing launched
    with pytest.raises(rt.RuntimeError) as e:
        rt.verify_many([])
    assert e.value.code == 9                                       # ZKIR_ERR_ARGUMENT
    assert rt.lib().zkir_verify_many_on_device(None, None, None, 1, None, None) == 9


# ---- 5: chains -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_total,seg", [(300, 128), (65, 33)])
def test_chains_get_the_host_chains_verdict(n_total, seg):
    seen = {}
    for what, proofs, expect in sq.chain_cases(n_total, seg):
        host = rt.verify_chain(proofs, expect)
        assert rt.verify_chain(proofs, expect, device=True) == host, what
        seen[what] = host
    n = len(sq.segments(n_total, seg)[1])
    assert seen["honest"] == seen["honest, no expect"] == 0 and seen["first dropped"] == 41 and seen["swapped"] in (41, 42)
    assert seen["wrong row count"] == 44 and seen["wrong program"] == 43
    assert [seen[f"row word of segment {i}"] for i in range(n)] == [1000 * (i + 1) + 21 for i in range(n)]
    assert seen["header of segment 1, query of segment 0"] == 1000 + 27      # the lower segment's code wins
    full, proofs = sq.segments(n_total, seg)
    assert rt.verify_chain(proofs, full, device=True) == 0
    d = rt.verify_queries_last()
    assert d["launches"] == 2 and d["hash_jobs"] == sum(jobs_of(p)[0] for p in proofs)
    if (n_total, seg) == (300, 128):
        assert [int(p[2]) for p in proofs] == [7, 7, 6]


def test_a_mode_2_chain_a_chain_of_one_and_no_chain():
    full, proofs = sq.segments(65, 33, mode=2)
    assert int(proofs[0][9]) == 2 and len(proofs) >= 2
    assert rt.verify_chain(proofs, full, device=True) == rt.verify_chain(proofs, full) == 0
    assert rt.verify_chain(proofs[::-1], None, device=True) == rt.verify_chain(proofs[::-1]) != 0
    p3, pub3 = sq.oracle_proof(3, 5)
    assert rt.verify_chain([p3], pub3) == 0 == rt.verify_chain([p3], pub3, device=True)
    assert rt.verify_queries_last()["hash_jobs"] == jobs_of(p3)[0]      # (the last call was the device's)
    q = sq.query_layout(p3)
    bad = sq.bump(p3, q["at_queries"] + q["records"][5] + 1)
    assert rt.verify_chain([bad], None, device=True) == rt.verify_chain([bad]) == 22
    assert rt.verify_chain([], None, device=True) == rt.verify_chain([]) == 40


# ---- 6: state and streams ------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_stream_of_the_callers():
    import torch
    s = torch.cuda.Stream()
    p, pub = sq.oracle_proof(2, 5)
    q = sq.query_layout(p)
    bad = sq.bump(p, q["at_queries"] + q["records"][1])
    assert on_device(p, pub, stream=s.cuda_stream) == 0 and on_device(bad, stream=s.cuda_stream) == 21 == rt.verify(bad)
    assert rt.verify_many([p, bad], stream=s.cuda_stream) == [0, 21]
    full, proofs = sq.segments(65, 33)
    assert rt.verify_chain(proofs, full, device=True, stream=s.cuda_stream) == 0
    s.synchronize()


def test_small_large_small():
    """the device block grows for the large batch and is reused by the small one after it"""
    small, large = sq.oracle_proof(0, 3)[0], sq.oracle_proof(4, 7)[0]
    many = [sq.oracle_proof(m, 7)[0] for m in (0, 1, 2, 3, 4)] * 3
    assert len(small) < len(large)
    bad = sq.bump(small, sq.query_layout(small)["at_queries"] + sq.query_layout(small)["records"][7])
    for _ in range(2):
        assert both(small) == 0 and both(large) == 0 and both(small) == 0
        assert rt.verify_many(many) == [0] * len(many)
        assert both(small) == 0 and both(bad) == 23


def test_four_threads():
    cases = []
    for mode, log_n in ((0, 3), (2, 5), (4, 4), (0, 7)):
        p, _ = sq.oracle_proof(mode, log_n)
        q = sq.query_layout(p)
        for t in (p, sq.bump(p, q["at_queries"]), sq.bump(p, q["at_queries"] + q["records"][3]), sq.bump(p, q["at_queries"] + q["qsize"] + q["records"][7] + 1), p[:-1], sq.bump(p, 0)):
            cases.append((t, rt.verify(t)))
    assert {c[1] for c in cases} >= {0, 1, 4, 20, 23, 27}
    errors = []

    def work(k):
        try:
            for i in range(12):
                t, want = cases[(7 * k + 5 * i) % len(cases)]
                got = on_device(t)
                d = rt.verify_queries_last()                         # (per thread)
                if got != want or (d["launches"] != 2 and want != 1):
                    errors.append((k, i, got, want, d))
        except Exception as e:                                       # noqa: BLE001 — a worker's failure is the test's
            errors.append((k, repr(e)))
    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors[:5]


def test_many_directly_after_a_mode_4_tape_verification(monkeypatch):
    """the tape stages and the query stage share the device block and the pinned staging: a batch right behind a tape verification, and a batch WITH a tape proof in it"""
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_RECORDS", "0")
    p4, pub4 = gpu_proof(4)
    p0, _ = sq.oracle_proof(0, 5)
    assert rt.verify(p4, pub4, device=True) == 0 and rt.verify_last_stages()["device_stages"] >= 3
    assert rt.verify_many([p0, p4, p0], [None, pub4, None]) == [0, 0, 0]
    assert rt.verify_last_stages()["device_stages"] >= 3 and rt.verify_queries_last()["launches"] == 2
    q = sq.query_layout(p0)
    bad = sq.bump(p0, q["at_queries"] + q["records"][2])
    assert rt.verify_many([p4, bad, p4[:len(p4) - 1]]) == [0, rt.verify(bad), rt.verify(p4[:len(p4) - 1])]
