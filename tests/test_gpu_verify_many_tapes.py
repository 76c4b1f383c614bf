"""zkir_tape_sections_stage_launch, zkir_verify_many_tapes_device and zkir_verify_rate_many_tapes_device (csrc/tape_stage_many.inl): the hash and wide tapes of MANY mode-4
proofs as one GPU batch — kernels that take a per-proof record from device memory, lanes of one wave in different proofs — against the host list stage, the Python reference
and the single-proof host verifier; what the batch reports; and that the entries from before it are as they were."""
import numpy as np
import pytest

import tape_digest_ref as D
import tape_many_ref as TR
import test_gpu_verify_device as tv
import test_verify_many_tapes as TH
from zkir_amd import runtime as rt, spec, stark

pytestmark = pytest.mark.gpu

NONE = {"records": 0, "launches": 0, "uploaded_words": 0}


@pytest.fixture(autouse=True)
def _every_batch_on_the_device(monkeypatch):
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_CELLS", "0")
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_RECORDS", "0")


def _three_ways(b, what=""):
    """the device stage against the host stage and the reference"""
    want = TR.stage_ref(*b)
    TR.assert_stage(rt.tape_sections_stage(*b, device=False), want, what + " (host)")
    got = rt.tape_sections_stage(*b, device=True)
    TR.assert_stage(got, want, what + " (device)")
    assert rt.verify_tapes_last()["launches"] <= 8
    return got


# ---- the kernels' edges: every designed batch of tests/tape_many_ref.py ---------------------------------------------------------------------------------------------------
# calls_012 / _210 / _102: calls255 | calls256 | calls257 in three orders (lanes of two proofs in one wave and one workgroup); one_call_x64: 64 one-call tapes, one wave;
# designed_l_dev: every length edge of the three functions beside the lanes' longest calls; no_predecessor; failing_between; lowest_wins; header_only; empty_and_not;
# wide_sizes (1, 255, 256, 257 records); wide_failing (a zero divisor and a bad opcode: 57 there only); ragged_chunks (hash sections of exactly 512, 513 and 1023 words)
@pytest.mark.parametrize("name", list(TR.designed_batches()))
def test_the_designed_batches(name):
    got = _three_ways(TR.designed_batches()[name], name)
    if name in TR.WANT_VERDICTS:
        assert (got[0], got[1]) == TR.WANT_VERDICTS[name]
    else:
        assert not any(got[0]) and not any(got[1])


def test_patches_land_in_their_proofs_cells():
    """designed | l_dev | max_len (three calls of 1 MiB: hashed on host threads, patched in before the sides) | designed: against the host stage (the Python sums of 400 000
    cells are out of a test's reach), and the pairs the reference can reach against the reference"""
    b = TR.batch([(D.tape("designed"), TR.EMPTY), (D.tape("l_dev"), TR.EMPTY), (D.tape("max_len"), TR.wide_of(3)), (D.tape("designed"), TR.EMPTY)], n_real=1 << 22, seed=12)
    host = rt.tape_sections_stage(*b, device=False)
    assert host[0] == [0, 0, 0, 0] and all(any(s[0]) for s in host[3])
    got = rt.tape_sections_stage(*b, device=True)
    TR.assert_stage(got, host, "designed | l_dev | max_len | designed")
    assert rt.verify_tapes_last()["launches"] == 8               # (two checks, digests, old and new bytes, the patch, two sides)
    for k in (0, 1, 3):
        one = tuple(x[k:k + 1] for x in b)
        TR.assert_stage(tuple(x[k:k + 1] for x in got), TR.stage_ref(*one), f"pair {k}")


def test_the_entrys_cap_of_one_call_sections():
    pairs = [(TR.one_call(k % 64, cycle=2 + k), TR.EMPTY) for k in range(1024)]
    b = TR.batch(pairs, seed=13)
    b = (b[0], b[1], b[2], b[3], [TR.challenge(i % 7) for i in range(1024)], [TR.challenge(7 + i % 5) for i in range(1024)])
    host = rt.tape_sections_stage(*b, device=False)
    assert not any(host[0])
    TR.assert_stage(rt.tape_sections_stage(*b, device=True), host)
    k = 1000                                                    # (the reference on one of them)
    TR.assert_stage(tuple(x[k:k + 1] for x in host), TR.stage_ref(*tuple(x[k:k + 1] for x in b)))
    with pytest.raises(rt.RuntimeError):
        rt.tape_sections_stage(*(x + x[:1] for x in b), device=True)


# ---- the entries ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_honest_mixed_batch_is_one_batch(monkeypatch):
    corpus = TR.honest_corpus()
    proofs, pubs = [p for _, p, _ in corpus], [e for _, _, e in corpus]
    want = [rt.verify(p, e) for p, e in zip(proofs, pubs)]
    assert want == [0] * len(proofs)
    records = sum(TR.records(p) for p in proofs)
    TH._in_orders(proofs, pubs, want, "honest")
    assert rt.verify_many(proofs, pubs, tapes=True) == want
    last = rt.verify_tapes_last()
    assert last["records"] == records and 0 < last["launches"] <= 8 and last["uploaded_words"] > 0
    assert rt.verify_memory_last()["launches"] == 3 and rt.verify_queries_last()["launches"] == 2
    # the same composition, 1, 2 and 7 times: the same launches — no per-proof launch can hide
    comp = [proofs[2], proofs[4]]                                # (blake3_multi_chunk: a patch; wide_and_hash: both tapes)
    counts = []
    for k in (1, 2, 7):
        assert rt.verify_many(comp * k, tapes=True) == [0, 0] * k
        counts.append(rt.verify_tapes_last()["launches"])
        assert rt.verify_tapes_last()["records"] == k * sum(TR.records(p) for p in comp)
    assert counts == [8, 8, 8], counts
    # every entry from before, and tapes=False: no tape batch
    for kw in ({}, {"memory": True}):
        assert rt.verify_many(proofs, pubs, **kw) == want and rt.verify_tapes_last() == NONE
    assert rt.verify(proofs[0], pubs[0], device=True) == 0 and rt.verify_tapes_last() == NONE
    # the threshold applies to the TOTAL: one record more keeps the whole batch with the fronts
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_RECORDS", str(records + 1))
    assert rt.verify_many(proofs, pubs, tapes=True) == want and rt.verify_tapes_last() == NONE
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_RECORDS", str(records))
    assert rt.verify_many(proofs, pubs, tapes=True) == want and rt.verify_tapes_last()["records"] == records


def test_mutated_and_forged_proofs_get_the_host_verdict():
    muts = TR.mutants()
    proofs = [t for _, t in muts]
    want = [rt.verify(t) for t in proofs]
    assert rt.verify_many(proofs, tapes=True) == want
    assert rt.verify_tapes_last()["launches"] <= 8 and rt.verify_memory_last()["launches"] == 3
    rng = np.random.default_rng(2)
    perm = [int(i) for i in rng.permutation(len(proofs))][:40]
    assert rt.verify_many([proofs[i] for i in perm], tapes=True) == [want[i] for i in perm]
    honest = [TR.oracle_mode4("sha256_hello")[0], TR.oracle_mode4("wide_and_hash")[0]]
    proofs, want = [], []
    for k, (case, pr, verdict) in enumerate(TR.forged()):
        proofs += [pr, honest[k % 2]]; want += [verdict, 0]
    TH._in_orders(proofs, None, want, "forged")


def test_rate_proofs_and_their_mutants():
    corpus = TR.rate_corpus()
    proofs, pubs = [c[1] for c in corpus], [c[2] for c in corpus]
    mq, mb = [c[3] for c in corpus], [c[4] for c in corpus]
    want = [rt.verify_rate(p, e, q, b) for p, e, q, b in zip(proofs, pubs, mq, mb)]
    assert set(want) - {0} == TR.RATE_MUTATION_CODES
    assert rt.verify_rate_many(proofs, pubs, mq, mb, tapes=True) == want
    last = rt.verify_tapes_last()
    assert last["records"] > 0 and 0 < last["launches"] <= 8
    rev = list(reversed(range(len(proofs))))
    assert rt.verify_rate_many([proofs[i] for i in rev], [pubs[i] for i in rev], [mq[i] for i in rev], [mb[i] for i in rev], tapes=True) == [want[i] for i in rev]
    p3, o3, _, _, q3, b3 = TR.RM.golden("mode3")
    assert rt.verify_rate_many([p3, proofs[0], p3], [TR.pub_c(o3), pubs[0], None], [q3, mq[0], q3], [b3, mb[0], b3], tapes=True) == [0, 0, 0]
    assert rt.verify_memory_last()["launches"] == 3
    assert rt.verify_rate_many(proofs, pubs, mq, mb, memory=True) == want and rt.verify_tapes_last() == NONE
    assert rt.verify_rate_many(proofs, pubs, mq, mb) == want and rt.verify_tapes_last() == NONE


def test_the_gpu_provers_proofs_with_an_array_loop_between_them():
    """the GPU prover's mode-4 proofs (tests/test_gpu_verify_device.py: _mode4_proof) with spec.memory_loop_program(300)'s mode-3 proof between them: the memory region
    and the tape region behind it must both survive the fronts for phase B"""
    from zkir_amd import pipeline as pl
    blob = spec.memory_loop_program(300).to_bytes()
    log = rt.interpret(blob, [], rt.VMConfig(enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    pub3 = rt.public_inputs(log, blob, [], mem_mode=True, mem_witness="device")
    ctx = stark.StarkContext(stark.padded_log_n(log.n_rows))
    p3 = stark.prove(ctx, tr, pub3)
    ctx.close()
    log.close()
    m4 = [tv._mode4_proof(name) for name in ("sha256_hello", "wide_and_hash", "hash_edge_calls", "sha_chain_2p12")]
    proofs = [m4[0][0], m4[1][0], p3, m4[2][0], p3, m4[3][0]]
    pubs = [m4[0][1], m4[1][1], pub3, m4[2][1], pub3, m4[3][1]]
    assert rt.verify_many(proofs, pubs, tapes=True) == [0] * 6
    assert rt.verify_tapes_last()["records"] == sum(TR.records(p) for p in proofs) and rt.verify_tapes_last()["launches"] <= 8
    assert rt.verify_memory_last()["launches"] == 3 and rt.verify_queries_last()["launches"] == 2
    lay = stark.proof_layout(proofs[5])
    t = proofs[5].copy(); t[lay["hash_section"] + 1 + 8 + 1] ^= 1      # a byte of the chain's first touched cell, in the LAST proof
    want = rt.verify(t, pubs[5])
    assert want != 0 and rt.verify_many(proofs[:5] + [t], pubs, tapes=True) == [0] * 5 + [want]
    t3 = p3.copy(); t3[stark.proof_layout(p3)["mem_section"] + 1 + 7 * 299 + 2] ^= 1
    want3 = rt.verify(t3, pub3)
    assert want3 != 0 and rt.verify_many(proofs[:4] + [t3, proofs[5]], pubs, tapes=True) == [0] * 4 + [want3, 0]


def test_the_probe_on_the_device():
    TH._probe_checks(device=True)
