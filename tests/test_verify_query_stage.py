"""The STARK verifier's query stage behind its interface (verify_stages.h: StarkQueries, StarkQueryStage), host form.  zkir_stark_query_stage_probe runs the verifier's
host part on an honest proof, perturbs what the VERIFIER drew and runs the stage: that reaches checks 24, 25 and 26, which no single-word mutation of a proof can (the
roots are in the transcript), and pins the wiring of the description — a swapped exponent, or zeta and zeta w exchanged, turns the unperturbed run into 24.  The host
entries' verdicts on the mutation lists of tests/test_gpu_verify_queries_device.py are compared with the oracle's verifier, an independent implementation.  No GPU."""
import pytest

import stark_query_cases as sq
from oracle import stark_api as so
from zkir_amd import runtime as rt


@pytest.mark.parametrize("mode,log_n", [(0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (1, 4), (2, 5), (3, 6), (4, 7)])
def test_the_host_stage_on_honest_proofs_and_perturbed_draws(mode, log_n):
    proof, _ = sq.oracle_proof(mode, log_n)
    n_layers, nq = len(sq.SCHEDULES[log_n]), int(proof[4])
    assert rt.stark_query_stage_probe(proof, 0) == 0 == rt.verify(proof)
    for what in (1, 2, 3):                                        # a0, b0, zeta: the layer-0 value
        assert rt.stark_query_stage_probe(proof, what) == 24, what
    for j in range(n_layers):                                     # beta_j: the value carried into layer j + 1, or into the final layer
        assert rt.stark_query_stage_probe(proof, 4, j) == (25 if j < n_layers - 1 else 26), j
    for t in (0, nq // 2, nq - 1):                                # a sample: the proof's index word is no longer it
        assert rt.stark_query_stage_probe(proof, 5, t) == 20, t
    assert rt.verify_queries_last() == {"hash_jobs": 0, "value_jobs": 0, "launches": 0, "uploaded_words": 0}


def test_the_probe_refuses_what_it_cannot_perturb():
    proof, _ = sq.oracle_proof(0, 3)
    for what, index in ((6, 0), (4, 1), (5, 50)):
        with pytest.raises(rt.RuntimeError):
            rt.stark_query_stage_probe(proof, what, index)
    assert rt.stark_query_stage_probe(proof[:100], 0) == rt.verify(proof[:100]) != 0      # (a proof that fails before its queries: the host part's code)


def _host_and_oracle_agree(muts):
    codes = set()
    for what, t in muts:
        host = rt.verify(t)
        assert host != 0, ("a mutated proof was accepted", what)
        assert host == so.verify(t), ("the host verifier and the oracle disagree", what)
        codes.add(host)
    return codes


@pytest.mark.parametrize("chunk", range(sq.BUMP_CHUNKS))
@pytest.mark.parametrize("t", [0, -1])
@pytest.mark.parametrize("mode,log_n", sq.MUTANT_PROOFS)
def test_host_verdicts_on_bumped_query_words_are_the_oracles(mode, log_n, t, chunk):
    proof, pub = sq.oracle_proof(mode, log_n)
    _host_and_oracle_agree(sq.query_bumps(proof, t, chunk))


@pytest.mark.parametrize("mode,log_n", sq.MUTANT_PROOFS)
def test_host_verdicts_on_roots_cuts_and_a_trailing_word_are_the_oracles(mode, log_n):
    proof, pub = sq.oracle_proof(mode, log_n)
    assert rt.verify(proof, pub) == 0 == so.verify(proof)
    codes = _host_and_oracle_agree(sq.record_bumps(proof, 0) + sq.record_bumps(proof, -1) + sq.other_mutants(proof))
    assert sq.WANTED_CODES <= codes, codes                        # (a condition on the inputs: the lists reach every check of a query)


@pytest.mark.parametrize("n_total,seg", [(300, 128), (65, 33)])
def test_host_chain_verdicts_are_the_oracles(n_total, seg):
    seen = {}
    for what, proofs, expect in sq.chain_cases(n_total, seg):
        host = rt.verify_chain(proofs, expect)
        o_expect = None
        if expect is not None:
            o_expect = so.PublicC(expect.n_real, expect.deferred, expect.fri_params, expect.entry_point)
            o_expect.prog[:] = list(expect.program_digest); o_expect.io[:] = list(expect.io_digest)
        assert host == so.verify_chain(proofs, o_expect), what
        seen[what] = host
    n = len(sq.segments(n_total, seg)[1])
    assert seen["honest"] == seen["honest, no expect"] == 0 and seen["first dropped"] == 41 and seen["swapped"] in (41, 42)
    assert seen["wrong row count"] == 44 and seen["wrong program"] == 43
    assert [seen[f"row word of segment {i}"] for i in range(n)] == [1000 * (i + 1) + 21 for i in range(n)]
    assert seen["header of segment 1, query of segment 0"] == 1000 + 27      # the lower segment's code wins
    if (n_total, seg) == (300, 128):
        assert [int(p[2]) for p in sq.segments(n_total, seg)[1]] == [7, 7, 6]
