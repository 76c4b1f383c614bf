"""A mode-4 proof's tape stages over a LIST of proofs, without a GPU: the host list stage (zkir_tape_sections_stage_host) against the Python reference, and the
orchestration the device entries share — both locators, phase A before any front, fronts that DEFER check 10 for their tapes, their cells or both, phase B, the
resolution — through zkir_verify_many_tapes_host / zkir_verify_rate_many_tapes_host and the probe's host form: every verdict is the single-proof host verifier's."""
import numpy as np
import pytest

import tape_many_ref as TR
import test_gpu_verify_device as tv
from zkir_amd import runtime as rt, stark


# ---- the host list stage -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TR.designed_batches()))
def test_the_host_list_stage_gives_the_reference(name):
    b = TR.designed_batches()[name]
    want = TR.stage_ref(*b)
    if name in TR.WANT_VERDICTS:
        assert (want[0], want[1]) == TR.WANT_VERDICTS[name]
    else:
        assert not any(want[0]) and not any(want[1]), (want[0], want[1])
    TR.assert_stage(rt.tape_sections_stage(*b, device=False), want, name)


def test_the_list_stage_refuses_what_is_not_a_list_of_whole_sections():
    hs, ws, nr, ce, al, la = TR.batch([(TR.one_call(0), TR.wide_of(2)), (TR.one_call(1), TR.EMPTY)])
    with pytest.raises(rt.RuntimeError):                        # words behind the last record
        rt.tape_sections_stage([np.concatenate([hs[0], [0]]), hs[1]], ws, nr, ce, al, la, device=False)
    with pytest.raises(rt.RuntimeError):                        # a wide section that is not [n] + 8 n words
        rt.tape_sections_stage(hs, [ws[0][:-1], ws[1]], nr, ce, al, la, device=False)
    with pytest.raises(rt.RuntimeError):
        rt.tape_sections_stage(hs, ws, nr, ce, [al[0], [TR.P, 0, 0, 0]], la, device=False)
    with pytest.raises(rt.RuntimeError):
        rt.tape_sections_stage([], [], [], [], [], [], device=False)
    # a wide count above n_real is 57, as the front answers it before its stage is asked
    got = rt.tape_sections_stage(hs, ws, [1, nr[1]], ce, al, la, device=False)
    assert got[0] == [56, 0] and got[1] == [57, 0]


# ---- the orchestration over the host stages ------------------------------------------------------------------------------------------------------------------------------
def _in_orders(proofs, pubs, want, what, **kw):
    n = len(proofs)
    rng = np.random.default_rng(3)
    for order in (list(range(n)), list(reversed(range(n))), [int(i) for i in rng.permutation(n)]):
        got = rt.verify_many([proofs[i] for i in order], [pubs[i] for i in order] if pubs is not None else None, tapes=True, **kw)
        assert got == [want[i] for i in order], (what, order, got)


def test_honest_proofs_of_every_mode_in_one_batch():
    corpus = TR.honest_corpus()
    proofs, pubs = [p for _, p, _ in corpus], [e for _, _, e in corpus]
    want = [rt.verify(p, e) for p, e in zip(proofs, pubs)]
    assert want == [0] * len(corpus), list(zip([w for w, _, _ in corpus], want))
    lay = stark.proof_layout(proofs[2])                          # (blake3_multi_chunk: a call above 1024 bytes, so a patch on the device)
    assert max(int(proofs[2][at + 3]) for at in [lay["hash_section"] + o for o in TR.offsets(proofs[2][lay["hash_section"]:lay["wide_section"]])]) > 1024
    assert TR.records(proofs[3]) > 0 and int(proofs[3][stark.proof_layout(proofs[3])["wide_section"]]) > 0      # (wide arithmetic)
    _in_orders(proofs, pubs, want, "honest", device=False)
    # THE LOCATORS: every located pair of tapes that holds a record went through the list stage, and every located section through the memory one
    assert rt.verify_many(proofs, pubs, tapes=True, device=False) == want
    assert rt.verify_tapes_last() == {"records": sum(TR.records(p) for p in proofs), "launches": 0, "uploaded_words": 0}
    assert rt.verify_memory_last()["cells"] > 0
    assert rt.verify_many(proofs, None, tapes=True, device=False) == [rt.verify(p) for p in proofs]
    for k in (0, 3, 7):                                          # (one proof)
        assert rt.verify_many(proofs[k:k + 1], pubs[k:k + 1], tapes=True, device=False) == want[k:k + 1]
        assert rt.verify_tapes_last()["records"] == TR.records(proofs[k])
    # expectations that do not match fail check 6 before any stage is consulted
    assert rt.verify_many(proofs[:2], [pubs[1], pubs[0]], tapes=True, device=False) == [rt.verify(proofs[0], pubs[1]), rt.verify(proofs[1], pubs[0])]
    # every entry from before, and tapes=False: no record
    assert rt.verify_many(proofs, pubs, memory=True, device=False) == want and rt.verify_tapes_last()["records"] == 0
    assert rt.verify(proofs[0], pubs[0]) == 0 and rt.verify_tapes_last()["records"] == 0


def test_mutated_proofs_get_the_host_verdict_in_any_order():
    muts = TR.mutants()
    proofs = [t for _, t in muts]
    want = [rt.verify(t) for t in proofs]
    assert want[0] == 0 and all(w != 0 for w in want[1:]) and {4, 10, 56, 57} <= set(want[1:])
    assert rt.verify_many(proofs, tapes=True, device=False) == want
    rng = np.random.default_rng(2)
    for _ in range(2):
        perm = [int(i) for i in rng.permutation(len(proofs))]
        got = rt.verify_many([proofs[i] for i in perm[:40]], tapes=True, device=False)
        assert got == [want[i] for i in perm[:40]]


def test_forged_hash_tapes_between_honest_proofs():
    forged = TR.forged()
    honest = [TR.oracle_mode4("sha256_hello")[0], TR.oracle_mode4("wide_and_hash")[0]]
    proofs, want = [], []
    for k, (case, pr, verdict) in enumerate(forged):
        assert rt.verify(pr) == verdict == tv.FORGED[case], case
        proofs += [pr, honest[k % 2]]; want += [verdict, 0]
    assert sum(1 for w in want if w == 10) == 5                  # (five of them reach check 10 through the tape's share alone)
    _in_orders(proofs, None, want, "forged", device=False)


def test_rate_proofs_and_their_mutants():
    corpus = TR.rate_corpus()
    proofs, pubs = [c[1] for c in corpus], [c[2] for c in corpus]
    mq, mb = [c[3] for c in corpus], [c[4] for c in corpus]
    want = [rt.verify_rate(p, e, q, b) for p, e, q, b in zip(proofs, pubs, mq, mb)]
    assert want[0] == 0 and all(w != 0 for w in want[1:])
    assert set(want) - {0} == TR.RATE_MUTATION_CODES, set(want)
    n = len(proofs)
    rng = np.random.default_rng(4)
    for order in (list(range(n)), list(reversed(range(n))), [int(i) for i in rng.permutation(n)]):
        got = rt.verify_rate_many([proofs[i] for i in order], [pubs[i] for i in order], [mq[i] for i in order], [mb[i] for i in order], tapes=True, device=False)
        assert got == [want[i] for i in order], order
    assert rt.verify_tapes_last()["records"] > 0
    # the caller's floors are checked per proof (2), before anything else
    assert rt.verify_rate_many(proofs[:1], pubs[:1], [mq[0] + 1], mb[:1], tapes=True, device=False) == [2]
    # a mode-3 'ZKSR' proof beside it: the memory list stage and the tape list stage around one pass of fronts
    p3, o3, _, _, q3, b3 = TR.RM.golden("mode3")
    assert rt.verify_rate_many([p3, proofs[0], p3], [TR.pub_c(o3), pubs[0], None], [q3, mq[0], q3], [b3, mb[0], b3], tapes=True, device=False) == [0, 0, 0]


# ---- the probe: a perturbed share reaches the deferred check 10 ----------------------------------------------------------------------------------------------------------
def _probe_checks(device):
    corpus = TR.honest_corpus()
    proofs, pubs = [p for _, p, _ in corpus], [e for _, _, e in corpus]
    want = [0] * len(proofs)
    assert rt.verify_many(proofs, pubs, tapes=True, device=device, probe=(0, 0)) == want
    for i, p in enumerate(proofs):
        lay = stark.proof_layout(p) if int(p[9]) == 4 else None
        has = [bool(lay and int(p[lay["hash_section"]])), bool(lay and int(p[lay["wide_section"]]))]
        for what in (1, 2):                                     # (an honest batch is unchanged by a probe on a proof whose tape is empty, or that has none)
            got = rt.verify_many(proofs, pubs, tapes=True, device=device, probe=(what, i))
            assert got == [10 if (j == i and has[what - 1]) else 0 for j in range(len(proofs))], (corpus[i][0], what, got)
    # a front that fails BEFORE check 10 deferred nothing; one that fails behind it (a cut query) did
    honest = TR.mutants()[0][1]
    lay = stark.proof_layout(honest)
    cut = honest[:-1]
    host = rt.verify(cut)
    assert host in (4, 30)
    early = honest.copy(); early[lay["hash_section"] + 1 + 6] = 4      # (call 0's kind: 56)
    assert rt.verify(early) == 56
    batch = [honest, cut, early, honest[:lay["hash_section"]]]
    base = [0, host, 56, 4]
    assert rt.verify_many(batch, tapes=True, device=device, probe=(0, 0)) == base
    for i, perturbed in enumerate([10, 10, 56, 4]):
        got = rt.verify_many(batch, tapes=True, device=device, probe=(1, i))
        assert got == [perturbed if j == i else b for j, b in enumerate(base)], (i, got)
    with pytest.raises(rt.RuntimeError):
        rt.verify_many(batch, tapes=True, device=device, probe=(1, len(batch)))
    with pytest.raises(rt.RuntimeError):
        rt.verify_many(batch, tapes=True, device=device, probe=(3, 0))


def test_the_probe_reaches_the_deferred_check():
    _probe_checks(device=False)


def test_the_entries_refuse_an_empty_list_and_too_many():
    p = TR.honest_corpus()[0][1]
    for bad in ([], [p] * 1025):
        with pytest.raises(rt.RuntimeError):
            rt.verify_many(bad, tapes=True, device=False)
        with pytest.raises(rt.RuntimeError):
            rt.verify_rate_many(bad, tapes=True, device=False)
