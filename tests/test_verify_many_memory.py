"""The memory stages over a LIST of proofs, without a GPU: the host list stage (zkir_mem_sections_stage_host) against the Python reference, and the orchestration the device
entries share — the section locator, phase A before any front, fronts that DEFER check 10, phase B, the resolution — through zkir_verify_many_memory_host /
zkir_verify_rate_many_memory_host and the probe's host form: every verdict is the single-proof host verifier's."""
import numpy as np
import pytest

import mem_many_ref as MR
import mem_stage_ref as M
import test_gpu_verify_memory_device as tm
from zkir_amd import runtime as rt, stark


# ---- the host list stage -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", range(len(MR.SIZES_ORDERS)))
def test_the_host_list_stage_gives_the_reference(order):
    b = MR.batch(MR.sizes_sections(MR.SIZES_ORDERS[order]), seed=order)
    MR.assert_stage(rt.mem_sections_stage(*b, device=False), MR.stage_ref(*b))


def edge_batch():
    """the image's edges (tests/mem_stage_ref.py: side_cases) three times, each section with ANOTHER image; no code segment, so the cells on the code pass the check"""
    _, edge, blob, _, _ = M.side_cases()[0]
    other = M.make_blob(blob[32:52], bytes(reversed(blob[52:])))
    secs, modes, code_words, _, alphas, lams = MR.batch([edge, edge, edge], seed=9)
    return secs, modes, [0, 0, 0], [blob, blob[:31], other], alphas, lams


def failing_batch():
    """well-formed and failing sections side by side: a failing cell in one section leaves its neighbours at 0, and a section whose FIRST address lies below its
    predecessor's last one passes (cell 0 has no predecessor)"""
    high, low = M.increasing(40, seed=1, start=1 << 30), M.increasing(40, seed=2, start=0x2000)
    bad54 = [list(c) for c in low]; bad54[0][3] = 0x10000
    on_code = M.cells_at([0xFF8, 0x1000, 0x2000])
    return MR.batch([M.section(high), M.section(low), M.section(bad54), M.section(high), M.section(on_code), M.section(low)], seed=5)


def test_the_host_list_stage_keeps_sections_apart():
    b = edge_batch()
    want = MR.stage_ref(*b)
    assert want[2][0] != want[2][1] != want[2][2]               # (the images differ, so the sums do)
    MR.assert_stage(rt.mem_sections_stage(*b, device=False), want)
    b = failing_batch()
    want = MR.stage_ref(*b)
    assert want[0] == [0, 0, 54, 0, 55, 0]
    MR.assert_stage(rt.mem_sections_stage(*b, device=False), want)


def test_the_list_stage_refuses_what_is_not_a_list_of_whole_sections():
    secs, modes, code_words, blobs, alphas, lams = MR.batch(MR.sizes_sections([1, 2]))
    with pytest.raises(rt.RuntimeError):
        rt.mem_sections_stage([secs[0], secs[1][:-1]], modes, code_words, blobs, alphas, lams, device=False)
    with pytest.raises(rt.RuntimeError):
        rt.mem_sections_stage(secs, [3, 2], code_words, blobs, alphas, lams, device=False)
    with pytest.raises(rt.RuntimeError):
        rt.mem_sections_stage([], [], [], [], [], [], device=False)


# ---- the orchestration over the host stages ------------------------------------------------------------------------------------------------------------------------------
def test_honest_proofs_of_every_mode_in_one_batch():
    corpus = MR.honest_corpus()
    proofs, pubs = [p for _, p, _ in corpus], [e for _, _, e in corpus]
    want = [rt.verify(p, e) for p, e in zip(proofs, pubs)]
    assert want == [0, 0, 55, 0, 0, 0, 0, 0, 0], list(zip([w for w, _, _ in corpus], want))
    assert rt.verify_many(proofs, pubs, memory=True, device=False) == want
    # THE LOCATOR: every located section went through the list stage — the reported cells are the sum of the count words (a front whose arguments differed from the
    # located ones would have taken the host stage all the same, so only this count shows the routing)
    assert rt.verify_memory_last() == {"cells": sum(MR.count_word(p) for p in proofs), "launches": 0, "uploaded_words": 0}
    assert rt.verify_many(proofs, None, memory=True, device=False) == [rt.verify(p) for p in proofs]
    for k in (1, 4):                                            # (one proof; a batch without the refused one)
        assert rt.verify_many(proofs[k:k + 1], pubs[k:k + 1], memory=True, device=False) == want[k:k + 1]
        assert rt.verify_memory_last()["cells"] == MR.count_word(proofs[k])
    # expectations that do not match fail check 6 before the memory stage is consulted
    assert rt.verify_many(proofs[:2], [pubs[1], pubs[0]], memory=True, device=False) == [rt.verify(proofs[0], pubs[1]), rt.verify(proofs[1], pubs[0])]
    assert rt.verify(proofs[0], pubs[0]) == 0 and rt.verify_memory_last()["cells"] == 0      # (any other entry: no record)


def test_mutated_proofs_get_the_host_verdict_in_any_order():
    muts = MR.mutants()
    proofs = [t for _, t in muts]
    want = [rt.verify(t) for t in proofs]
    assert want[0] == 0 and all(w != 0 for w in want[1:]) and set(want[1:]) == tm.MUTATION_CODES
    assert rt.verify_many(proofs, memory=True, device=False) == want
    rng = np.random.default_rng(2)
    for _ in range(2):
        perm = [int(i) for i in rng.permutation(len(proofs))]
        got = rt.verify_many([proofs[i] for i in perm[:40]], memory=True, device=False)
        assert got == [want[i] for i in perm[:40]]


def test_rate_proofs_and_their_mutants():
    corpus = MR.rate_corpus()
    proofs, pubs = [c[1] for c in corpus], [c[2] for c in corpus]
    mq, mb = [c[3] for c in corpus], [c[4] for c in corpus]
    want = [rt.verify_rate(p, e, q, b) for p, e, q, b in zip(proofs, pubs, mq, mb)]
    honest = [i for i, c in enumerate(corpus) if c[0].endswith("honest")]
    assert len(honest) == 2 and all(want[i] == 0 for i in honest) and all(w != 0 for i, w in enumerate(want) if i not in honest)
    assert set(want) - {0} == MR.RATE_MUTATION_CODES, set(want)
    assert rt.verify_rate_many(proofs, pubs, mq, mb, memory=True, device=False) == want
    assert rt.verify_memory_last()["cells"] == sum(MR.located_cells(c[1], c[5]) for c in corpus)
    rev = list(reversed(range(len(proofs))))
    assert rt.verify_rate_many([proofs[i] for i in rev], [pubs[i] for i in rev], [mq[i] for i in rev], [mb[i] for i in rev], memory=True, device=False) == [want[i] for i in rev]
    # the caller's floors are checked per proof (2), before anything else
    assert rt.verify_rate_many(proofs[:1], pubs[:1], [mq[0] + 1], mb[:1], memory=True, device=False) == [2]


# ---- the probe: a perturbed share reaches the deferred check 10 ----------------------------------------------------------------------------------------------------------
def probe_cases():
    """[(what, proof, the host verdict, the verdict with the proof's share perturbed)]: 10 where the front deferred — also where it failed a LATER check — and the host
    verdict where it failed before check 10 (then nothing was deferred)"""
    muts = MR.mutants()
    honest = muts[0][1]
    lay = stark.proof_layout(honest)
    out, seen = [("honest", honest, 0, 10)], set()
    for what, t in muts[1:]:
        host = rt.verify(t)
        if host in seen or host == 4:
            continue
        seen.add(host)
        assert host in {3, 8, 12, 54, 55, 21, 22, 23, 27}, host
        out.append((what, t, host, 10 if host >= 20 and host < 30 else host))
    assert {8, 12, 54, 55} <= seen and seen & {21, 22, 23, 27}, seen
    cut = honest[:-1]                                           # the last query is cut: the front reaches the queries, the stage (4) or the length check (30) fails
    host = rt.verify(cut)
    assert host in (4, 30), host
    out.append(("the last word cut", cut, host, 10))
    out.append(("cut in front of the section", honest[:lay["mem_section"]], 4, 4))
    return out


def _probe_checks(device):
    corpus = MR.honest_corpus()
    proofs, pubs = [p for _, p, _ in corpus], [e for _, _, e in corpus]
    want = [rt.verify(p, e) for p, e in zip(proofs, pubs)]
    assert rt.verify_many(proofs, pubs, memory=True, device=device, probe=(0, 0)) == want
    for i, p in enumerate(proofs):
        deferred = want[i] == 0 and MR.count_word(p) > 0       # (the refused proof fails check 55 first; fib30's have no cell to defer for)
        got = rt.verify_many(proofs, pubs, memory=True, device=device, probe=(1, i))
        assert got == [10 if (j == i and deferred) else w for j, w in enumerate(want)], (corpus[i][0], got)
    cases = probe_cases()
    batch = [t for _, t, _, _ in cases]
    assert rt.verify_many(batch, memory=True, device=device, probe=(0, 0)) == [h for _, _, h, _ in cases]
    for i, (what, t, host, perturbed) in enumerate(cases):
        got = rt.verify_many(batch, memory=True, device=device, probe=(1, i))
        assert got == [perturbed if j == i else c[2] for j, c in enumerate(cases)], (what, got)
    with pytest.raises(rt.RuntimeError):
        rt.verify_many(batch, memory=True, device=device, probe=(1, len(batch)))
    with pytest.raises(rt.RuntimeError):
        rt.verify_many(batch, memory=True, device=device, probe=(2, 0))


def test_the_probe_reaches_the_deferred_check():
    _probe_checks(device=False)


def test_the_entries_refuse_an_empty_list_and_too_many():
    p = MR.honest_corpus()[0][1]
    for bad in ([], [p] * 1025):
        with pytest.raises(rt.RuntimeError):
            rt.verify_many(bad, memory=True, device=False)
        with pytest.raises(rt.RuntimeError):
            rt.verify_rate_many(bad, memory=True, device=False)
