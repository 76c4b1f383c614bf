"""zkir_verify_rate_segment and zkir_verify_rate_chain without a GPU, against tests/rate_chain_ref.py: a 64-cycle run proven by the reference 'ZKSR' prover in three
segments at blow-up 2, 4 and 8 (modes 0 and 1; cuts with log_n 4, 5, 5 and with a one-row tail at log_n 3) is accepted as ONE run; every segment is accepted on its own
and hands out its header's states, while zkir_verify_rate refuses the ones that do not start the run (7); wrong chains, damaged segments and about 150 single-word
mutants get the reference's code."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import batch_eval_ref as be
import prove_rate_ref as pr
import rate_chain_ref as rc
from oracle import api as oracle, stark_api as so
from zkir_amd import runtime as rt, spec

P = pr.P
N_RUN, NQ = 64, 3
CUTS = {"A": [(0, 9), (8, 40), (39, 64)], "B": [(0, 33), (32, 64), (63, 64)]}       # log_n 4, 5, 5; 6, 5 and the one-row tail at log_n 3
BITS = {"A": 0, "B": 4}
CHAINS = [(mode, cuts, b) for mode in (0, 1) for cuts in ("A", "B") for b in (1, 2, 3)]
IDS = [f"mode{m}-cuts{c}-b{b}" for m, c, b in CHAINS]


def pub_c(p: so.PublicC) -> rt.PublicInputsC:
    out = rt.PublicInputsC(p.n_real, p.entry, p.deferred, 0)
    out.program_digest[:] = list(p.prog); out.io_digest[:] = list(p.io)
    return out


@functools.lru_cache(maxsize=None)
def run(mode: int):
    blob = spec.fib_endless_program().to_bytes()
    cfg = {"enable_deferred_model": True} if mode else {}
    res = oracle.run(blob, max_cycles=N_RUN, enable_execution_trace=True, **cfg)
    assert len(res.rows) == N_RUN
    return res.rows, so.public_inputs(N_RUN, blob, [], list(res.outputs), (res.halt_kind, res.halt_code), deferred=bool(mode))


@functools.lru_cache(maxsize=None)
def segment(mode: int, a: int, e: int, b: int, nq: int, bits: int):
    rows, run_pub = run(mode)
    proof = pr.prove_ref(rows[a:e], rc.segment_pub(run_pub, a, e), b, nq, bits)
    proof.setflags(write=False)
    return proof


@functools.lru_cache(maxsize=None)
def chain(mode: int, cuts: str, b: int):
    return [segment(mode, a, e, b, NQ, BITS[cuts]) for a, e in CUTS[cuts]]


def both(proofs, expect, honests, min_q=1, min_bits=0) -> int:
    """the product's verdict on a chain, which must be the reference's"""
    got = rt.verify_rate_chain(proofs, pub_c(expect) if expect is not None else None, min_q, min_bits)
    want = rc.verify_chain_ref(proofs, expect, min_q, min_bits, honests)
    assert got == want, f"zkir_verify_rate_chain says {got}, the reference {want}"
    return got


def test_the_entries_exist():
    L = rt.lib()
    assert all(hasattr(L, n) for n in ("zkir_verify_rate_segment", "zkir_verify_rate_chain"))


@pytest.mark.parametrize("case", CHAINS, ids=IDS)
def test_chain_is_accepted_and_its_segments_stand_alone(case):
    mode, cuts, b = case
    proofs = chain(*case)
    _, run_pub = run(mode)
    bits = BITS[cuts]
    assert [int(p[2]) for p in proofs] == ([4, 5, 5] if cuts == "A" else [6, 5, 3])
    assert both(proofs, run_pub, proofs) == 0 and both(proofs, None, proofs) == 0 and both(proofs, run_pub, proofs, NQ, bits) == 0
    for i, (p, (a, e)) in enumerate(zip(proofs, CUTS[cuts])):
        seg_pub = rc.segment_pub(run_pub, a, e)
        for expect in (None, seg_pub):
            code, first, last = rt.verify_rate_segment(p, pub_c(expect) if expect is not None else None, NQ, bits)
            assert code == 0 == rc.verify_segment_ref(p, expect, NQ, bits, p)
            assert np.array_equal(first, p[21:21 + 68]) and np.array_equal(last, p[21 + 68:21 + 136])
        # the whole-run verifier accepts the segment that starts the run and refuses the others at check 7, as the reference does
        want = 0 if i == 0 else 7
        assert rt.verify_rate(p, None, 1, 0) == want == pr.verify_ref(p, None, 1, 0, p)
        if i:
            assert np.array_equal(p[21:21 + 68], proofs[i - 1][21 + 68:21 + 136])          # header words 21 .. 157 link
    # one more query or bit than the segments state: every segment fails check 2, the first one decides
    assert both(proofs, run_pub, proofs, min_q=NQ + 1) == 1002 and both(proofs, run_pub, proofs, min_bits=bits + 1) == 1002
    # a segment under another segment's expectation
    assert rt.verify_rate_segment(proofs[1], pub_c(rc.segment_pub(run_pub, *CUTS[cuts][0])), 1, 0)[0] == 6


@pytest.mark.parametrize("mode,cuts,b", [(0, "A", 2), (1, "B", 3), (0, "B", 1)])
def test_wrong_chains_get_the_reference_code(mode, cuts, b):
    s = chain(mode, cuts, b)
    _, run_pub = run(mode)
    (a1, e1), bits = CUTS[cuts][1], BITS[cuts]
    assert rt.verify_rate_chain([], None) == 40 == rc.verify_chain_ref([], None, 1, 0, [])
    assert both(s[1:], None, s[1:]) == 41                                           # the first segment dropped
    assert both([s[0], s[2]], None, [s[0], s[2]]) == 42                             # a gap
    assert both([s[0], s[1], s[1]], None, [s[0], s[1], s[1]]) == 42                 # a repeat
    for other in (segment(mode, a1, e1, b % 3 + 1, NQ, bits),                        # a segment of another rate
                  segment(mode, a1, e1, b, NQ + 1, bits),                            # of another query count
                  segment(mode, a1, e1, b, NQ, bits + 1),                            # of another grinding
                  segment(1 - mode, a1, e1, b, NQ, bits)):                           # of the other mode
        t = [s[0], other, s[2]]
        assert both(t, run_pub, t) == 43
    # not the expected run; a wrong total
    o = run_pub.clone(); o.entry += 4
    assert both(s, o, s) == 43
    o = run_pub.clone(); o.io[0] = (o.io[0] + 1) % P
    assert both(s, o, s) == 43
    for total in (N_RUN - 1, N_RUN + 1, N_RUN + 2):
        o = run_pub.clone(); o.n_real = total
        assert both(s, o, s) == 44
    # a damaged segment 0, 1, 2: a record word of its first query, a layer value of its last
    for i in range(3):
        at = pr.layout(s[i])["eval_proof"]
        ia = be.layout(s[i][at:])
        for pos, want in ((at + ia["queries"] + ia["records"][0][0], 107), (at + ia["queries"] + (ia["num_queries"] - 1) * ia["qsize"] + ia["layers"][0][0], 108)):
            t = [p.copy() for p in s]
            t[i][pos] = (int(t[i][pos]) + 1) % P
            assert both(t, run_pub, s) == 1000 * (i + 1) + want
        t = [p.copy() for p in s]
        t[i] = t[i][:-1]
        assert both(t, run_pub, s) == 1000 * (i + 1) + 101
    # two damaged segments: the first one decides; a damaged segment in front of a chain fault decides too
    t = [s[0].copy(), s[2].copy(), s[2].copy()]
    t[0][-1] = (int(t[0][-1]) + 1) % P; t[2][5] = 7
    assert both(t, None, [s[0], s[2], s[2]]) // 1000 == 1


@pytest.mark.parametrize("mode,cuts,b", [(0, "A", 2), (1, "B", 1)])
def test_single_word_mutants_get_the_reference_code(mode, cuts, b):
    """about 150 mutants across the chain: word `pos` of segment k becomes (w + 1 + r) mod p, r drawn — never the word it was"""
    s = chain(mode, cuts, b)
    _, run_pub = run(mode)
    rng = np.random.default_rng(1000 * mode + b)
    picks = []
    for k in range(3):
        at = pr.layout(s[k])
        ev = at["eval_proof"]
        ia = be.layout(s[k][ev:])
        fixed = list(range(13)) + [13, 17, 21, 22, 21 + 68, 21 + 135, at["program"], at["program"] + 3, at["rom_mult"], at["rc_mult"] + 2, at["trace_root"], at["aux_root"] + 1,
                                   at["quotient_root"] + 2, ev, ev + 3, ev + 6, ev + ia["roots"], ev + ia["points"] + 1, ev + ia["evals"], ev + ia["layer_roots"], ev + ia["final"],
                                   ev + ia["nonce"], ev + ia["queries"], len(s[k]) - 1]
        picks += [(k, p) for p in fixed] + [(k, int(p)) for p in rng.integers(0, len(s[k]), 14)]
    assert 140 <= len(picks) <= 170
    seen = {}
    for k, pos in picks:
        t = [p.copy() for p in s]
        t[k][pos] = (int(t[k][pos]) + 1 + int(rng.integers(0, 1000))) % P
        assert t[k][pos] != s[k][pos]
        code = both(t, run_pub, s)
        assert code != 0, f"segment {k} word {pos}: accepted"
        seen.setdefault(code, (k, pos))
    assert {c // 1000 for c in seen} >= {1, 2, 3} and {c % 1000 for c in seen} >= {1, 2, 8, 10}, sorted(seen)


def test_a_chain_of_one_mode3_proof_is_the_whole_run_verifier():
    from test_prove_rate_modes_verify import golden
    golden_pub = pub_c
    proof, opub, _, b, nq, bits = golden("mode3")
    assert rt.verify_rate_chain([proof], golden_pub(opub), nq, bits) == rt.verify_rate(proof, golden_pub(opub), nq, bits) == 0
    t = proof.copy(); t[len(t) - 1] = (int(t[-1]) + 1) % P
    assert rt.verify_rate_chain([t], None) == rt.verify_rate(t, None, 1, 0) != 0
    assert rt.verify_rate_chain([proof], None, nq + 1, 0) == 2
    # such a proof is never a segment, alone or in a longer chain
    assert rt.verify_rate_segment(proof)[0] == 2 and rt.verify_rate_chain([proof, proof]) == 1002
