"""zkir_verify_rate without a GPU, against tests/prove_rate_ref.py: reference 'ZKSR' proofs of fib runs at blow-up 2, 4 and 8 in modes 0 and 1 are accepted; the reference
quotient is of low degree at every rate and agrees across rates; mutants of every section, truncations and extensions get the reference verifier's code."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import batch_eval_ref as be
import lowdeg_ref as ld
import prove_rate_ref as pr
from oracle import api as oracle, stark_api as so
from zkir_amd import runtime as rt, spec

P = ld.P
# (n_real, b, mode, num_queries, pow_bits): log_n 3 and 6, every rate, both modes; small parameters keep the Python grinding and FRI in seconds
CASES = [(5, 1, 0, 3, 0), (5, 2, 1, 4, 4), (5, 3, 0, 5, 0), (64, 1, 1, 6, 4), (64, 2, 0, 7, 0), (64, 3, 1, 8, 4)]
IDS = [f"n{n}-b{b}-mode{m}" for n, b, m, _, _ in CASES]
EDGES = [0, 1, 1 << 16, (1 << 20) - 1, 1 << 24, (1 << 30) + 1, P - 1, P, 1 << 31, 0xFFFFFFFF]


def pub_c(p: so.PublicC) -> rt.PublicInputsC:
    out = rt.PublicInputsC(p.n_real, p.entry, p.deferred, 0)
    out.program_digest[:] = list(p.prog); out.io_digest[:] = list(p.io)
    return out


@functools.lru_cache(maxsize=None)
def run(n_real: int, mode: int):
    blob = spec.fib_endless_program().to_bytes()
    cfg = {"enable_deferred_model": True} if mode else {}
    res = oracle.run(blob, max_cycles=n_real, enable_execution_trace=True, **cfg)
    assert len(res.rows) == n_real
    return res.rows, so.public_inputs(n_real, blob, [], list(res.outputs), (res.halt_kind, res.halt_code), deferred=bool(mode))


@functools.lru_cache(maxsize=None)
def built(case):
    n_real, b, mode, nq, bits = case
    rows, pub = run(n_real, mode)
    proof, bt = pr.prove_ref(rows, pub, b, nq, bits, want_built=True)
    proof.setflags(write=False)
    return proof, bt, pub


def both(t, pub, honest, min_q=1, min_bits=0) -> int:
    """the product's verdict, which must be the reference's"""
    got, want = rt.verify_rate(t, pub_c(pub), min_q, min_bits), pr.verify_ref(t, pub, min_q, min_bits, honest)
    assert got == want, f"zkir_verify_rate says {got}, the reference {want}"
    return got


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_proof_is_accepted_and_its_parts_stand_alone(case):
    proof, bt, pub = built(case)
    n_real, b, mode, nq, bits = case
    assert both(proof, pub, proof) == 0 and rt.verify_rate(proof, None, nq, bits) == 0
    at = pr.layout(proof)
    assert at["eval_proof"] == bt.at_eval and np.array_equal(proof[at["trace_root"]:at["eval_proof"]], bt.roots)
    inner = proof[at["eval_proof"]:]
    assert rt.batch_eval_verify(inner, bt.roots.reshape(3, 4), bt.points) == 0 and be.verify_ref(inner, bt.roots, bt.points) == 0
    rows, _ = run(n_real, mode)
    assert np.array_equal(bt.roots[:4], so.commit_trace(rows, b, pub=pub))          # the main commitment is the oracle's at this rate
    # one more query or bit than the proof states: 2
    assert both(proof, pub, proof, min_q=nq + 1) == 2 and both(proof, pub, proof, min_bits=bits + 1) == 2
    # not the expected run
    other = pub.clone(); other.n_real += 1
    assert both(proof, other, proof) == 6


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_quotient_is_of_low_degree(case):
    """the four coordinate columns of Q over the M-row coset have no coefficient from N up"""
    _, bt, pub = built(case)
    n = 1 << so.padded_log_n(pub.n_real)
    for i in range(4):
        c = so.ntt(bt.Q[i], inverse=True)
        assert c[:n].any() and not c[n:].any()


@pytest.mark.parametrize("n_real,mode", [(5, 0), (64, 1)])
def test_reference_quotients_of_different_rates_agree_on_the_shared_rows(n_real, mode):
    """built with the same challenges, row j of the blow-up-2 quotient is row j 2^(b-1) of the one at blow-up 2^b: the cosets nest"""
    rows, pub = run(n_real, mode)
    chal = tuple(np.random.default_rng(77 + n_real).integers(1, P, (3, 4), dtype=np.uint32))
    qs = {b: pr.prove_ref(rows, pub, b, 3, 0, want_built=True, challenges=chal)[1].Q for b in (1, 2, 3)}
    for b in (2, 3):
        assert np.array_equal(qs[b][:, ::1 << (b - 1)], qs[1])


def mutants(proof, rng):
    """[(label, words)]: header words at edges, a boundary-state word, program words, multiplicities, each root, the embedded header, shape, roots, points, evaluations, layer
    roots, final layer, nonce, query words, record and path words; cuts at every section boundary and at random; extensions; words >= p"""
    at, n = pr.layout(proof), len(proof)
    ev = at["eval_proof"]
    ia = be.layout(proof[ev:])
    out = []

    def put(label, pos, val):
        if val & 0xFFFFFFFF == int(proof[pos]):                       # (not a mutant)
            return
        t = proof.copy(); t[pos] = val & 0xFFFFFFFF
        out.append((f"{label}@{pos}={val}", t))

    def bump(label, pos):
        put(label, pos, (int(proof[pos]) + 1) % P)
    for pos in range(13):                                            # magic, version, log_n, width, queries, log_blowup, bits, n_real (2), mode, entry (3)
        for v in EDGES + [int(proof[pos]) + 1, max(int(proof[pos]) - 1, 0), 2, 3, 4, 5, 24, 25, 27, 128, 129]:
            put(f"header{pos}", pos, v)
    for pos in (13, 16, 17, 20):
        bump("digest", pos)
    for pos in (21, 22, 21 + 67, 21 + 68, 21 + 70, pr.HEADER - 1):
        bump("state", pos); put("state", pos, P)
    put("blob_len", at["program"], int(proof[at["program"]]) + 1); put("blob_len", at["program"], 0); put("blob_len", at["program"], 31); put("blob_len", at["program"], 1 << 31)
    for pos in (at["program"] + 1, at["program"] + 7, at["program"] + 17, at["rom_mult"] - 1):
        bump("program", pos); put("program", pos, 0x10000)
    for pos in (at["rom_mult"], at["rc_mult"], at["rc_mult"] + 5, at["trace_root"] - 1):
        bump("mult", pos)
    for pos in (at["trace_root"], at["trace_root"] + 3, at["aux_root"] + 1, at["quotient_root"] + 2):
        bump("root", pos)
    for pos in range(15):                                            # the embedded header and shape
        for v in (0, 1, 2, 3, 4, int(proof[ev + pos]) + 1, max(int(proof[ev + pos]) - 1, 0), 128, 129, P, 0xFFFFFFFF):
            put(f"inner header{pos}", ev + pos, v)
    for m in range(3):
        bump("inner root", ev + ia["roots"] + 4 * m + m)
    for i in range(2):
        bump("inner point", ev + ia["points"] + 4 * i + i)
    t = proof.copy(); t[ev + ia["points"] + 1:ev + ia["points"] + 4] = 0
    out.append(("inner point in the base field", t))
    for (i, m), pos in ia["evals_of"].items():
        for where in (pos, pos + 4 * ia["widths"][m] - 1):
            bump(f"eval({i},{m})", ev + where)
    bump("layer root", ev + ia["layer_roots"] + 1)
    bump("final", ev + ia["final"] + 2)
    for v in (0, int(proof[ev + ia["nonce"]]) + 1, P):
        put("nonce", ev + ia["nonce"], v)
    starts = [ev + ia["queries"] + t * ia["qsize"] for t in range(ia["num_queries"])]
    for s in (starts[0], starts[-1]):
        put("query", s, int(proof[s]) ^ 1)
        for m in range(3):
            for r0 in ia["records"][m]:
                bump(f"record{m} row", s + r0)
                bump(f"record{m} path", s + r0 + ia["widths"][m])
        for v_at, p_at, depth in ia["layers"]:
            bump("layer value", s + v_at)
            if depth:
                bump("layer path", s + p_at)
    bounds = [13, 21, pr.HEADER, at["program"] + 1, at["rom_mult"], at["rc_mult"], at["trace_root"], at["aux_root"], at["quotient_root"], ev, ev + 9, ev + 15, ev + ia["points"],
              ev + ia["evals"], ev + ia["layer_roots"], ev + ia["final"], ev + ia["queries"], starts[-1], n]
    for b in bounds:
        for cut in (b - 1, b, b + 1):
            if 0 <= cut < n:
                out.append((f"cut{cut}", proof[:cut].copy()))
    for cut in rng.integers(0, n, 8):
        out.append((f"cut{cut}", proof[:int(cut)].copy()))
    for extra in (1, 3, 32):
        out.append((f"extend{extra}", np.concatenate([proof, rng.integers(0, P, extra).astype(np.uint32)])))
    for pos in rng.integers(2, n, 24):
        bump("word", int(pos))
    for pos in rng.integers(2, n, 6):
        put("word>=p", int(pos), P + 5)
    return out


@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[5]], ids=[IDS[1], IDS[4], IDS[5]])
def test_every_mutant_gets_the_reference_code(case):
    proof, bt, pub = built(case)
    seen = {}
    for label, t in mutants(proof, np.random.default_rng(len(proof))):
        code = both(t, pub, proof)
        assert code != 0, f"{label}: accepted"
        seen.setdefault(code, label)
    want = {1, 2, 3, 6, 8, 10, 107, 108, 113}
    assert want <= set(seen) and (4 in seen or 101 in seen), f"codes seen: {sorted(seen)}"


def test_a_corrupted_trace_is_refused():
    """one written value of one row changed: the reference prover, following the honest procedure on the wrong trace, produces a quotient that is not of low degree, and the
    proof is refused"""
    rows, pub = run(64, 0)
    bad = rows.copy()
    bad["registers"][30, 4] ^= 1
    proof, bt = pr.prove_ref(bad, pub, 2, 6, 0, want_built=True)
    n = 1 << so.padded_log_n(pub.n_real)
    assert any(so.ntt(bt.Q[i], inverse=True)[n:].any() for i in range(4))
    assert rt.verify_rate(proof, pub_c(pub), 1, 0) != 0
