"""The device query stage is ONE record, one kernel pair and one runner (query_stage.inl) behind the single-proof commitment entries, the list entries and the STARK
entries.  This file holds the entries against each other on the smallest proofs the other files build: every proof and every mutant goes through its single-proof entry,
its list entry with n = 1 and its list entry in a batch of three between two honest proofs of other shapes, and all three verdicts are the host entry's.

Mutants, one per flag class (hash jobs of a matrix record, hash jobs through a path, the layer-0 waves, the fold lanes, the final layer a fold lane ends on), plus for the
STARK proof a cut inside the last query (n_full < num_queries: the device takes the whole queries, the host loop the cut one).  The four small proofs have ONE FRI layer, so
their "middle layer" mutant falls on that layer's second value; the two [1, 3, 1] proofs behind them have a real middle layer.  No test provokes a device fault."""
import pytest

import stark_query_cases as sq
import test_gpu_pcs_verify_device as tp
from zkir_amd import runtime as rt

pytestmark = pytest.mark.gpu

# the smallest 'ZKLD', 'ZKEV' and 'ZKBE' shapes of test_gpu_pcs_verify_device.py (log_n 3, b 1, three queries), then a 'ZKLD' proof with the schedule [1, 3, 1]
PCS_CASES = [("ld", tp.LD_SHAPES[0]), ("ev", tp.EV_SHAPES[0]), ("be", tp.BE_SHAPES[0]), ("ld", (7, 2, 17, 4, 4))]
# the honest neighbours of a batch of three: other kinds, rates, widths and schedules than any case above
PCS_NEIGHBOURS = [("ev", (5, 2, 5, 2, 4, 3)), ("be", (3, 3, ((8, 0b11), (1, 0b01)), 2, 3, 3))]
KIND_NO = {"ld": 0, "ev": 1, "be": 2}
# mode 0 at log_n 3 (one layer), then log_n 7 (the schedule [1, 3, 1]); the neighbours: other modes (so widths), heights and schedules
STARK_CASES = [(0, 3), (0, 7)]
STARK_NEIGHBOURS = [(1, 4), (2, 5)]


def pcs_mutants(kind, pr):
    """[(what, words)]: the honest proof and one mutant per flag class, all in query 0 (the final layer has no query)"""
    at = tp.LAYOUT[kind](pr)
    s, layers = at["queries"], at["layers"]
    v0 = layers[0][0]
    mid = layers[len(layers) // 2][0]
    return [("honest", pr), ("a leaf word", tp.bump(pr, s + 1)), ("a path word", tp.bump(pr, s + v0 - 1)), ("a layer-0 value", tp.bump(pr, s + v0 + 4)),
            ("a middle layer's value", tp.bump(pr, s + mid + 1)), ("a final-layer word", tp.bump(pr, at["final"] + 1))]


def stark_mutants(proof):
    q = sq.query_layout(proof)
    a, rec, nl = q["at_queries"], q["records"], q["n_layers"]
    last = a + (q["num_queries"] - 1) * q["qsize"]
    return [("honest", proof), ("a leaf word", sq.bump(proof, a + rec[1])), ("a path word", sq.bump(proof, a + rec[1] + q["WM"])), ("a layer-0 value", sq.bump(proof, a + rec[7] + 4)),
            ("a middle layer's value", sq.bump(proof, a + rec[7 + nl // 2] + 1)), ("a final-layer word", sq.bump(proof, a - 33 + 1)),
            ("cut inside the last query", proof[:last + rec[4] + 2])]


@pytest.mark.parametrize("kind,shape", PCS_CASES)
def test_a_commitment_proof_gets_one_verdict_from_every_entry(kind, shape):
    pr = tp.PROOF[kind](shape)
    (ka, a), (kb, b) = [(k, tp.PROOF[k](s)) for k, s in PCS_NEIGHBOURS]
    codes = set()
    for what, m in pcs_mutants(kind, pr):
        host = tp.HOST[kind](m)
        assert (host == 0) == (what == "honest"), (what, host)
        single = tp.device_verdict(kind, m)
        alone = rt.pcs_verify_many([KIND_NO[kind]], [m])
        three = rt.pcs_verify_many([KIND_NO[ka], KIND_NO[kind], KIND_NO[kb]], [a, m, b])
        assert single == host and alone == [host] and three == [0, host, 0], (what, host, single, alone, three)
        codes.add(host)
    assert {0, 7, 8} <= codes, codes                                 # (a condition on the inputs: a hash flag and a layer-0 flag decide among them)


@pytest.mark.parametrize("mode,log_n", STARK_CASES)
def test_a_stark_proof_gets_one_verdict_from_every_entry(mode, log_n):
    proof, _ = sq.oracle_proof(mode, log_n)
    a, b = [sq.oracle_proof(*c)[0] for c in STARK_NEIGHBOURS]
    codes = set()
    for what, m in stark_mutants(proof):
        host = rt.verify(m)
        assert (host == 0) == (what == "honest"), (what, host)
        single = rt.verify(m, device=True, queries=True)
        alone = rt.verify_many([m])
        three = rt.verify_many([a, m, b])
        assert single == host and alone == [host] and three == [0, host, 0], (what, host, single, alone, three)
        codes.add(host)
    assert {0, 4, 21, 23} <= codes, codes                            # (a condition on the inputs: a cut, a matrix record's and a layer's hash flag are among them)


def test_alternating_shapes_on_one_thread():
    """a STARK call, a commitment call, a STARK call on one thread and device: the stages share the staging and the record, and none reads another's leftovers"""
    proof, _ = sq.oracle_proof(0, 3)
    stark_cases = [m for _, m in stark_mutants(proof)]
    stark_host = [rt.verify(m) for m in stark_cases]
    for kind, shape in PCS_CASES[:3]:
        pcs_cases = [m for _, m in pcs_mutants(kind, tp.PROOF[kind](shape))]
        pcs_host = [tp.HOST[kind](m) for m in pcs_cases]
        for i, (m, want) in enumerate(zip(pcs_cases, pcs_host)):
            before, after = i % len(stark_cases), (i + 3) % len(stark_cases)
            got = (rt.verify(stark_cases[before], device=True, queries=True), tp.device_verdict(kind, m), rt.verify(stark_cases[after], device=True, queries=True))
            assert got == (stark_host[before], want, stark_host[after]), (kind, i, got)
