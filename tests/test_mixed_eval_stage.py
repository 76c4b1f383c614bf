"""zkir_mixed_eval_verify behind its query stage (verify_stages.h: MixedQueries), without a GPU: the host stage is the loop it was, so the entry gives the reference's verdict
with and without the device= keyword; the mixed schedule's longest case — 10 layers, one more than a single-height proof can have — is reached by HOLLOW proofs (a correct
header, the exact length, zeros below), which pin the stage's own layer bound on the host path.  The helpers here are also the device tests'."""
from __future__ import annotations

import functools
import itertools

import numpy as np
import pytest

import lowdeg_ref as ld
import mixed_eval_ref as mx
import test_mixed_eval_verify as tm
from zkir_amd import runtime as rt

MAX_LAYERS = 10                                                      # verify_stages.h: MIXED_MAX_LAYERS
LONG_PAIR = ((26, 3), 1)                                             # the tallest trace over the lowest table: depth-26 paths and 10 layers


@functools.lru_cache(maxsize=None)
def longest_schedules():
    """(the most layers any pair or triple of heights has at any b, the first pair reaching it, the first triple reaching it): every (log_ns, b) a proof can state"""
    best, first = 0, {}
    for b in (1, 2, 3):
        for r in (2, 3):
            for log_ns in itertools.combinations(range(27 - b, 2, -1), r):
                n = len(mx.schedule(log_ns, b))
                if n > best:
                    best, first = n, {}
                if n == best:
                    first.setdefault(r, (log_ns, b))
    return best, first[2], first[3]


def hollow(log_ns, b: int, num_queries: int = 2) -> np.ndarray:
    """A proof of one width-1 matrix and one point per group with pow_bits 0: a correct header, the exact length, points outside the base field, zeros everywhere else.
    It passes checks 1 - 5 (zeros are a final layer of degree < 4; no grinding) and reaches the query stage."""
    shapes = [([1], [1], 1)] * len(log_ns)
    pr = np.zeros(rt.mixed_eval_proof_words(log_ns, b, shapes, num_queries), np.uint32)
    assert len(pr) == mx.proof_words(log_ns, b, shapes, num_queries) > 0
    pr[:7] = [mx.MAGIC, mx.VERSION, b, len(log_ns), num_queries, 0, len(mx.schedule(log_ns, b))]
    for h, log_n in enumerate(log_ns):
        pr[7 + 5 * h:12 + 5 * h] = [log_n, 1, 1, 1, 1]
    at = mx.layout(pr)
    for g in at["groups"]:
        pr[g["points"]:g["points"] + 4] = [1, 1 + g["log_n"], 0, 0]
    return pr


def samples(pr) -> list:
    """the rows the transcript of `pr` (one that passes checks 1 - 5) samples: verify_ref's transcript"""
    at = mx.layout(pr)
    ch = ld.Challenger()
    ch.observe_n(pr[:at["layer_roots"]])
    ch.sample_ext()
    for j in range(len(at["ks"])):
        ch.observe_n(pr[at["layer_roots"] + 4 * j:at["layer_roots"] + 4 * j + 4])
        ch.sample_ext()
    ch.observe_n(pr[at["final"]:at["nonce"]])
    assert ch.check_pow(int(pr[at["nonce"]]), int(pr[5]))
    return [ch.sample_bits(at["groups"][0]["log_M"] - 1) for _ in range(at["num_queries"])]


def with_index_words(pr) -> np.ndarray:
    """`pr` with every query's index word set to the transcript's sample (the query section is not part of the transcript): check 6 passes"""
    at = mx.layout(pr)
    t = pr.copy()
    for i, q in enumerate(samples(pr)):
        t[at["queries"] + i * at["qsize"]] = q
    return t


def test_no_pair_or_triple_has_more_than_ten_layers():
    best, pair, triple = longest_schedules()
    assert best == MAX_LAYERS
    assert len(pair[0]) == 2 and len(triple[0]) == 3 and len(mx.schedule(*pair)) == len(mx.schedule(*triple)) == MAX_LAYERS
    assert mx.schedule(*LONG_PAIR) == [1, 3, 3, 3, 3, 3, 3, 3, 1, 1]
    # the hash jobs of a query at their most: group 0's four matrices twice, two lower groups' four once, the layers
    assert 2 * 4 + 2 * 4 + best == 26


@pytest.mark.parametrize("shape", tm.SHAPES, ids=lambda s: f"{s[0]}/{s[1]}")
def test_the_host_entry_is_the_reference_with_and_without_the_keyword(shape):
    pr = tm.proof(shape)
    want = mx.verify_ref(pr)
    assert want == 0 and rt.mixed_eval_verify(pr) == want and rt.mixed_eval_verify(pr, device=False) == want
    exp = tm.expectations(pr, pr)
    assert rt.mixed_eval_verify(pr, *exp, device=False) == mx.verify_ref(pr, *exp) == 0
    at = mx.layout(pr)
    for pos, code in ((at["queries"], 6), (at["queries"] + 1, 7), (at["queries"] + at["layers"][0][0], 8), (at["queries"] + at["layers"][-1][1], 9)):
        t = tm.bumped(pr, pos)
        assert rt.mixed_eval_verify(t, device=False) == rt.mixed_eval_verify(t) == mx.verify_ref(t) == code, pos


@pytest.mark.parametrize("which", [1, 2], ids=["pair", "triple"])
def test_hollow_ten_layer_proofs_get_the_references_verdict(which):
    log_ns, b = LONG_PAIR if which == 1 else longest_schedules()[2]
    pr = hollow(log_ns, b)
    assert int(pr[6]) == MAX_LAYERS and len(pr) < 4096               # (a proof's length grows with log M, not with M)
    got = rt.mixed_eval_verify(pr)
    assert got == mx.verify_ref(pr) and got in (6, 7), got         # (6 unless both samples are row 0)
    t = with_index_words(pr)                                         # past check 6: the zero records do not hash to the zero roots
    assert rt.mixed_eval_verify(t) == mx.verify_ref(t) == 7
    for cut in (pr[:-1], np.concatenate([pr, pr[:1]])):
        assert rt.mixed_eval_verify(cut) == mx.verify_ref(cut) == 1
    more = pr.copy(); more[6] += 1
    assert rt.mixed_eval_verify(more) == mx.verify_ref(more) == 1
