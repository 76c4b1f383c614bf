"""zkir_batch_eval_verify under AddressSanitizer + UndefinedBehaviorSanitizer on honest and malformed batched evaluation proofs.  The stand-alone driver of
tests/test_eval_sanitized.py (tests/cpp/eval_san_driver.cpp with the host sources, one build for both files; case kind 1 calls zkir_batch_eval_verify) is run on
test_batch_eval_verify's reference proofs and mutants, each copied into a heap block of exactly its length: no sanitizer report, and every verdict the one
tests/batch_eval_ref.py gives.  CPU only; nothing is loaded into Python and nothing is preloaded."""
from __future__ import annotations

import numpy as np
import pytest

import batch_eval_ref as be
import test_batch_eval_verify as tv
from test_eval_sanitized import build_driver
from test_host_sanitized import Corpus, _check

BATCH = 1


@pytest.fixture(scope="module")
def driver():
    return build_driver()


def test_batch_eval_verify(driver):
    """zkir_batch_eval_verify with every combination of expectations on three reference proofs (one, two and three matrices) and their mutants"""
    c = Corpus("batch_eval")
    for shape in tv.SHAPES:
        pr = tv.proof(shape)
        rng = np.random.default_rng(199 + shape[0])
        roots, pts, ys = tv.expectations(pr, pr)
        assert be.verify_ref(pr, roots, pts, ys) == 0
        base = c.base(pr)

        def add(label, t, exp, mutant):
            flags = sum(1 << k for k, e in enumerate(exp) if e is not None)
            want = be.verify_ref(t, *exp)
            c.add(label, BATCH, [flags], [(base, t)] + [np.ascontiguousarray(e, dtype=np.uint32) for e in exp if e is not None], f"rc {want}", mutant=mutant, accepted=want == 0)
        for exp in ((None, None, None), (roots, None, None), (roots, pts, ys), (None, pts, None), (None, None, ys)):
            add("honest", pr, exp, False)
        for k, wrong in enumerate((roots, pts, ys)):
            w = wrong.copy(); w[-1] ^= 1
            add("honest, another expectation", pr, tuple(w if i == k else e for i, e in enumerate((roots, pts, ys))), True)
        for i, (label, t) in enumerate(tv.batch_mutants(pr, rng)):
            r2, p2, y2 = tv.expectations(t, pr)
            add(f"log_n {shape[0]} {label}", t, [(None, None, None), (r2, None, None), (r2, p2, y2), (None, p2, y2)][i % 4], True)
    assert len(c.cases) >= 900
    codes = _check(driver, c, min_codes=5)
    assert {"rc 1", "rc 2", "rc 7", "rc 8", "rc 12", "rc 13"} <= set(codes), codes
    print(f"batch_eval: {len(c.cases)} cases, {codes}")
