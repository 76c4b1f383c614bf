"""zkir_verify_rate under AddressSanitizer + UndefinedBehaviorSanitizer on honest and malformed 'ZKSR' proofs.  The host sources (zkir_amd.build.HOST_SOURCES) and a
stand-alone driver (tests/cpp/rate_san_driver.cpp, its own main) are compiled with -fsanitize=address,undefined as tests/test_eval_sanitized.py builds its driver, and the
driver is run on test_prove_rate_verify's reference proofs and mutants, each copied into a heap block of exactly its length: no sanitizer report, and every verdict the one
tests/prove_rate_ref.py gives.  CPU only; nothing is loaded into Python and nothing is preloaded."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import prove_rate_ref as pr
import test_prove_rate_verify as tv
from test_eval_sanitized import build_driver as build_host_objects
from test_host_sanitized import SAN, SAN_FLAGS, Corpus, _check, _linker
from zkir_amd import build as zbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "rate_san_driver.cpp")
BIN = os.path.join(SAN, "rate_san_driver")


@pytest.fixture(scope="module")
def driver():
    """the sanitizer objects of the host sources are test_eval_sanitized's (built once for every driver); this driver's own object and link"""
    build_host_objects()
    objs = [os.path.join(SAN, name + ".o") for name in zbuild.HOST_SOURCES]
    obj = os.path.join(SAN, "rate_san_driver.cpp.o")
    deps = [os.path.normpath(os.path.join(zbuild.CSRC, h)) for h in zbuild.HEADERS]
    if zbuild._newer(DRIVER_SRC, obj, deps):
        subprocess.check_call([zbuild.HIPCC, "-x", "c++", "-std=c++17", *SAN_FLAGS, "-Wall", "-Wno-unused-function", "-c", DRIVER_SRC, "-o", obj])
    if zbuild._newer(obj, BIN, objs):
        subprocess.check_call([_linker(), "-fsanitize=address,undefined", *objs, obj, "-o", BIN])
    return BIN


def expect_words(pub) -> np.ndarray:
    return np.array([pub.n_real & 0xFFFFFFFF, pub.n_real >> 32, pub.entry & 0xFFFFFFFF, pub.entry >> 32, pub.deferred, *pub.prog, *pub.io], np.uint32)


def test_verify_rate(driver):
    """three reference proofs (log_n 3 and 6, blow-up 4 and 8, both modes), their mutants, cuts and extensions, with and without the expected run, and a higher query floor"""
    c = Corpus("prove_rate")
    for case in (tv.CASES[1], tv.CASES[4], tv.CASES[5]):
        proof, bt, pub = tv.built(case)
        nq, bits = case[3], case[4]
        base = c.base(proof)
        exp = expect_words(pub)

        def add(label, t, with_expect, min_q, min_bits, mutant):
            want = pr.verify_ref(t, pub if with_expect else None, min_q, min_bits, proof)
            c.add(label, 0, [min_q, min_bits, int(with_expect)], [(base, t)] + ([exp] if with_expect else []), f"rc {want}", mutant=mutant, accepted=want == 0)
        add("honest", proof, True, nq, bits, False)
        add("honest, no expectation", proof, False, 1, 0, False)
        add("honest, one query more asked", proof, True, nq + 1, bits, True)
        add("honest, one bit more asked", proof, False, nq, bits + 1, True)
        for i, (label, t) in enumerate(tv.mutants(proof, np.random.default_rng(len(proof)))):
            add(f"{tv.IDS[tv.CASES.index(case)]} {label}", t, i % 3 != 0, 1, 0, True)
    assert len(c.cases) >= 900
    codes = _check(driver, c, min_codes=8)
    assert {"rc 1", "rc 2", "rc 3", "rc 8", "rc 10", "rc 107", "rc 108", "rc 113"} <= set(codes), codes
    print(f"prove_rate: {len(c.cases)} cases, {codes}")
