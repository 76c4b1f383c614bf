"""zkir_mixed_eval_verify under AddressSanitizer + UndefinedBehaviorSanitizer on honest and malformed 'ZKMH' proofs.  The host sources (zkir_amd.build.HOST_SOURCES) and a
stand-alone driver (tests/cpp/mixed_eval_san_driver.cpp, its own main) are compiled with -fsanitize=address,undefined exactly as tests/test_eval_sanitized.py builds its
driver, and the driver is run on test_mixed_eval_verify's reference proofs and mutants, each copied into a heap block of exactly its length: no sanitizer report, and every
verdict the one tests/mixed_eval_ref.py gives.  CPU only; nothing is loaded into Python and nothing is preloaded."""
from __future__ import annotations

import functools
import os
import subprocess

import numpy as np
import pytest

import mixed_eval_ref as mx
import test_mixed_eval_verify as tv
from test_host_sanitized import SAN, SAN_FLAGS, Corpus, _check, _linker
from zkir_amd import build as zbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "mixed_eval_san_driver.cpp")
BIN = os.path.join(SAN, "mixed_eval_san_driver")
MIXED = 0


@functools.lru_cache(maxsize=None)
def build_driver() -> str:
    """the sanitizer build of the host sources (the objects tests/test_eval_sanitized.py builds, shared) and this file's driver"""
    os.makedirs(SAN, exist_ok=True)
    probe = os.path.join(SAN, "probe.cpp")
    with open(probe, "w") as f:
        f.write("#include <vector>\nint main() { std::vector<int> v(3, 1); return v[0] + v[2] - 2; }\n")
    p = subprocess.run([zbuild.HIPCC, "-x", "c++", *SAN_FLAGS, probe, "-o", os.path.join(SAN, "probe")], capture_output=True, text=True)
    # a toolchain that cannot build or run a sanitized program is a failure of this test, not a reason to leave it out
    assert p.returncode == 0, "the compiler cannot link a program with the AddressSanitizer / UndefinedBehaviorSanitizer runtime: " + p.stderr[-300:]
    assert subprocess.run([os.path.join(SAN, "probe")], capture_output=True).returncode == 0, "a program linked with the sanitizer runtime does not run"
    deps = [os.path.normpath(os.path.join(zbuild.CSRC, h)) for h in zbuild.HEADERS]
    objs, jobs = [], []
    for src in [os.path.join(zbuild.CSRC, name) for name in zbuild.HOST_SOURCES] + [DRIVER_SRC]:
        obj = os.path.join(SAN, os.path.basename(src) + ".o")
        objs.append(obj)
        if zbuild._newer(src, obj, deps):
            jobs.append(subprocess.Popen([zbuild.HIPCC, "-x", "c++", "-std=c++17", *SAN_FLAGS, "-Wall", "-Wno-unused-function", "-c", src, "-o", obj]))
    for j in jobs:
        assert j.wait() == 0, "a sanitizer build of a host source failed"
    if zbuild._newer(objs[0], BIN, objs[1:]):
        subprocess.check_call([_linker(), "-fsanitize=address,undefined", *objs, "-o", BIN])
    return BIN


@pytest.fixture(scope="module")
def driver():
    return build_driver()


def test_mixed_eval_verify(driver):
    """zkir_mixed_eval_verify with every combination of expectations on the six reference proofs (two and three groups, every blow-up) and their mutants"""
    c = Corpus("mixed_eval")
    for shape in tv.SHAPES:
        pr = tv.proof(shape)
        rng = np.random.default_rng(299 + sum(shape[0]))
        roots, pts, ys = tv.expectations(pr, pr)
        assert mx.verify_ref(pr, roots, pts, ys) == 0
        base = c.base(pr)

        def add(label, t, exp, mutant):
            flags = sum(1 << k for k, e in enumerate(exp) if e is not None)
            want = mx.verify_ref(t, *exp)
            c.add(label, MIXED, [flags], [(base, t)] + [np.ascontiguousarray(e, dtype=np.uint32) for e in exp if e is not None], f"rc {want}", mutant=mutant, accepted=want == 0)
        for exp in ((None, None, None), (roots, None, None), (roots, pts, ys), (None, pts, None), (None, None, ys)):
            add("honest", pr, exp, False)
        for k, wrong in enumerate((roots, pts, ys)):
            w = wrong.copy(); w[-1] ^= 1
            add("honest, another expectation", pr, tuple(w if i == k else e for i, e in enumerate((roots, pts, ys))), True)
        for i, (label, t) in enumerate(tv.mixed_mutants(pr, rng)):
            r2, p2, y2 = tv.expectations(t, pr)
            add(f"{shape[0]}/{shape[1]} {label}", t, [(None, None, None), (r2, None, None), (r2, p2, y2), (None, p2, y2)][i % 4], True)
    # the cheating provers' proofs: a false evaluation of each group over the true codewords (8, then 10 below), a lower record at another row (7)
    shape = tv.SHAPES[4]
    groups = tv.groups_of(shape)
    y = mx.evaluate(groups, shape[1])
    for g in mx.layout(tv.proof(shape))["groups"]:
        off = y.copy(); off[g["first_e"], 0] = (off[g["first_e"], 0] + np.uint64(1)) % np.uint64(tv.P)
        t = mx.prove_ref(groups, shape[1], shape[3], shape[4], evals=off, quotient_evals=y)
        c.add("a false evaluation over the true codewords", MIXED, [0], [t], f"rc {mx.verify_ref(t)}", mutant=True, accepted=False)
    t = mx.prove_ref(groups, shape[1], shape[3], shape[4], low_q=lambda q, Mh: q * Mh // (1 << (shape[0][0] + shape[1] - 1)))
    c.add("a lower record at another row", MIXED, [0], [t], f"rc {mx.verify_ref(t)}", mutant=True, accepted=False)
    t = mx.prove_ref(groups, shape[1], shape[3], shape[4], final_add=[1, 0, 2, tv.P - 1])      # a final layer of degree < 4 that the last fold does not give (11)
    c.add("a shifted final layer", MIXED, [0], [t], f"rc {mx.verify_ref(t)}", mutant=True, accepted=False)
    assert len(c.cases) >= 1500
    codes = _check(driver, c, min_codes=5)
    assert {"rc 1", "rc 2", "rc 3", "rc 7", "rc 8", "rc 9", "rc 10", "rc 11", "rc 12", "rc 13"} <= set(codes), codes
    print(f"mixed_eval: {len(c.cases)} cases, {codes}")
