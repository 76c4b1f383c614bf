"""zkir_eval_verify under AddressSanitizer + UndefinedBehaviorSanitizer on honest and malformed evaluation proofs.  The host sources (zkir_amd.build.HOST_SOURCES) and a
stand-alone driver (tests/cpp/eval_san_driver.cpp, its own main; case kind 0 calls zkir_eval_verify) are compiled with -fsanitize=address,undefined exactly as tests/test_host_sanitized.py builds its driver,
and the driver is run on test_eval_verify's reference proofs and mutants, each copied into a heap block of exactly its length: no sanitizer report, and every verdict the one
tests/eval_ref.py gives.  CPU only; nothing is preloaded."""
from __future__ import annotations

import functools
import os
import subprocess

import numpy as np
import pytest

import eval_ref as ev
import test_eval_verify as tv
from test_host_sanitized import SAN, SAN_FLAGS, Corpus, _check, _linker
from zkir_amd import build as zbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "eval_san_driver.cpp")
BIN = os.path.join(SAN, "eval_san_driver")
EVAL = 0


@functools.lru_cache(maxsize=None)
def build_driver() -> str:
    """the sanitizer build of the host sources and the driver (shared with tests/test_batch_eval_sanitized.py: one binary, built once)"""
    os.makedirs(SAN, exist_ok=True)
    probe = os.path.join(SAN, "probe.cpp")
    with open(probe, "w") as f:
        f.write("#include <vector>\nint main() { std::vector<int> v(3, 1); return v[0] + v[2] - 2; }\n")
    p = subprocess.run([zbuild.HIPCC, "-x", "c++", *SAN_FLAGS, probe, "-o", os.path.join(SAN, "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([os.path.join(SAN, "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler cannot link or run a program with the AddressSanitizer / UndefinedBehaviorSanitizer runtime: " + p.stderr[-300:])
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


def test_eval_verify(driver):
    """zkir_eval_verify with every combination of expectations on three reference proofs with distinct schedules and their mutants"""
    c = Corpus("eval")
    for shape in tv.SHAPES:
        pr = tv.proof(shape)
        rng = np.random.default_rng(99 + shape[0])
        root, pts, ys = tv.expectations(pr, pr)
        assert ev.verify_ref(pr, root, pts, ys) == 0
        base = c.base(pr)

        def add(label, t, exp, mutant):
            flags = sum(1 << k for k, e in enumerate(exp) if e is not None)
            want = ev.verify_ref(t, *exp)
            c.add(label, EVAL, [flags], [(base, t)] + [np.ascontiguousarray(e, dtype=np.uint32) for e in exp if e is not None], f"rc {want}", mutant=mutant, accepted=want == 0)
        for exp in ((None, None, None), (root, None, None), (root, pts, ys), (None, pts, None), (None, None, ys)):
            add("honest", pr, exp, False)
        for k, wrong in enumerate((root, pts, ys)):
            w = wrong.copy(); w[-1] ^= 1
            add("honest, another expectation", pr, tuple(w if i == k else e for i, e in enumerate((root, pts, ys))), True)
        for i, (label, t) in enumerate(tv.eval_mutants(pr, rng)):
            r2, p2, y2 = tv.expectations(t, pr)
            add(f"log_n {shape[0]} {label}", t, [(None, None, None), (r2, None, None), (r2, p2, y2), (None, p2, y2)][i % 4], True)
    assert len(c.cases) >= 900
    codes = _check(driver, c, min_codes=5)
    assert {"rc 8", "rc 12", "rc 13"} <= set(codes), codes
    print(f"eval: {len(c.cases)} cases, {codes}")
