"""The host forms of the memory stages and zkir_verify under AddressSanitizer + UndefinedBehaviorSanitizer.  The host sources (zkir_amd.build.HOST_SOURCES) and a
stand-alone driver (tests/cpp/mem_stage_san_driver.cpp, its own main) are compiled with -fsanitize=address,undefined as tests/test_prove_rate_sanitized.py builds its
driver, and the driver is run on the sections of tests/mem_stage_ref.py and on the mutated mode-4 proofs of tests/test_gpu_verify_memory_device.py, each copied into a heap
block of exactly its length: no sanitizer report, every stage verdict and sum the Python reference's, every proof's verdict the oracle verifier's.  CPU only; nothing is
loaded into Python and nothing is preloaded."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import mem_stage_ref as M
import test_gpu_verify_memory_device as tm
from oracle import stark_api as so
from test_eval_sanitized import build_driver as build_host_objects
from test_host_sanitized import SAN, SAN_FLAGS, Corpus, _check, _linker
from zkir_amd import build as zbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "mem_stage_san_driver.cpp")
BIN = os.path.join(SAN, "mem_stage_san_driver")


@pytest.fixture(scope="module")
def driver():
    """the sanitizer objects of the host sources are test_eval_sanitized's (built once for every driver); this driver's own object and link"""
    build_host_objects()
    objs = [os.path.join(SAN, name + ".o") for name in zbuild.HOST_SOURCES]
    obj = os.path.join(SAN, "mem_stage_san_driver.cpp.o")
    deps = [os.path.normpath(os.path.join(zbuild.CSRC, h)) for h in zbuild.HEADERS]
    if zbuild._newer(DRIVER_SRC, obj, deps):
        subprocess.check_call([zbuild.HIPCC, "-x", "c++", "-std=c++17", *SAN_FLAGS, "-Wall", "-Wno-unused-function", "-c", DRIVER_SRC, "-o", obj])
    if zbuild._newer(obj, BIN, objs):
        subprocess.check_call([_linker(), "-fsanitize=address,undefined", *objs, obj, "-o", BIN])
    return BIN


def test_the_stages_and_the_verifier(driver):
    c = Corpus("mem_stage")
    for what, sec, mode, n_code, built_for in M.check_cases():
        assert M.section_verdict(sec, mode, n_code) == built_for
        c.add(what, 0, [mode, n_code], [sec], f"rc 0 v {built_for}", mutant=built_for != 0, accepted=built_for == 0)
    u32 = lambda a: np.asarray(a, dtype=np.uint32)  # noqa: E731
    for what, sec, blob, alpha, lam in M.side_cases():
        s = M.table_side(sec, blob, alpha, lam)
        c.add(what, 1, [], [sec, np.frombuffer(blob, dtype=np.uint8), u32(alpha), u32(lam)], f"rc 0 s {s[0]} {s[1]} {s[2]} {s[3]}")
    # sections the side refuses (ZKIR_ERR_ARGUMENT = 9): cut, and a cell out of range
    sec = M.section(M.increasing(9))
    bad = sec.copy(); bad[1 + 7 * 8] = 1 << 20
    for what, s in (("cut", sec[:-1]), ("limb", bad), ("empty buffer", sec[:0])):
        c.add(f"side refuses: {what}", 1, [], [s, np.zeros(0, np.uint8), u32(M.ALPHA), u32(M.LAM)], "rc 9 s")
    muts = tm.mutations()
    base = c.base(muts[0][1])
    for what, t in muts:
        want = so.verify(t)
        c.add(what, 2, [], [(base, t)], f"rc {want}", mutant=what != "honest", accepted=want == 0)
    codes = _check(driver, c, min_codes=8)
    assert {"rc 4", "rc 12", "rc 54", "rc 55", "rc 0 v 4", "rc 0 v 54", "rc 0 v 55"} <= set(codes), codes
    print(f"mem_stage: {len(c.cases)} cases, {codes}")
