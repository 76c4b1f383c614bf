"""The host code of the memory stages over a LIST of proofs under AddressSanitizer + UndefinedBehaviorSanitizer: the section locator, the host list stage and the
deferring orchestration behind zkir_verify_many_memory_host / zkir_verify_rate_many_memory_host.  The host sources and a stand-alone driver
(tests/cpp/mem_many_san_driver.cpp, its own main) are compiled with -fsanitize=address,undefined exactly as tests/test_mem_stage_sanitized.py builds its driver, and the
driver is run on the batches of tests/test_verify_many_memory.py — every proof, section and blob in a heap block of exactly its length: no sanitizer report, every
verdict the single-proof host verifier's, every stage answer the Python reference's.  CPU only; nothing sanitized is loaded into Python and nothing is preloaded."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import mem_many_ref as MR
import test_verify_many_memory as TH
from test_eval_sanitized import build_driver as build_host_objects
from test_host_sanitized import SAN, SAN_FLAGS, Corpus, _check, _linker
from zkir_amd import build as zbuild, runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "mem_many_san_driver.cpp")
BIN = os.path.join(SAN, "mem_many_san_driver")


@pytest.fixture(scope="module")
def driver():
    """the sanitizer objects of the host sources are test_eval_sanitized's (built once for every driver); this driver's own object and link"""
    build_host_objects()
    objs = [os.path.join(SAN, name + ".o") for name in zbuild.HOST_SOURCES]
    obj = os.path.join(SAN, "mem_many_san_driver.cpp.o")
    deps = [os.path.normpath(os.path.join(zbuild.CSRC, h)) for h in zbuild.HEADERS]
    if zbuild._newer(DRIVER_SRC, obj, deps):
        subprocess.check_call([zbuild.HIPCC, "-x", "c++", "-std=c++17", *SAN_FLAGS, "-Wall", "-Wno-unused-function", "-c", DRIVER_SRC, "-o", obj])
    if zbuild._newer(obj, BIN, objs):
        subprocess.check_call([_linker(), "-fsanitize=address,undefined", *objs, obj, "-o", BIN])
    return BIN


def _stage_case(c, what, b):
    secs, modes, code_words, blobs, alphas, lams = b
    v, d, s = MR.stage_ref(*b)
    u32 = lambda a: np.asarray(a, dtype=np.uint32)  # noqa: E731
    words = lambda rows: " ".join(str(int(x)) for row in rows for x in row)  # noqa: E731
    bufs = []
    for sec, blob, a, l in zip(secs, blobs, alphas, lams):
        bufs += [u32(sec), np.frombuffer(blob, dtype=np.uint8), u32(a), u32(l)]
    c.add(what, 0, [x for m, n in zip(modes, code_words) for x in (m, n)], bufs,
          "rc 0 v " + " ".join(str(x) for x in v) + " s " + words(s) + " d " + words([row for sec in d for row in sec]))


def test_the_list_stage_and_the_orchestration(driver):
    c = Corpus("mem_many")
    for k, order in enumerate(MR.SIZES_ORDERS):
        _stage_case(c, f"the sizes batch, order {k}", MR.batch(MR.sizes_sections(order), seed=k))
    _stage_case(c, "the image's edges under three images", TH.edge_batch())
    _stage_case(c, "failing sections among well-formed ones", TH.failing_batch())
    secs, modes, code_words, blobs, alphas, lams = MR.batch(MR.sizes_sections([1, 2]))
    u32 = lambda a: np.asarray(a, dtype=np.uint32)  # noqa: E731
    cut = [secs[0], np.frombuffer(blobs[0], np.uint8), u32(alphas[0]), u32(lams[0]), secs[1][:-1], np.frombuffer(blobs[1], np.uint8), u32(alphas[1]), u32(lams[1])]
    c.add("a cut section is refused (ZKIR_ERR_ARGUMENT = 9)", 0, [3, 5, 3, 5], cut, "rc 9")
    # the proofs: every batch of the CPU tests, the expected verdicts from the single-proof host verifier
    honest = [p for _, p, _ in MR.honest_corpus()]
    c.add("the honest mixed batch", 1, [], honest, "rc 0 v " + " ".join(str(rt.verify(p)) for p in honest) + f" cells {sum(MR.count_word(p) for p in honest)}")
    muts = [t for _, t in MR.mutants()]
    base = c.base(muts[0])
    want = [rt.verify(t) for t in muts]
    c.add("the mutants in one batch", 1, [], [(base, t) for t in muts], "rc 0 v " + " ".join(str(x) for x in want))
    perm = [int(i) for i in np.random.default_rng(4).permutation(len(muts))][:40]
    c.add("mutants in shuffled order", 1, [], [(base, muts[i]) for i in perm], "rc 0 v " + " ".join(str(want[i]) for i in perm))
    for _, t, host, _ in TH.probe_cases()[-2:]:               # (the two cuts, alone)
        c.add("a cut proof alone", 1, [], [(base, t)], f"rc 0 v {host}")
    rate = MR.rate_corpus()
    rwant = [rt.verify_rate(p, None, q, b) for _, p, _, q, b, _ in rate]
    c.add("the rate proofs and their mutants", 2, [x for r in rate for x in (r[3], r[4])], [r[1] for r in rate],
          "rc 0 v " + " ".join(str(x) for x in rwant) + f" cells {sum(MR.located_cells(r[1], r[5]) for r in rate)}")
    _check(driver, c)
    assert {4, 12, 54, 55} <= set(want) and {10, 54} <= set(rwant)
    print(f"mem_many: {len(c.cases)} cases")
