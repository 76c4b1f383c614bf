"""The host code of a mode-4 proof's tape stages over a LIST of proofs under AddressSanitizer + UndefinedBehaviorSanitizer: the tape locator, the host list stage and the
deferring orchestration behind zkir_verify_many_tapes_host / zkir_verify_rate_many_tapes_host.  The host sources and a stand-alone driver
(tests/cpp/tape_many_san_driver.cpp, its own main) are compiled with -fsanitize=address,undefined exactly as tests/test_mem_many_sanitized.py builds its driver, and the
driver is run on honest, mutated and truncated proofs — the truncations cut at every section boundary — every proof and section in a heap block of exactly its length:
no sanitizer report, every verdict the single-proof host verifier's, every stage answer the Python reference's.  CPU only; nothing sanitized is loaded into Python and
nothing is preloaded."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import tape_many_ref as TR
from test_eval_sanitized import build_driver as build_host_objects
from test_host_sanitized import SAN, SAN_FLAGS, Corpus, _check, _linker
from zkir_amd import build as zbuild, runtime as rt, stark

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "tape_many_san_driver.cpp")
BIN = os.path.join(SAN, "tape_many_san_driver")

STAGE_BATCHES = ["calls_102", "one_call_x64", "no_predecessor", "failing_between", "lowest_wins", "header_only", "empty_and_not", "wide_failing", "ragged_chunks"]


@pytest.fixture(scope="module")
def driver():
    """the sanitizer objects of the host sources are test_eval_sanitized's (built once for every driver); this driver's own object and link"""
    build_host_objects()
    objs = [os.path.join(SAN, name + ".o") for name in zbuild.HOST_SOURCES]
    obj = os.path.join(SAN, "tape_many_san_driver.cpp.o")
    deps = [os.path.normpath(os.path.join(zbuild.CSRC, h)) for h in zbuild.HEADERS]
    if zbuild._newer(DRIVER_SRC, obj, deps):
        subprocess.check_call([zbuild.HIPCC, "-x", "c++", "-std=c++17", *SAN_FLAGS, "-Wall", "-Wno-unused-function", "-c", DRIVER_SRC, "-o", obj])
    if zbuild._newer(obj, BIN, objs):
        subprocess.check_call([_linker(), "-fsanitize=address,undefined", *objs, obj, "-o", BIN])
    return BIN


def _stage_case(c, what, b):
    hs, ws, n_real, code_end, alphas, lams = b
    hv, wv, d, s = TR.stage_ref(*b)
    u32 = lambda a: np.asarray(a, dtype=np.uint32)  # noqa: E731
    bufs = []
    for h, w, a, l in zip(hs, ws, alphas, lams):
        bufs += [u32(h), u32(w), u32(a), u32(l)]
    c.add(what, 0, [x for nr, ce in zip(n_real, code_end) for x in (nr, ce)], bufs,
          "rc 0 hv " + " ".join(str(x) for x in hv) + " wv " + " ".join(str(x) for x in wv) + " s " + " ".join(str(int(x)) for pair in s for e in pair for x in e)
          + " d " + " ".join(str(int(x)) for pair in d for sec in pair for row in sec for x in row))


def _located(proof, cut, lay):
    """what the locator answers on proof[:cut]: the hash section is located once its count word lies in the proof, the wide section once all its words do"""
    if cut <= lay["hash_section"]:
        return "rc 0 ok 0"
    words, whole = lay["wide_section"] - lay["hash_section"], cut >= lay["wide_section"]
    if not whole:                                               # the walk stops at the last record that lies in the proof whole
        q, hs = 1, proof[lay["hash_section"]:cut]
        for _ in range(int(hs[0])):
            if q + 8 > len(hs) or q + 8 + 5 * int(hs[q + 7]) > len(hs):
                break
            q += 8 + 5 * int(hs[q + 7])
        words = q
    wide = lay["wide_section"] if cut >= lay["rom_mult"] else -1
    return f"rc 0 ok 1 at {lay['hash_section']} words {words} whole {1 if whole else 0} wide {wide} n {int(proof[lay['wide_section']]) if wide >= 0 else 0}"


def test_the_list_stage_the_locator_and_the_orchestration(driver):
    c = Corpus("tape_many")
    batches = TR.designed_batches()
    for name in STAGE_BATCHES:
        _stage_case(c, name, batches[name])
    hs, ws, nr, ce, al, la = TR.batch([(TR.one_call(0), TR.wide_of(2)), (TR.one_call(1), TR.EMPTY)])
    u32 = lambda a: np.asarray(a, dtype=np.uint32)  # noqa: E731
    c.add("a cut wide section is refused (ZKIR_ERR_ARGUMENT = 9)", 0, [nr[0], ce[0], nr[1], ce[1]], [hs[0], ws[0][:-1], u32(al[0]), u32(la[0]), hs[1], ws[1], u32(al[1]), u32(la[1])], "rc 9")
    # the proofs: the expected verdicts from the single-proof host verifier
    honest = [p for _, p, _ in TR.honest_corpus()]
    c.add("the honest mixed batch", 1, [], honest, "rc 0 v " + " ".join(str(rt.verify(p)) for p in honest) + f" records {sum(TR.records(p) for p in honest)}")
    muts = [t for _, t in TR.mutants()]
    base = c.base(muts[0])
    want = [rt.verify(t) for t in muts]
    c.add("the mutants in one batch", 1, [], [(base, t) for t in muts], "rc 0 v " + " ".join(str(x) for x in want))
    perm = [int(i) for i in np.random.default_rng(4).permutation(len(muts))][:40]
    c.add("mutants in shuffled order", 1, [], [(base, muts[i]) for i in perm], "rc 0 v " + " ".join(str(want[i]) for i in perm))
    forged = TR.forged()
    c.add("the forged hash tapes", 1, [], [pr for _, pr, _ in forged], "rc 0 v " + " ".join(str(v) for _, _, v in forged))
    # truncations at EVERY section boundary (and one word to either side), alone and as one batch; the locator on each
    proof = muts[0]
    lay = stark.proof_layout(proof)
    at = stark.proof_layout(proof)["hash_section"]
    first_record = at + 1 + 8 + 5 * int(proof[at + 1 + 7])
    cuts = sorted({b + d for b in (lay["io_section"], lay["mem_section"], lay["hash_section"], first_record, lay["hash_section"] + 9, lay["wide_section"], lay["rom_mult"], len(proof))
                   for d in (-1, 0, 1) if 0 < b + d <= len(proof)})
    for cut in cuts:
        t = proof[:cut]
        c.add(f"cut at {cut}", 1, [], [(base, t)], f"rc 0 v {rt.verify(t)}")
        c.add(f"the locator, cut at {cut}", 3, [0], [(base, t)], _located(proof, cut, lay))
    c.add("every cut in one batch", 1, [], [(base, proof[:cut]) for cut in cuts], "rc 0 v " + " ".join(str(rt.verify(proof[:cut])) for cut in cuts))
    rate = TR.rate_corpus()
    rwant = [rt.verify_rate(p, None, q, b) for _, p, _, q, b in rate]
    c.add("the rate proof and its mutants", 2, [x for r in rate for x in (r[3], r[4])], [r[1] for r in rate], "rc 0 v " + " ".join(str(x) for x in rwant))
    rlay = stark.rate_proof_layout(rate[0][1])
    for cut in (rlay["hash_section"], rlay["hash_section"] + 1, rlay["wide_section"], rlay["wide_section"] + 1, rlay["rom_mult"]):
        t = rate[0][1][:cut]
        c.add(f"the rate proof cut at {cut}", 2, [rate[0][3], rate[0][4]], [t], f"rc 0 v {rt.verify_rate(t, None, rate[0][3], rate[0][4])}")
        c.add(f"the locator on the rate proof cut at {cut}", 3, [1], [t], _located(rate[0][1], cut, rlay))
    _check(driver, c)
    assert {4, 10, 56, 57} <= set(want) and {10, 56} <= set(rwant)
    print(f"tape_many: {len(c.cases)} cases")
