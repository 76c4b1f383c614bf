"""zkir_verify_rate_segment and zkir_verify_rate_chain under AddressSanitizer + UndefinedBehaviorSanitizer on honest and malformed 'ZKSR' segments and chains.  The host
sources (zkir_amd.build.HOST_SOURCES) and a stand-alone driver (tests/cpp/rate_chain_san_driver.cpp, its own main) are compiled with -fsanitize=address,undefined as
tests/test_prove_rate_sanitized.py builds its driver, and the driver is run on test_rate_chain_host's reference chains, wrong chains and about 300 mutants, each proof copied
into a heap block of exactly its length: no sanitizer report, and every verdict the one tests/rate_chain_ref.py gives.  CPU only; nothing is loaded into Python and nothing
is preloaded."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import rate_chain_ref as rc
import test_rate_chain_host as th
from test_eval_sanitized import build_driver as build_host_objects
from test_host_sanitized import SAN, SAN_FLAGS, Corpus, _check, _linker
from test_prove_rate_sanitized import expect_words
from zkir_amd import build as zbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "rate_chain_san_driver.cpp")
BIN = os.path.join(SAN, "rate_chain_san_driver")
SEGMENT, CHAIN = 0, 1
P = th.P


@pytest.fixture(scope="module")
def driver():
    """the sanitizer objects of the host sources are test_eval_sanitized's (built once for every driver); this driver's own object and link"""
    build_host_objects()
    objs = [os.path.join(SAN, name + ".o") for name in zbuild.HOST_SOURCES]
    obj = os.path.join(SAN, "rate_chain_san_driver.cpp.o")
    deps = [os.path.normpath(os.path.join(zbuild.CSRC, h)) for h in zbuild.HEADERS]
    if zbuild._newer(DRIVER_SRC, obj, deps):
        subprocess.check_call([zbuild.HIPCC, "-x", "c++", "-std=c++17", *SAN_FLAGS, "-Wall", "-Wno-unused-function", "-c", DRIVER_SRC, "-o", obj])
    if zbuild._newer(obj, BIN, objs):
        subprocess.check_call([_linker(), "-fsanitize=address,undefined", *objs, obj, "-o", BIN])
    return BIN


def states_fold(p) -> int:
    h = 0
    for w in p[21:21 + 136]:
        h = (31 * h + int(w)) & 0xFFFFFFFF
    return h


def test_segments_and_chains(driver):
    c = Corpus("rate_chain")
    rng = np.random.default_rng(23)
    n_mut = 0
    for mode, cuts, b in ((0, "A", 2), (1, "B", 3), (0, "B", 1)):
        s = th.chain(mode, cuts, b)
        _, run_pub = th.run(mode)
        bits = th.BITS[cuts]
        bases = [c.base(p) for p in s]
        exp = expect_words(run_pub)

        def add_chain(label, t, honests, with_expect, min_q=1, min_bits=0, mutant=True, base_of=None):
            want = rc.verify_chain_ref(t, run_pub if with_expect else None, min_q, min_bits, honests)
            bufs = [(base_of[k], p) if base_of and base_of[k] is not None else p for k, p in enumerate(t)]
            c.add(label, CHAIN, [min_q, min_bits, int(with_expect), len(t)], bufs + ([exp] if with_expect else []), f"rc {want}", mutant=mutant, accepted=want == 0)
        add_chain("honest", s, s, True, th.NQ, bits, mutant=False, base_of=bases)
        add_chain("honest, no expectation", s, s, False, mutant=False, base_of=bases)
        add_chain("one query more asked", s, s, True, th.NQ + 1, 0, base_of=bases)
        add_chain("empty", [], [], False)
        add_chain("first dropped", s[1:], s[1:], False, base_of=bases[1:])
        add_chain("a gap", [s[0], s[2]], [s[0], s[2]], True, base_of=[bases[0], bases[2]])
        add_chain("a repeat", [s[0], s[1], s[1]], [s[0], s[1], s[1]], False, base_of=[bases[0], bases[1], bases[1]])
        (a1, e1) = th.CUTS[cuts][1]
        for label, other in (("another rate", th.segment(mode, a1, e1, b % 3 + 1, th.NQ, bits)), ("another query count", th.segment(mode, a1, e1, b, th.NQ + 1, bits)),
                             ("the other mode", th.segment(1 - mode, a1, e1, b, th.NQ, bits))):
            t = [s[0], other, s[2]]
            add_chain(label, t, t, True, base_of=[bases[0], None, bases[2]])
        for i, (p, (a, e)) in enumerate(zip(s, th.CUTS[cuts])):
            seg_exp = expect_words(rc.segment_pub(run_pub, a, e))
            c.add(f"segment {i}", SEGMENT, [th.NQ, bits, 1], [(bases[i], p), seg_exp], f"rc 0 states {states_fold(p)}", accepted=True)
            c.add(f"segment {i} under the run's expectation", SEGMENT, [1, 0, 1], [(bases[i], p), exp], "rc 6", mutant=True, accepted=False)
        # single-word mutants, cuts and extensions of one segment: the chain's verdict and the segment's own
        for it in range(100):
            k = it % 3
            t = [p.copy() for p in s]
            kind = it % 10
            if kind == 8:
                t[k] = t[k][:int(rng.integers(0, len(t[k])))]
            elif kind == 9:
                t[k] = np.concatenate([t[k], rng.integers(0, P, int(rng.integers(1, 9))).astype(np.uint32)])
            else:
                pos = int(rng.integers(0, len(t[k]))) if kind % 2 else int(rng.integers(0, 200))
                t[k][pos] = (int(t[k][pos]) + 1 + int(rng.integers(0, 1000))) % P if kind < 7 else int(rng.integers(P, 1 << 32))
            if len(t[k]) == len(s[k]) and np.array_equal(t[k], s[k]):
                continue
            add_chain(f"mutant {it} of segment {k}", t, s, it % 2 == 0, base_of=bases)
            want = rc.verify_segment_ref(t[k], None, 1, 0, s[k])
            c.add(f"mutant {it} alone", SEGMENT, [1, 0, 0], [(bases[k], t[k])], f"rc {want}", mutant=True, accepted=want == 0)
            n_mut += 1
    assert n_mut >= 290
    codes = _check(driver, c, min_codes=10)
    assert {"rc 40", "rc 41", "rc 42", "rc 43", "rc 6", "rc 1002"} <= set(codes), codes
    print(f"rate_chain: {len(c.cases)} cases, {codes}")
