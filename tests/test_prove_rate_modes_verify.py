"""zkir_verify_rate on mode-3 and mode-4 'ZKSR' proofs without a GPU: the two proofs of tests/golden/rate_mode_proofs.json (the GPU prover's own output, frozen by
tests/golden/make_rate_mode_proofs.py — no outside reference) are accepted under public inputs rebuilt from the oracle's run of the same programs, and mutants of every
section are refused with the code include/zkir_amd.h names.  A verifier without these modes answers 2 to both proofs."""
from __future__ import annotations

import base64
import functools
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

import batch_eval_ref as be
import programs as pg
from oracle import api as oracle, stark_api as so
from test_prove_rate_verify import pub_c
from zkir_amd import runtime as rt, stark

P = so.P
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rate_mode_proofs.json")
KEYS = ["mode3", "mode4"]


@functools.lru_cache(maxsize=None)
def golden(key):
    doc = json.load(open(GOLDEN))
    g = doc["proofs"][key]
    raw = zlib.decompress(base64.b64decode(g["words"]))
    assert hashlib.sha256(raw).hexdigest() == g["sha256"] and len(raw) == 4 * g["n_words"]
    proof = np.frombuffer(raw, dtype="<u4").astype(np.uint32)
    proof.setflags(write=False)
    wide = g["mode"] == 4
    blob, ins, cfg = pg.off_code(g["program"])
    cfg = {k: v for k, v in cfg.items() if k == "max_cycles"}
    ores = oracle.run(blob, list(ins), enable_execution_trace=True, **cfg)
    assert len(ores.rows) == g["rows"]
    opub = so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code), mem_mode=not wide, wide_mode=wide)
    return proof, opub, ores.rows, doc["log_blowup"], doc["num_queries"], doc["pow_bits"]


def test_the_fixture_is_small():
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "config_proofs.json"))


@pytest.mark.parametrize("key", KEYS)
def test_golden_proof_is_accepted(key):
    proof, opub, rows, b, nq, bits = golden(key)
    mode = 3 if key == "mode3" else 4
    at = stark.rate_proof_layout(proof)
    assert (int(proof[0]), int(proof[1]), int(proof[9]), at["log_blowup"], at["num_queries"], at["pow_bits"]) == (0x52534B5A, 1, mode, b, nq, bits)
    assert int(proof[3]) == so.committed_width(mode) == (264 if mode == 3 else 288)
    assert rt.verify_rate(proof, pub_c(opub), nq, bits) == 0 and rt.verify_rate(proof, None, 1, 0) == 0
    # the main commitment is the oracle's at this rate; the embedded proof stands alone under the outer roots
    assert np.array_equal(proof[at["trace_root"]:at["trace_root"] + 4], so.commit_trace(rows, b, pub=opub))
    inner = proof[at["eval_proof"]:]
    ia = be.layout(inner)
    assert ia["widths"] == [so.committed_width(mode), so.aux_width(mode), 4]
    roots = proof[at["trace_root"]:at["eval_proof"]].reshape(3, 4)
    assert rt.batch_eval_verify(inner, roots, inner[ia["points"]:ia["evals"]].reshape(2, 4)) == 0
    # more than the proof states; another run; the other verifier
    assert rt.verify_rate(proof, pub_c(opub), nq + 1, bits) == 2 and rt.verify_rate(proof, pub_c(opub), nq, bits + 1) == 2
    other = opub.clone(); other.n_real += 1
    assert rt.verify_rate(proof, pub_c(other), nq, bits) == 6
    assert rt.verify(proof) != 0


@pytest.mark.parametrize("key", KEYS)
def test_mutants_are_refused_with_the_expected_codes(key):
    proof, opub, rows, b, nq, bits = golden(key)
    mode = 3 if key == "mode3" else 4
    pub = pub_c(opub)
    at, n = stark.rate_proof_layout(proof), len(proof)
    ev = at["eval_proof"]
    ia = be.layout(proof[ev:])

    def code_of(pos, val):
        t = proof.copy(); t[pos] = val & 0xFFFFFFFF
        return rt.verify_rate(t, pub, nq, bits)

    def bumped(pos):
        return code_of(pos, (int(proof[pos]) + 1) % P)
    # header: magic and version 1; ranges 2 (a mode whose width is not the header's among them); a word >= p where a field element is expected 3
    assert code_of(0, 0x46504B5A) == 1 and code_of(1, 2) == 1 and code_of(1, 12) == 1
    for pos, val in ((2, 27), (3, 160), (3, 264 if mode == 4 else 288), (4, 0), (4, 129), (5, 0), (5, 4), (6, 25), (9, 2), (9, 7 - mode), (9, 5)):
        assert code_of(pos, val) in ((1, 2) if (pos, val) == (9, 5) else (2,)), (pos, val)
    assert code_of(21, P) == 3 and code_of(at["trace_root"], P + 1) == 3
    # the touched cells: an address that is no multiple of 8, the first two cells in the wrong order
    m0 = at["mem_section"]
    n_cells = int(proof[m0])
    assert n_cells >= 1
    assert bumped(m0 + 1) == 54
    if n_cells >= 2:
        t = proof.copy(); t[m0 + 1:m0 + 8], t[m0 + 8:m0 + 15] = proof[m0 + 8:m0 + 15], proof[m0 + 1:m0 + 8]
        assert rt.verify_rate(t, pub, nq, bits) == 54
    assert bumped(m0 + 3) in (54, 10) and bumped(m0 + 4) == 10             # a cell's final time, its final bytes: the memory check does not close
    if mode == 4:                                                            # the hash tape: the call's record
        h0 = at["hash_section"]
        assert int(proof[h0]) == 1 and int(proof[at["wide_section"]]) == 0
        for word in (1, 2, 8):
            assert bumped(h0 + word) in (56, 10), word
        assert code_of(h0, 2) in (56, 4) and code_of(at["wide_section"], 1) in (57, 4)
    # multiplicities and roots: the table side, then the transcript, no longer match — the constraints fail at zeta
    for pos in (at["rom_mult"], at["rc_mult"], at["trace_root"] - 1, at["trace_root"] + 1, at["aux_root"] + 2, at["quotient_root"] + 3):
        assert bumped(pos) == 10, pos
    # the embedded proof: its shape 5; the quotient's evaluations at zeta, which the identity reads, 10; any other evaluation 10 or the evaluation proof's own code
    assert code_of(ev + 2, int(proof[ev + 2]) + 1) == 5 and code_of(ev + 9, 160) == 5 and code_of(ev + 6, nq + 1) == 5
    q_at = ia["evals_of"][(0, 2)]
    for k in range(16):
        assert bumped(ev + q_at + k) == 10, k
    for (i, m), pos in ia["evals_of"].items():
        for where in (pos, pos + 4 * ia["widths"][m] - 1):
            c = bumped(ev + where)
            assert c == 10 or c > 100, (i, m, where, c)
    # the one query: a record's row (hashed into its leaf) and its path 107; the first layer's values, compared with the combination of the records before their own path, 108
    s = ev + ia["queries"]
    for m in range(3):
        for r0 in ia["records"][m]:
            assert bumped(s + r0) == 107 and bumped(s + r0 + ia["widths"][m]) == 107, m
    assert bumped(s + ia["layers"][0][0]) == 108
    # cuts at every section boundary: truncated (1 inside the header, 4 behind it, the evaluation proof's "wrong length" inside its query section)
    bounds = [13, 21, at["rom_mult"], at["rc_mult"], at["trace_root"], at["aux_root"], at["quotient_root"], ev, ev + 15, ev + ia["points"], ev + ia["evals"], ev + ia["layer_roots"],
              ev + ia["final"], ev + ia["queries"], n, m0, m0 + 1 + 7 * n_cells] + ([at["io_section"]] if at["io_section"] else []) + ([at["hash_section"], at["wide_section"]] if mode == 4 else [])
    for bnd in bounds:
        for cut in (bnd - 1, bnd, bnd + 1):
            if 0 <= cut < n:
                c = rt.verify_rate(proof[:cut].copy(), pub, nq, bits)
                assert c in (1, 4, 101), (cut, c)
    assert rt.verify_rate(np.concatenate([proof, np.zeros(1, np.uint32)]), pub, nq, bits) != 0
