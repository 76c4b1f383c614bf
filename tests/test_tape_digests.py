"""(mode 4) What every hash call of a tape wrote, recomputed from the tape alone — zkir_hash_tape_new_bytes_host (hashcall::new_bytes over the parsed calls: what the
host verifier runs per call) against a Python reconstruction whose digests are the oracle's (tests/tape_digest_ref.py).  The device form is held to both in
tests/test_gpu_tape_digests.py."""
import os
import re

import numpy as np
import pytest

import tape_digest_ref as D
import tape_side_ref as R
from zkir_amd import runtime as rt


def test_host_new_bytes_equal_the_reconstruction_on_the_designed_tape():
    """SHA-256 lengths 0 1 55 56 63 64 65 119 120 128, Keccak-256 0 1 135 136 137 271 272 273, BLAKE3 0 1 63 64 65 1023 1024 1025 2048 2049 3072 (three chunks); in_ptr & 7
    over 0..7; out_ptr & 7 over 0..7 for kinds 5 / 6 and over 0 and 4 for kind 3; the output inside the input, the input inside the output's cells, exactly one shared cell,
    len = 0."""
    words = D.tape("designed")
    got = rt.hash_tape_new_bytes(words, device=False)
    want = D.designed_expected()
    assert got.dtype == np.uint64 and got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, ("first differing cell", int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])))
    calls = R.parse_tape(words)
    assert {c[2] for c in calls if c[4] == 3} >= set(D.SHA_LENS) and {c[2] for c in calls if c[4] == 5} >= set(D.KECCAK_LENS) and {c[2] for c in calls if c[4] == 6} >= set(D.BLAKE3_LENS)


def test_the_output_changes_only_the_cells_under_it():
    words = D.tape("designed")
    got = rt.hash_tape_new_bytes(words, device=False)
    h = 0
    for _, in_ptr, length, out_ptr, _, cells in R.parse_tape(words):
        for addr, (_, old) in zip(R.cells_of(in_ptr, length, out_ptr), cells):
            if addr + 8 <= out_ptr or addr >= out_ptr + 32:
                assert int(got[h]) == old, hex(addr)
            h += 1
    assert h == len(got)


def test_calls_of_max_len_equal_the_oracle():
    """one call of hashcall::MAX_LEN = 1 MiB per kind: the cells under the outputs hold the oracle's digests of the three messages, every other cell its old bytes"""
    words = D.tape("max_len")
    got = rt.hash_tape_new_bytes(words, device=False)
    at, want = D.expected_output_cells(words)
    assert len(at) == 4 + 4 + 5 + 5 and np.array_equal(got[at], want)
    old = np.concatenate([np.array([b for _, b in c[5]], np.uint64) for c in R.parse_tape(words)])
    rest = np.ones(len(got), bool); rest[at] = False
    assert np.array_equal(got[rest], old[rest])


def test_the_empty_tape_has_no_cells():
    assert len(rt.hash_tape_new_bytes(R.EMPTY, device=False)) == 0
    assert len(rt.hash_tape_new_bytes(None, device=False)) == 0


def test_a_malformed_section_is_refused_with_its_check():
    words = D.tape("designed").copy()
    words[1 + 8 + 5 + 2] = 0x10000                                                     # a piece of the first call's second cell
    with pytest.raises(rt.RuntimeError) as e:
        rt.hash_tape_new_bytes(words, device=False)
    assert e.value.code == rt.ERR_ARGUMENT and "56" in e.value.message
    with pytest.raises(rt.RuntimeError) as e:
        rt.hash_tape_new_bytes(D.tape("designed")[:-3], device=False)                  # cut inside the last record's cells
    assert e.value.code == rt.ERR_ARGUMENT and "4" in e.value.message


def test_the_header_declares_the_entries():
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "zkir_amd.h")).read()
    for name in ("zkir_hash_tape_new_bytes_launch", "zkir_hash_tape_new_bytes_host", "zkir_verify_device"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(rt.lib(), name), name


def test_verify_reports_its_stage_clocks_and_no_device_stage():
    """zkir_verify stays a host call: its clocks are recorded, none of its stages ran on a device."""
    import programs as pg
    from oracle import api as oracle, stark_api as so
    blob, ins, cfg = pg.sha256_hello()
    ores = oracle.run(blob, list(ins), enable_execution_trace=True, **{k: v for k, v in cfg.items() if k == "max_cycles"})
    pub = so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code), wide_mode=True)
    proof = so.prove(ores.rows, pub)
    assert rt.verify(proof) == 0
    st = rt.verify_last_stages()
    assert st["device_stages"] == 0 and all(st[k] >= 0 for k in ("parse", "section_digests", "hash_table_side", "wide_table_side", "rest")) and st["hash_table_side"] > 0
