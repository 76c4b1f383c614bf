"""(mode 4) The tapes' share of the lookup table side and the hash tape's record checks as calls of their own, HOST forms (zkir_tape_table_side_host: the function zkir_prove
runs for the hash calls of a caller's host witness; zkir_hash_tape_check_host: hashcall::parse_section itself) against a reference in Python integers that applies the
fingerprint convention to the tape words (tests/tape_side_ref.py).  The device forms are held to both in tests/test_gpu_tape_table_side.py."""
import numpy as np
import pytest

import tape_side_ref as R
from zkir_amd import runtime as rt


@pytest.mark.parametrize("name", R.SYNTHETIC)
def test_host_table_side_equals_the_reference_on_designed_tapes(name):
    """sum, every hh and every ww, word for word: the empty tape, len = 0, one and two spans, a 2^17-byte call between two small ones, item counts around the kernels'
    workgroup size, the five wide opcodes at their edges (sorted and reversed), both sections at once."""
    hs, nb, ws = R.synthetic(name)
    R.assert_equal(rt.tape_table_side(hs, nb, ws, R.ALPHA, R.LAM, device=False), R.synthetic_reference(name), name)


def test_record_order_of_the_wide_section_permutes_ww_and_keeps_the_sum():
    a = rt.tape_table_side(*R.synthetic("wide_sorted"), R.ALPHA, R.LAM, device=False)
    b = rt.tape_table_side(*R.synthetic("wide_reversed"), R.ALPHA, R.LAM, device=False)
    assert np.array_equal(a["sum"], b["sum"]) and np.array_equal(a["ww"], b["ww"][::-1]) and len(a["ww"]) == len(R.RECORD_OPS)
    assert len({tuple(int(x) for x in r) for r in a["ww"]}) == len(R.RECORD_OPS)          # (distinct values: the permutation is visible)


@pytest.mark.parametrize("name", R.REAL)
def test_host_table_side_and_checks_on_the_sections_of_real_runs(name):
    """The sections the ORACLE's proof of the run carries; each touched cell's new bytes derived here: its old bytes from the tape, overlaid with the call's 32 bytes from the
    interpreter's hash_outs record.  Other challenges than the designed tapes'."""
    hs, nb, ws, n_real, code_end = R.real_sections(name)
    assert (int(hs[0]) > 0) == (name != "signed_division_loop") and (int(ws[0]) > 0) == (name in ("signed_division_loop", "wide_and_hash"))
    alpha, lam = [7, R.P - 1, 0, 123456], [2, 0, 0, 1]
    R.assert_equal(rt.tape_table_side(hs, nb, ws, alpha, lam, device=False), R.reference(hs, nb, ws, alpha, lam), name)
    assert rt.hash_tape_check(hs, n_real, code_end, device=False) == 0


# what the issue lists, with the code hashcall.h states for it
LISTED = {"r1_limb_2p20": 56, "r0_cycle_n_real": 56, "r1_cycle_not_above": 56, "r2_kind_4": 56, "r0_sha_out_misaligned": 56, "r1_len_over": 56, "r2_out_in_code": 55,
          "r0_count_plus": 56, "r2_count_minus": 56, "r1_piece_2p16": 56, "r2_told_after": 56, "cut_in_last_cells": 4, "cut_in_last_header": 4}


def test_host_check_codes_on_single_fault_mutations():
    base, _ = R.check_tape()
    assert rt.hash_tape_check(base, R.CHECK_N_REAL, R.CHECK_CODE_END, device=False) == 0 == R.expected_check_code(base)
    muts = dict(R.check_mutations())
    assert set(LISTED) <= set(muts)
    for name, words in muts.items():
        want = R.expected_check_code(words)
        assert want in (4, 55, 56) and LISTED.get(name, want) == want, name
        assert rt.hash_tape_check(words, R.CHECK_N_REAL, R.CHECK_CODE_END, device=False) == want, name


def test_arguments_are_checked():
    hs, nb, ws = R.synthetic("both")
    with pytest.raises(ValueError):
        rt.tape_table_side(hs, nb[:-1], ws, R.ALPHA, R.LAM, device=False)            # one new-bytes entry short
    with pytest.raises(ValueError):
        rt.tape_table_side(hs, nb, ws[:-1], R.ALPHA, R.LAM, device=False)
    with pytest.raises(rt.RuntimeError) as e:
        rt.tape_table_side(hs, nb, ws, [R.P, 0, 0, 0], R.LAM, device=False)          # alpha not canonical
    assert e.value.code == rt.ERR_ARGUMENT
    bad = hs.copy(); bad[1 + 6] = 4                                                    # kind 4: a section parse_section rejects
    with pytest.raises(rt.RuntimeError) as e:
        rt.tape_table_side(bad, nb, ws, R.ALPHA, R.LAM, device=False)
    assert e.value.code == rt.ERR_ARGUMENT and "56" in e.value.message
