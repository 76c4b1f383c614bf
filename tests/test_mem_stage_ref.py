"""The HOST forms of the memory stages as calls of their own (zkir_mem_section_check_host: the cell loop of zkir_verify; zkir_mem_table_side_host: the cells' share of the
lookup table side by batch inversion) against the Python reference of tests/mem_stage_ref.py, on the sections the GPU tests hold the kernels to.  No GPU."""
import numpy as np
import pytest

import mem_stage_ref as M
from zkir_amd import runtime as rt

CHECK, SIDE = M.check_cases(), M.side_cases()


@pytest.mark.parametrize("case", CHECK, ids=[c[0] for c in CHECK])
def test_the_cell_checks_give_the_reference_verdict(case):
    what, sec, mode, n_code, built_for = case
    assert M.section_verdict(sec, mode, n_code) == built_for, "the reference disagrees with what the case was built to show"
    assert rt.mem_section_check(sec, mode, n_code, device=False) == built_for


@pytest.mark.parametrize("case", SIDE, ids=[c[0] for c in SIDE])
def test_the_table_side_is_the_reference_sum(case):
    what, sec, blob, alpha, lam = case
    assert M.section_verdict(sec, 3, 0) == 0
    assert [int(x) for x in rt.mem_table_side(sec, blob, alpha, lam, device=False)] == M.table_side(sec, blob, alpha, lam)


def test_the_image_rule():
    """image_cell: the bytes at 0x1000 + i are blob[32 + i] for i below code + data; a short blob and one whose header claims more than it holds give zeros"""
    blob = M.make_blob(bytes(range(1, 21)), bytes(range(101, 114)))
    assert M.image_cell(blob, 0x1000) == int.from_bytes(bytes(range(1, 9)), "little")
    assert M.image_cell(blob, 0xFF8) == 0 and M.image_cell(blob, 0x1028) == 0
    assert M.image_cell(blob, 0x1020) == 113                   # (the data's last byte, then zeros)
    assert M.image_cell(blob[:31], 0x1000) == 0 and M.image_cell(M.make_blob(bytes(20), bytes(13), claim_data=14), 0x1000) == 0
    # an empty section sums to zero whatever the blob; one cell whose final tuple IS its initial tuple (time 0, the image's bytes) cancels
    assert [int(x) for x in rt.mem_table_side(M.section([]), blob, M.ALPHA, M.LAM, device=False)] == [0, 0, 0, 0]
    img = M.image_cell(blob, 0x1008)
    one = M.section([[0x1008, 0, 0, *[(img >> (16 * i)) & 0xFFFF for i in range(4)]]])
    assert [int(x) for x in rt.mem_table_side(one, blob, M.ALPHA, M.LAM, device=False)] == [0, 0, 0, 0]


def test_the_side_refuses_what_is_not_a_checked_section():
    sec = M.section(M.increasing(5))
    bad = sec.copy(); bad[1] = 1 << 20
    for s, a in ((sec[:-1], M.ALPHA), (bad, M.ALPHA), (sec, [M.P, 0, 0, 0])):
        with pytest.raises(Exception):
            rt.mem_table_side(s, b"", a, M.LAM, device=False)


def test_memory_needs_the_device():
    with pytest.raises(ValueError):
        rt.verify(np.zeros(4, np.uint32), memory=True)
    with pytest.raises(ValueError):
        rt.verify_rate(np.zeros(4, np.uint32), memory=True)
