"""The DEVICE forms of the memory stages as calls of their own (zkir_mem_section_check_launch: mem_section_check_kernel; zkir_mem_table_side_launch:
mem_section_side_kernel — csrc/mem_stage.inl) against both the host forms and the Python reference of tests/mem_stage_ref.py, on synthetic sections at the kernels' edges:
chunk and workgroup boundaries, the lowest failing cell among several, every check of a cell, the code segment's two ends, the image's edges, and one cell past the side
kernel's grid cap.  The chunk digests run through the verifier entry: tests/test_gpu_verify_memory_device.py."""
import numpy as np
import pytest

import mem_stage_ref as M
from zkir_amd import runtime as rt

pytestmark = pytest.mark.gpu

CHECK, SIDE = M.check_cases(), M.side_cases()


@pytest.mark.parametrize("case", CHECK, ids=[c[0] for c in CHECK])
def test_the_check_kernel_gives_the_host_and_reference_verdict(case):
    what, sec, mode, n_code, built_for = case
    assert M.section_verdict(sec, mode, n_code) == built_for
    assert rt.mem_section_check(sec, mode, n_code, device=True) == rt.mem_section_check(sec, mode, n_code, device=False) == built_for


def test_the_lowest_failing_cell_wins_across_workgroups():
    """failing cells with different codes in different workgroups and in one: the verdict is the lowest cell's, whichever workgroup's atomic lands first"""
    addrs = [8 * i for i in range(300)] + [0x1000] + [0x1008 + 8 * i for i in range(600)]      # cell 300 is on the code (55 with two code words)
    base = M.cells_at(addrs, seed=5)
    for bad_at, want in ((100, 54), (299, 54), (301, 55), (600, 55), (900, 55)):
        c = [list(x) for x in base]; c[bad_at][5] = 0x10000
        sec = M.section(c)
        assert M.section_verdict(sec, 3, 2) == want
        assert rt.mem_section_check(sec, 3, 2, device=True) == rt.mem_section_check(sec, 3, 2, device=False) == want


@pytest.mark.parametrize("case", SIDE, ids=[c[0] for c in SIDE])
def test_the_side_kernel_gives_the_host_and_reference_sum(case):
    what, sec, blob, alpha, lam = case
    dev = [int(x) for x in rt.mem_table_side(sec, blob, alpha, lam, device=True)]
    assert dev == [int(x) for x in rt.mem_table_side(sec, blob, alpha, lam, device=False)]
    assert dev == M.table_side(sec, blob, alpha, lam)


def test_one_cell_past_the_grid_cap():
    """MEM_MAX_BLOCKS x NT + 1 cells (3.7 MB): the first lane takes a second cell at the grid's stride.  Against the host form (the reference holds it at the small sizes)."""
    n = M.SIDE_GRID_CAP * M.NT + 1
    rng = np.random.default_rng(9)
    addr = 0x1000 + 8 * np.arange(n, dtype=np.int64)           # (the first cells lie in the image)
    cells = np.stack([addr & 0xFFFFF, addr >> 20, rng.integers(0, M.P, n), *rng.integers(0, 1 << 16, (4, n))], axis=1)
    sec = M.section(cells)
    blob = M.make_blob(bytes(rng.integers(0, 256, 64, dtype=np.uint8)), bytes(rng.integers(0, 256, 1000, dtype=np.uint8)))
    assert rt.mem_section_check(sec, 3, 0, device=True) == 0
    assert rt.mem_section_check(sec, 3, 16, device=True) == rt.mem_section_check(sec, 3, 16, device=False) == 55
    last = sec.copy(); last[-1] = 0x10000                        # .. and the check kernel's last workgroup holds one cell
    assert rt.mem_section_check(last, 3, 0, device=True) == 54
    dev = rt.mem_table_side(sec, blob, M.ALPHA, M.LAM, device=True)
    assert [int(x) for x in dev] == [int(x) for x in rt.mem_table_side(sec, blob, M.ALPHA, M.LAM, device=False)]
    # the cell past the cap counts: without it the sum is another
    assert [int(x) for x in rt.mem_table_side(M.section(cells[:-1]), blob, M.ALPHA, M.LAM, device=True)] != [int(x) for x in dev]


def test_the_side_refuses_what_is_not_a_checked_section():
    sec = M.section(M.increasing(300))
    bad = sec.copy(); bad[1 + 7 * 299 + 3] = 0x10000
    for s in (sec[:-1], bad):
        with pytest.raises(Exception):
            rt.mem_table_side(s, b"", M.ALPHA, M.LAM, device=True)
