"""The witness-expansion kernels (witness.hip) through their public launch entry points on synthetic event logs that sit on the kernels' path edges, bit-exact against the
plain references of tests/witness_ref.py (which tests/test_witness_ref.py holds against the CPU oracle).

Every output buffer is a little larger than needed and prefilled with the byte 0xA5, which no correct output consists of; after the call the live part must equal the
reference and every other byte must still be 0xA5 — an entry a kernel fails to store shows, and so does a store behind the end, into the padding columns of a matrix or
into an output of a refused call."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from zkir_amd import runtime as rt

import witness_ref as wr

pytestmark = pytest.mark.gpu

FILL = 0xA5
SLACK = 96                                                    # items behind the live part of every buffer


class Buf:
    """`count + SLACK` items of `dtype` on the device, every byte FILL."""

    def __init__(self, count, dtype):
        self.dtype, self.count = np.dtype(dtype), count
        self.t = torch.full(((count + SLACK) * self.dtype.itemsize,), FILL, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr()

    def host(self):
        return self.t.cpu().numpy().view(self.dtype)

    def check(self, want, what):
        """the first len(want) items equal `want`, every byte behind them is untouched"""
        got, n = self.host(), len(want)
        assert n <= self.count
        assert np.array_equal(got[:n], want), f"{what}: differs first at {np.nonzero(got[:n] != want)[0][:4]} of {n}"
        assert (got[n:].view(np.uint8) == FILL).all(), f"{what}: bytes behind item {n} were written"

    def check_matrix(self, want, stride, what, lead=0):
        """behind `lead` untouched items, rows of `stride` items: the first want.shape[1] of each equal `want`, the padding columns and everything else are untouched"""
        got = self.host()
        rows, n = want.shape
        m = got[lead:lead + rows * stride].reshape(rows, stride)
        assert np.array_equal(m[:, :n], want), f"{what}: differs first at (row, column) {np.argwhere(m[:, :n] != want)[:4].tolist()}"
        assert (np.ascontiguousarray(m[:, n:]).view(np.uint8) == FILL).all(), f"{what}: columns {n}..{stride} were written"
        assert (got[:lead].view(np.uint8) == FILL).all() and (got[lead + rows * stride:].view(np.uint8) == FILL).all(), f"{what}: bytes outside the matrix were written"

    def untouched(self, what):
        assert (self.host().view(np.uint8) == FILL).all(), f"{what} was written"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc):
    assert rc == rt.ZKIR_OK, rt.lib().zkir_last_error().decode()


# ---- memory ops ---------------------------------------------------------------------------------------------------------------------------------------------------------
MEMOP_FIELDS = rt._MEMOP_DTYPE.names                         # the order of zkir_memop_columns


class MemopBufs:
    def __init__(self, n):
        self.b = {f: Buf(n, rt._MEMOP_DTYPE[f]) for f in MEMOP_FIELDS}
        self.c = rt.MemopColumnsC(*[self.b[f].ptr for f in MEMOP_FIELDS])

    def check(self, want, what):
        for f in MEMOP_FIELDS:
            self.b[f].check(want[f], f"{what}.{f}")


@functools.lru_cache(maxsize=None)
def _mem_want(name, cycle_base):
    ev, n_rows, _ = wr.MEM_CASES[name]
    return wr.memops(ev, n_rows, cycle_base)


@pytest.mark.parametrize("cycle_base", [0, 2**33 + 5], ids=["base_0", "base_2p33_5"])
@pytest.mark.parametrize("route", ["one_pass_csr", "separate_passes"])
@pytest.mark.parametrize("name", sorted(wr.MEM_CASES))
def test_memory_ops(name, route, cycle_base):
    """Both routes to the same columns: zkir_memops_expand_csr_launch + _sort_prepared_launch (inline and queued gaps, the neighbour by shuffle or by lane 0's own load, the
    shape flags) and _row_offsets_launch + _expand_launch + _sort_launch; the sort by merge rank in LDS (segments of at most 2048 ops), in global memory, or by counting."""
    ev, n_rows, _ = wr.MEM_CASES[name]
    rows, offsets, srt, flags = _mem_want(name, cycle_base)
    L, n, d_ev, sp = rt.lib(), len(ev), _dev(ev), _sp()
    row_b, srt_b, offs, seg = MemopBufs(n), MemopBufs(n), Buf(n_rows + 1, "<u8"), Buf(n_rows, "u1")
    if route == "one_pass_csr":
        _ok(L.zkir_memops_expand_csr_launch(d_ev.data_ptr(), n, n_rows, cycle_base, C.byref(row_b.c), offs.ptr, seg.ptr, sp))
    else:
        _ok(L.zkir_memops_row_offsets_launch(d_ev.data_ptr(), n, n_rows, offs.ptr, sp))
        _ok(L.zkir_memops_expand_launch(d_ev.data_ptr(), n, cycle_base, C.byref(row_b.c), sp))
    torch.cuda.synchronize()
    offs.check(offsets, "row_offsets")                        # before the sort reads them: it trusts the offsets and the flags it is given
    row_b.check(rows, "row order")
    if route == "one_pass_csr":
        seg.check(flags, "shape flags")
        _ok(L.zkir_memops_sort_prepared_launch(d_ev.data_ptr(), n, cycle_base, offs.ptr, seg.ptr, C.byref(srt_b.c), sp))
    else:
        _ok(L.zkir_memops_sort_launch(d_ev.data_ptr(), n, n_rows, cycle_base, offs.ptr, seg.ptr, C.byref(srt_b.c), sp))
    torch.cuda.synchronize()
    seg.check(flags, "shape flags")                           # the check pass of the stand-alone sort leaves the same flags in its scratch
    srt_b.check(srt, "sorted")
    offs.check(offsets, "row_offsets behind the sort")


# ---- range checks -------------------------------------------------------------------------------------------------------------------------------------------------------
def _range_check(ev, chunk_bits, with_mult=True, expect=rt.ZKIR_OK):
    L, n, d_ev = rt.lib(), len(ev), _dev(ev)
    stride = (n + 127) // 128 * 128                            # the result handle's rounding
    value, pc, chunks, mult = Buf(n, "<u8"), Buf(n, "<u8"), Buf(4 * stride, "<u2"), Buf(1 << chunk_bits, "<u4")
    rc = L.zkir_range_check_expand_launch(d_ev.data_ptr(), n, chunk_bits, value.ptr, pc.ptr, chunks.ptr, stride, mult.ptr if with_mult else None, _sp())
    torch.cuda.synchronize()
    assert rc == expect
    if expect != rt.ZKIR_OK:
        for b, what in ((value, "value"), (pc, "pc"), (chunks, "chunks"), (mult, "multiplicity")):
            b.untouched(f"refused call: {what}")
        return
    w_value, w_pc, w_chunks, w_mult = wr.range_checks(ev, chunk_bits)
    value.check(w_value, "value"); pc.check(w_pc, "pc")
    chunks.check_matrix(np.ascontiguousarray(w_chunks.T), stride, "chunks")
    if with_mult:
        mult.check(w_mult, "multiplicity")
    else:
        mult.untouched("multiplicity (not passed)")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("chunk_bits", range(8, 16))
def test_range_check_every_chunk_width(chunk_bits, n):
    _range_check(wr.rc_log(n, 100 * chunk_bits + n), chunk_bits)


@pytest.mark.parametrize("with_mult", [True, False], ids=["multiplicity", "null_multiplicity"])
@pytest.mark.parametrize("n", [262145, 524365])
def test_range_check_grid_stride_passes(n, with_mult):
    """The grid is capped at 1024 workgroups of 256: event 262 144 is lane 0's second turn; 524 365 gives 77 lanes a third."""
    _range_check(wr.rc_log(n, n), 10, with_mult)


def test_range_check_one_table_entry_takes_every_atomic():
    _range_check(wr.rc_log(262145, 7, identical=True), 10)


def test_range_check_null_multiplicity_small():
    _range_check(wr.rc_log(257, 8), 12, with_mult=False)


@pytest.mark.parametrize("chunk_bits", [7, 16])
def test_range_check_refuses_chunk_widths_outside_8_to_15(chunk_bits):
    _range_check(wr.rc_log(300, 9), chunk_bits, expect=rt.ERR_ARGUMENT)


# ---- normalization ------------------------------------------------------------------------------------------------------------------------------------------------------
NORM_COLUMNS = (("cycle", "<u8"), ("pc", "<u8"), ("reg", "u1"), ("opcode", "u1"), ("accumulated0", "<u8"), ("accumulated1", "<u8"), ("normalized0", "<u4"),
                ("normalized1", "<u4"), ("carry0", "<u4"), ("carry1", "<u4"))                        # the order of zkir_norm_columns


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_normalization_events_over_the_raw_value_range(n):
    """Raw values over all 64 bits in both register states, the limb and carry edges among them (all twelve from n = 255 on)."""
    ev = wr.norm_log(n, n)
    want = wr.norm(ev)
    bufs = {k: Buf(n, dt) for k, dt in NORM_COLUMNS}
    cols = rt.NormColumnsC(*[bufs[k].ptr for k, _ in NORM_COLUMNS])
    d_ev = _dev(ev)
    _ok(rt.lib().zkir_norm_expand_launch(d_ev.data_ptr(), n, C.byref(cols), _sp()))
    torch.cuda.synchronize()
    for k in ("cycle", "pc", "reg", "opcode"):
        bufs[k].check(want[k], k)
    for j in (0, 1):
        bufs[f"accumulated{j}"].check(want["accumulated"][:, j], f"accumulated{j}")
        bufs[f"normalized{j}"].check(want["normalized"][:, j], f"normalized{j}")
        bufs[f"carry{j}"].check(want["carries"][:, j], f"carry{j}")


# ---- SHA-256 chip -------------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sha_case(n):
    blk = wr.sha_blocks(n, n)
    return blk, wr.sha256_witness_columns(blk["message_block"])


def _sha(n, stride, form, lead=0, with_ts=True):
    """`lead`: words by which `out` is advanced inside its allocation.  `form`: the kernel the launch rule of zkir_sha256_chip_launch must pick for these arguments (16-byte
    column stores need stride % 4 == 0 and a 16-byte aligned `out`)."""
    blk, want = _sha_case(n)
    d_blk = _dev(blk)
    out, ts = Buf(608 * stride + lead, "<u4"), Buf(n, "<u8")
    assert out.ptr % 16 == 0
    out_ptr = out.ptr + 4 * lead
    assert ("x4" if stride % 4 == 0 and out_ptr % 16 == 0 else "scalar") == form
    rc = rt.lib().zkir_sha256_chip_launch(d_blk.data_ptr(), n, out_ptr, stride, ts.ptr if with_ts else None, _sp())
    torch.cuda.synchronize()
    _ok(rc)
    out.check_matrix(want, stride, "columns", lead=lead)
    if with_ts:
        ts.check(blk["timestamp"], "timestamps")
    else:
        ts.untouched("timestamps (not passed)")


def _round64(n):
    return (n + 63) // 64 * 64


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 1022, 1025, 1027, 2049])
def test_sha256_chip_four_blocks_per_lane(n):
    """All 608 columns of all blocks: full lanes, ragged last lanes of 1, 2 and 3 blocks, in the first workgroup (1024 blocks) and in a second and a third."""
    _sha(n, _round64(n), "x4")


@pytest.mark.parametrize("n", [1, 255, 257, 1027])
def test_sha256_chip_one_block_per_lane_by_stride(n):
    _sha(n, n, "scalar")


def test_sha256_chip_one_block_per_lane_by_alignment():
    _sha(257, _round64(257), "scalar", lead=1)


@pytest.mark.parametrize("form", ["x4", "scalar"])
def test_sha256_chip_without_timestamps(form):
    _sha(5, 64 if form == "x4" else 5, form, with_ts=False)


@pytest.mark.parametrize("stride", [4, 0])
def test_sha256_chip_refuses_a_stride_below_n(stride):
    blk, _ = _sha_case(5)
    out, ts = Buf(608 * 64, "<u4"), Buf(5, "<u8")
    d_blk = _dev(blk)
    rc = rt.lib().zkir_sha256_chip_launch(d_blk.data_ptr(), 5, out.ptr, stride, ts.ptr, _sp())
    torch.cuda.synchronize()
    assert rc == rt.ERR_ARGUMENT
    out.untouched("refused call: columns"); ts.untouched("refused call: timestamps")
