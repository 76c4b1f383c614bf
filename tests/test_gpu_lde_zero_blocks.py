"""zkir_lde_launch on matrices with all-zero column blocks: lde_run's first inverse LDS pass finds the zero blocks and the kernels after it skip them
(ntt.hip: the zero-block flags).  Width 24 = three B8 blocks at log_n 14, 16, 18, 20 — the R = 2, 3, 4, 5 instances of the strided kernel, 20 being the
benchmark's own pair — and at log_n 12, whose chain has no kernel that could find out: the path must be what it was.

`out` is pre-filled with 0xFFFFFFFF.  Every block of the result must equal the extension of that block run ALONE as a width-8 matrix (a lone non-zero
block cannot be skipped); zero blocks must come out as zeros.  At log_n <= 16 every column is also held against the oracle, at log_n 20 the single-word
columns are (as test_gpu_lde_wide.py does at that size).  Block kinds: Z zero, D seeded random, a block that is zero but for one word 1 at (row 0,
column 0) / (last row, column 7) / (a row of the first inverse pass's last tile, column 5), and a block whose plane 0 (columns 0-3) is zero and plane 1 random.
Flag lifetime: two different patterns back to back on one context, in both orders, and concurrently on two streams."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from oracle import stark_api as so

pytestmark = pytest.mark.gpu

P = 0x78000001
LOG_NS = [12, 14, 16, 18, 20]
ORACLE_ALL_MAX = 16                      # every column against the oracle up to here
ORACLE_WORD_AT = (20,)                   # ... and the single-word columns here
# the first inverse pass of these sizes takes log_n - 10 stages: its tiles are rows 1024 apart, and the LAST tile of a block holds the last 2^C (<= 32)
# positions of every run of 1024 — row 3 * 1024 + 1022 is one of its rows at every size
WORD_CASES = {"w_first": (0, 0), "w_last": (-1, 7), "w_last_tile_plane1": (3 * 1024 + 1022, 5)}
PATTERNS = ["ZDZ", "DZD", "ZZZ", "DDD", "Zw_firstD", "Zw_lastD", "Zw_last_tile_plane1D", "ZHD"]


def _kinds(pattern):
    """'ZDZ' -> ['Z', 'D', 'Z'];  'Zw_firstD' -> ['Z', 'w_first', 'D']"""
    if len(pattern) == 3:
        return list(pattern)
    return [pattern[0], pattern[1:-1], pattern[-1]]


class _Size:
    """One log_n: a context, the three seeded dense blocks, the special blocks, every block's extension run alone, and the oracle's columns where they are asked for"""

    def __init__(self, log_n):
        import torch
        from zkir_amd import stark
        self.log_n, self.n = log_n, 1 << log_n
        self.ctx = stark.StarkContext(log_n)
        self.host, self.dev, self.alone, self._oracle = {}, {}, {}, {}
        rng = np.random.default_rng(2700 + log_n)
        for b in range(3):
            self.host[("D", b)] = rng.integers(0, P, (self.n, 8), dtype=np.uint32)
        half = rng.integers(0, P, (self.n, 8), dtype=np.uint32)
        half[:, :4] = 0
        self.host[("H", 1)] = half
        for name, (row, col) in WORD_CASES.items():
            blk = np.zeros((self.n, 8), np.uint32)
            blk[row, col] = 1
            self.host[(name, 1)] = blk
        for key, blk in self.host.items():
            self.dev[key] = torch.from_numpy(blk.view(np.int32)).cuda()
            self.alone[key] = self.launch([self.dev[key]])[0]
            assert bool(self.alone[key].any()) and int(self.alone[key].max()) < P and int(self.alone[key].min()) >= 0, f"log_n {log_n}: block {key} alone"
        self.zero = torch.zeros((self.n, 8), dtype=torch.int32, device="cuda")

    def block(self, kind, b):
        return self.zero if kind == "Z" else self.dev[(kind, b)]

    def prepare(self, blocks):
        """(src, out) for one launch: the blocks stacked (the call clobbers its input) and an `out` that holds 0xFFFFFFFF everywhere"""
        import torch
        return torch.stack(list(blocks)).contiguous(), torch.full((len(blocks), 2 * self.n, 8), -1, dtype=torch.int32, device="cuda")

    def fire(self, src, out, stream=None):
        import torch
        from zkir_amd import pipeline as pl, runtime as rt
        s = stream or torch.cuda.current_stream()
        pl._check(rt.lib().zkir_lde_launch(self.ctx.handle, src.data_ptr(), src.shape[0] * 8, out.data_ptr(), C.c_void_p(s.cuda_stream)))
        return out

    def launch(self, blocks):
        src, out = self.prepare(blocks)
        out._src = src                                                 # stays alive as long as the result
        return self.fire(src, out)

    def oracle_columns(self, kind, b):
        """[8][2n] u32: the oracle's extension of the block's eight columns (all-zero columns: zeros, see test_oracle_extends_zero_to_zero)"""
        key = (kind, b)
        if key not in self._oracle:
            blk = self.host[key]
            want = np.zeros((8, 2 * self.n), np.uint32)
            for c in np.flatnonzero(blk.any(axis=0)):
                want[c] = so.lde(np.ascontiguousarray(blk[:, c]), 1)[1]
            self._oracle[key] = want
        return self._oracle[key]

    def check(self, out, pattern, what):
        import torch
        torch.cuda.synchronize()
        for b, kind in enumerate(_kinds(pattern)):
            if kind == "Z":
                assert not bool(out[b].any()), f"log_n {self.log_n}, {what} {pattern}: zero block {b} did not come out as zeros"
                continue
            assert torch.equal(out[b], self.alone[(kind, b)]), f"log_n {self.log_n}, {what} {pattern}: block {b} ({kind}) differs from the block extended alone"
            if self.log_n <= ORACLE_ALL_MAX or (self.log_n in ORACLE_WORD_AT and kind in WORD_CASES):
                got = out[b].cpu().numpy().view(np.uint32).T
                bad = np.flatnonzero((got != self.oracle_columns(kind, b)).any(axis=1))
                assert bad.size == 0, f"log_n {self.log_n}, {what} {pattern}: block {b} ({kind}) columns {bad.tolist()} differ from the oracle"

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module", params=LOG_NS)
def size(request):
    s = _Size(request.param)
    yield s
    s.close()


def test_oracle_extends_zero_to_zero():
    assert not so.lde(np.zeros(1 << 12, np.uint32), 1)[1].any()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_blocks_equal_blocks_alone(size, pattern):
    blocks = [size.block(kind, b) for b, kind in enumerate(_kinds(pattern))]
    size.check(size.launch(blocks), pattern, "pattern")


@pytest.mark.parametrize("order", [("ZDZ", "DZD"), ("DZD", "ZDZ")])
def test_back_to_back_on_one_context(size, order):
    outs = [size.launch([size.block(kind, b) for b, kind in enumerate(_kinds(p))]) for p in order]          # no synchronisation in between
    for p, out in zip(order, outs):
        size.check(out, p, "back to back")


def test_two_streams_of_one_context(size):
    import torch
    order = ("ZDZ", "DZD")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [size.prepare([size.block(kind, b) for b, kind in enumerate(_kinds(p))]) for p in order]
    torch.cuda.synchronize()                                           # the buffers were filled on the current stream
    outs = [size.fire(src, out, stream=st) for (src, out), st in zip(bufs, streams)]
    for st in streams:
        st.synchronize()
    for p, out in zip(order, outs):
        size.check(out, p, "two streams")
