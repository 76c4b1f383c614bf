"""stark.lde against the oracle (oracle.stark_api.lde), byte for byte, over every kernel combination of lde_run: the small kernel (log_n 9), the fused
middle as the last forward kernel (10), and each ntt_stage / ntt_reg / strided split of the forward chain (11 .. 15, 17, 20) — the forward side runs in
wide signed arithmetic on words in (-p, p) and must hand out canonical words whichever kernel comes last.  Widths 8 and 152; inputs: all p-1, all 0,
alternating 0 / p-1, a single 1 in the first, last and middle row, and seeded random columns."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import stark_api as so

pytestmark = pytest.mark.gpu

P = 0x78000001
LOG_NS = [9, 10, 11, 12, 13, 14, 15, 17, 20]
WIDTHS = [8, 152]
INPUTS = ["all_pm1", "all_zero", "alt_0_pm1", "one_first", "one_last", "one_middle", "random"]


def _column(kind, n):
    c = np.zeros(n, np.uint32)
    if kind == "all_pm1":
        c[:] = P - 1
    elif kind == "alt_0_pm1":
        c[1::2] = P - 1
    elif kind == "one_first":
        c[0] = 1
    elif kind == "one_last":
        c[n - 1] = 1
    elif kind == "one_middle":
        c[n // 2] = 1
    else:
        assert kind == "all_zero"
    return c


_random_cache = {}


def _random(log_n):
    """152 seeded random columns and their extensions; width 8 takes the first eight"""
    if log_n not in _random_cache:
        _random_cache.clear()                                          # one size at a time: 1.9 GB at 2^20
        mat = np.random.default_rng(1000 + log_n).integers(0, P, (max(WIDTHS), 1 << log_n), dtype=np.uint32)
        with ThreadPoolExecutor(16) as ex:
            want = np.stack(list(ex.map(lambda k: so.lde(mat[k], 1)[1], range(len(mat)))))
        _random_cache[log_n] = (mat, want)
    return _random_cache[log_n]


@pytest.mark.parametrize("log_n,width", [(l, w) for l in LOG_NS for w in WIDTHS])
def test_lde_equals_oracle(log_n, width):
    import torch
    from zkir_amd import stark
    n = 1 << log_n
    ctx = stark.StarkContext(log_n)
    try:
        for kind in INPUTS:
            if kind == "random":
                mat, want = _random(log_n)
                mat, want = mat[:width], want[:width]
            else:
                col = _column(kind, n)
                mat, want = np.broadcast_to(col, (width, n)), so.lde(col, 1)[1][None, :]
            out = stark.lde(ctx, stark.to_b8(torch.from_numpy(np.ascontiguousarray(mat).view(np.int32)).cuda()))
            got = stark.from_b8(out, width).cpu().numpy().view(np.uint32)
            del out
            assert got.shape == (width, 2 * n)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, f"log_n {log_n}, width {width}, input {kind}: columns {bad[:8].tolist()} differ from the oracle"
            assert int(got.max()) < P, f"log_n {log_n}, width {width}, input {kind}: a word is not canonical"
    finally:
        ctx.close()
