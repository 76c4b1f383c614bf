"""stark.lde against the oracle (oracle.stark_api.lde), byte for byte and every word canonical, at the inverse splits tests/test_gpu_lde_wide.py does not
reach: log_n 16 (a 6-stage LDS pass before the middle kernel), 18 (8 stages), 19 (6 + 3: an LDS pass, then a register pass with per-lane block factors) and
21 (8 + 3) — the smallest sizes at which an LDS inverse pass, whose twiddles do not depend on the tile when it starts at stage 0, is followed by a register pass
or a middle kernel whose twiddles carry the factor of their block (tests/test_lde_inverse_model.py pins the same bookkeeping on the CPU).  Width 8; inputs: all
p-1, alternating 0 / p-1, a single 1 in the last row, and one seeded random matrix."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import stark_api as so

pytestmark = pytest.mark.gpu

P = 0x78000001
WIDTH = 8


def _inputs(log_n):
    n = 1 << log_n
    pm1 = np.full(n, P - 1, np.uint32)
    alt = np.zeros(n, np.uint32)
    alt[1::2] = P - 1
    one_last = np.zeros(n, np.uint32)
    one_last[n - 1] = 1
    for name, col in (("all_pm1", pm1), ("alt_0_pm1", alt), ("one_last", one_last)):
        yield name, np.broadcast_to(col, (WIDTH, n)), so.lde(col, 1)[1][None, :]
    mat = np.random.default_rng(2000 + log_n).integers(0, P, (WIDTH, n), dtype=np.uint32)
    with ThreadPoolExecutor(WIDTH) as ex:
        want = np.stack(list(ex.map(lambda k: so.lde(mat[k], 1)[1], range(WIDTH))))
    yield "random", mat, want


@pytest.mark.parametrize("log_n", [16, 18, 19, 21])
def test_lde_equals_oracle(log_n):
    import torch
    from zkir_amd import stark
    n = 1 << log_n
    ctx = stark.StarkContext(log_n)
    try:
        for kind, mat, want in _inputs(log_n):
            out = stark.lde(ctx, stark.to_b8(torch.from_numpy(np.ascontiguousarray(mat).view(np.int32)).cuda()))
            got = stark.from_b8(out, WIDTH).cpu().numpy().view(np.uint32)
            del out
            assert got.shape == (WIDTH, 2 * n)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, f"log_n {log_n}, input {kind}: columns {bad[:8].tolist()} differ from the oracle"
            assert int(got.max()) < P, f"log_n {log_n}, input {kind}: a word is not canonical"
    finally:
        ctx.close()
