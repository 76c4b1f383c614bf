"""The yardstick of the blow-up 4 / 8 extension, checked against itself on the CPU: the oracle's so.lde(x, b) equals the extension by definition
(bigint_ref.lde_naive: interpolate over <w_N>, evaluate on 31 <w_(N 2^b)>) for b = 1, 2, 3 at log_n 1 .. 8, and the extensions nest — every second row of
the extension at b is the extension at b - 1, since w_M^2 = w_(M/2)."""
from __future__ import annotations

import numpy as np
import pytest

import bigint_ref as ref
from oracle import stark_api as so

P = 0x78000001


def _inputs(log_n):
    n = 1 << log_n
    rng = np.random.default_rng(40 + log_n)
    edge = np.zeros(n, np.uint32)
    edge[::2] = P - 1
    return [rng.integers(0, P, n, dtype=np.uint32), edge, np.full(n, P - 1, np.uint32)]


@pytest.mark.parametrize("log_n", range(1, 9))
def test_oracle_lde_is_the_extension_by_definition(log_n):
    for x in _inputs(log_n)[:1 if log_n > 4 else 3]:              # the definition costs N * (N + M) big-integer products: one (random) input from 2^5 rows on
        for b in (1, 2, 3):
            got = so.lde(x, b)[1]
            assert got.shape == (len(x) << b,) and int(got.max()) < P
            assert got.tolist() == ref.lde_naive([int(v) for v in x], b), f"log_n {log_n}, log_blowup {b}"


@pytest.mark.parametrize("log_n", range(1, 9))
def test_oracle_extensions_nest(log_n):
    for x in _inputs(log_n):
        ext = {b: so.lde(x, b)[1] for b in (1, 2, 3)}
        coeffs = [so.lde(x, b)[0] for b in (1, 2, 3)]
        assert np.array_equal(coeffs[0], coeffs[1]) and np.array_equal(coeffs[0], coeffs[2])      # the interpolant does not depend on the rate
        for b in (2, 3):
            assert np.array_equal(ext[b][::2], ext[b - 1]), f"log_n {log_n}: rows 0, 2, 4 .. at log_blowup {b} are not the extension at {b - 1}"
