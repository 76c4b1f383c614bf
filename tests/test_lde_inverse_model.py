"""The twiddle bookkeeping of the LDE's inverse side (zkir_amd/csrc/ntt.hip, "the inverse side"), on the CPU: a scalar model of the multiply-first
natural -> bit-reversed transform, split into passes exactly as run_strided_stages<false> and the middle kernel split it, every twiddle formed as the
kernels form it — a root of the compact table small_inv (order 1024) with a bit-reversed exponent, times tw_inv[brv_s0(hi) << ..] for the s0 high bits
that a tile, a lane's group or a chunk fixes — with the kernels' table indices (asserted inside the tables' sizes) and LDS row indices.  Compared with
the oracle's interpolation (oracle.stark_api.ntt, inverse) for log_n 10 .. 16 and for one hand-picked three-pass split that the launcher does not pick
below log_n 24: a register pass at stage 0, an LDS pass with tile factors (s0 = 2), the middle kernel (s0 = 6)."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import stark_api as so

P = 0x78000001
ROOT27 = 0x1A427A41


def _mul(a, b):
    return (np.asarray(a, np.uint64) * np.asarray(b, np.uint64)) % np.uint64(P)


def _add(a, b):
    return (np.asarray(a, np.uint64) + np.asarray(b, np.uint64)) % np.uint64(P)


def _sub(a, b):
    return (np.asarray(a, np.uint64) + np.uint64(P) - np.asarray(b, np.uint64)) % np.uint64(P)


def _brv(x, bits):
    x = np.asarray(x, np.uint64)
    r = np.zeros_like(x)
    for i in range(bits):
        r |= ((x >> np.uint64(i)) & np.uint64(1)) << np.uint64(bits - 1 - i)
    return r


def _powers(w, n):
    out = np.empty(n, np.uint64)
    v = 1
    for i in range(n):
        out[i] = v
        v = v * w % P
    return out


class Tables:
    """LdeTables as zkir_stark_ctx builds them (plain field elements here): natural-order powers"""

    def __init__(self, L):
        self.L = L
        w = pow(ROOT27, 1 << (27 - L), P)
        self.tw_inv = _powers(pow(w, P - 2, P), 1 << (L - 1))                 # w_N^-k, k < N/2
        self.small_inv = _powers(pow(pow(ROOT27, 1 << 17, P), P - 2, P), 512)   # w_1024^-k, k < 512
        self.j = int(self.small_inv[256])                                     # the inverse 4th root
        self.r8 = int(self.small_inv[128])

    def tw(self, idx):
        idx = np.asarray(idx, np.int64)
        assert idx.min() >= 0 and idx.max() < len(self.tw_inv), "tw_inv index outside the table"
        return self.tw_inv[idx]

    def small(self, idx):
        idx = np.asarray(idx, np.int64)
        assert idx.min() >= 0 and idx.max() < 512, "small_inv index outside the table"
        return self.small_inv[idx]


def _quad(x0, x1, x2, x3, w1, w2, w2i):
    """stage one pairs (x0, x2), (x1, x3) with w1; stage two (x0, x1) with w2 and (x2, x3) with w2i"""
    t2, t3 = _mul(x2, w1), _mul(x3, w1)
    y0, y2, y1, y3 = _add(x0, t2), _sub(x0, t2), _add(x1, t3), _sub(x1, t3)
    u1, u3 = _mul(y1, w2), _mul(y3, w2i)
    return _add(y0, u1), _sub(y0, u1), _add(y2, u3), _sub(y2, u3)


def _bfly(a, b, w):
    t = _mul(b, w)
    return _add(a, t), _sub(a, t)


def lds_pass(x, t, s0, R, factor_shift_base, log_small=10):
    """ntt_strided_r4_kernel<false, R, ..> / the inverse rounds of lde_middle_r4_kernel: 2R stages on tiles of 2^(2R) rows (row distance stride_mid), R radix-4
    rounds; `factor_shift_base` - 2r is the shift of the uniform factor's table index (L - s0 - 2 for the strided pass, 8 for the middle kernel: the same number)"""
    L, n, B = t.L, 1 << t.L, 2 * R
    stride_mid = n >> (s0 + B)
    v = x.reshape(1 << s0, 1 << B, stride_mid).copy()
    hi = np.arange(1 << s0, dtype=np.uint64)
    e = _brv(hi, s0)
    for r in range(R):
        b = 2 * r
        lg = B - 2 - b
        h2 = 1 << lg
        qq = np.arange(1 << (B - 2), dtype=np.uint64)
        mid_lo, mid_hi = qq & np.uint64(h2 - 1), qq >> np.uint64(lg)
        i0 = ((mid_hi << np.uint64(lg + 2)) | mid_lo).astype(np.int64)
        sm = t.small(_brv(mid_hi, b) << np.uint64(log_small - (b + 2)))          # (lane, round)
        if s0 == 0:
            f = np.ones(1, np.uint64)                                           # the pass that starts at stage 0 reads no factor
        else:
            f = t.tw(e << np.uint64(factor_shift_base - b))                      # uniform over the tile / chunk
        w2 = _mul(f[:, None], sm[None, :])[:, :, None]                          # [hi, quad, 1]
        w1, w2i = _mul(w2, w2), _mul(w2, t.j)
        o = _quad(v[:, i0], v[:, i0 + h2], v[:, i0 + 2 * h2], v[:, i0 + 3 * h2], w1, w2, w2i)
        for k in range(4):
            v[:, i0 + k * h2] = o[k]
    return v.reshape(-1)


def reg_pass(x, t, s0, S):
    """ntt_reg_kernel<false, S>"""
    L, n = t.L, 1 << t.L
    d = n >> (s0 + S)
    v = x.reshape(1 << s0, 1 << S, d).copy()
    e = _brv(np.arange(1 << s0, dtype=np.uint64), s0)
    Tf = t.tw(e << np.uint64(L - s0 - S))[:, None]
    Tm = _mul(Tf, Tf)
    if S == 3:
        t0, m1 = _mul(Tm, Tm), _mul(Tm, t.j)
        for g in range(2):
            o = _quad(v[:, g], v[:, g + 2], v[:, g + 4], v[:, g + 6], t0, Tm, m1)
            for k in range(4):
                v[:, g + 2 * k] = o[k]
        wf = [Tf, _mul(Tf, t.j), _mul(Tf, t.r8), _mul(Tf, pow(t.r8, 3, P))]
        for m in range(4):
            v[:, 2 * m], v[:, 2 * m + 1] = _bfly(v[:, 2 * m], v[:, 2 * m + 1], wf[m])
    else:
        o = _quad(v[:, 0], v[:, 1], v[:, 2], v[:, 3], Tm, Tf, _mul(Tf, t.j))
        for k in range(4):
            v[:, k] = o[k]
    return v.reshape(-1)


def stage_pass(x, t, s0):
    """ntt_stage_kernel<false>"""
    L, n = t.L, 1 << t.L
    v = x.reshape(1 << s0, 2, n >> (s0 + 1)).copy()
    w = t.tw(_brv(np.arange(1 << s0, dtype=np.uint64), s0) << np.uint64(L - s0 - 1))[:, None]
    v[:, 0], v[:, 1] = _bfly(v[:, 0], v[:, 1], w)
    return v.reshape(-1)


def launcher_split(stages):
    """run_strided_stages: the passes that cover `stages` stages"""
    out = []
    while stages > 0:
        if stages >= 10 and stages != 11:
            take = 10
        elif stages == 11:
            take = 8
        elif stages == 9:
            take = 6
        elif stages == 7:
            take = 4
        elif stages == 5:
            take = 3
        else:
            take = stages
        out.append(take)
        stages -= take
    return out


def inverse_model(col, L, split=None):
    t = Tables(L)
    x = np.asarray(col, np.uint64)
    s0 = 0
    for take in (launcher_split(L - 10) if split is None else split):
        if take in (10, 8, 6, 4):
            x = lds_pass(x, t, s0, take // 2, L - s0 - 2)
        elif take in (3, 2):
            x = reg_pass(x, t, s0, take)
        else:
            assert take == 1
            x = stage_pass(x, t, s0)
        s0 += take
    assert s0 == L - 10
    # the middle kernel: s0 = L - 10, hi = the chunk; its factor index is brv(chunk) << (8 - 2r) = << (L - s0 - 2r - 2)
    if s0 == 0:
        x = lds_pass_middle(x, t)
    else:
        x = lds_pass(x, t, s0, 5, 8)
    # position p holds N * coefficient brv_L(p)
    k = _brv(np.arange(1 << L, dtype=np.uint64), L).astype(np.int64)
    coeffs = np.empty(1 << L, np.uint64)
    coeffs[k] = _mul(x, pow(1 << L, P - 2, P))
    return coeffs.astype(np.uint32)


def lds_pass_middle(x, t):
    """the middle kernel at log_n = 10 multiplies by its chunk factor tw_inv[0] = 1: the same numbers as a pass without one"""
    assert int(t.tw_inv[0]) == 1
    return lds_pass(x, t, 0, 5, 8)


def _columns(L):
    n = 1 << L
    rng = np.random.default_rng(4200 + L)
    one_last = np.zeros(n, np.uint32)
    one_last[n - 1] = 1
    alt = np.zeros(n, np.uint32)
    alt[1::2] = P - 1
    return [rng.integers(0, P, n, dtype=np.uint32), one_last, alt]


@pytest.mark.parametrize("log_n", [10, 11, 12, 13, 14, 15, 16])
def test_model_equals_oracle_interpolation(log_n):
    for col in _columns(log_n):
        want = so.ntt(col, inverse=True)
        got = inverse_model(col, log_n)
        assert np.array_equal(got, want), f"log_n {log_n}: {int((got != want).sum())} coefficients differ"


def test_three_pass_split():
    L = 16
    for col in _columns(L):
        want = so.ntt(col, inverse=True)
        got = inverse_model(col, L, split=[2, 4])          # register pass at stage 0, LDS pass at s0 = 2 (tile factors), middle at s0 = 6
        assert np.array_equal(got, want)


def test_launcher_split_covers_what_the_gpu_tests_name():
    assert [launcher_split(s) for s in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)] == [[1], [2], [3], [4], [3, 2], [6], [4, 3], [8], [6, 3], [10], [8, 3]]
