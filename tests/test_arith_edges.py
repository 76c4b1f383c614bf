"""Host build of the field arithmetic (babybear.h) and of Poseidon2 (poseidon2.h) at the edges of their documented domains, word for word against
the big-integer reference (tests/bigint_ref.py), which is itself pinned once against the oracle and the product's host permutation."""
from __future__ import annotations

import zlib

import numpy as np
import pytest

import arith_probe as ap
import bigint_ref as ref
from oracle import stark_api as so
from zkir_amd import runtime as rt

P = ref.P
N_RANDOM = 1 << 14


# ---- the reference against the oracle --------------------------------------------------------------------------------------------------
def test_reference_constants_and_permutation_match_oracle():
    ext, inn, diag = so.constants()
    assert ext.tolist() == ref.EXT_RC and inn.tolist() == ref.INT_RC and diag.tolist() == ref.INT_DIAG
    rng = np.random.default_rng(1)
    states = [rng.integers(0, P, 12).tolist() for _ in range(40)] + ap.edge_states()
    for s in states:
        want = so.permute(np.array(s, np.uint32)).tolist()
        assert ref.permute(s) == want, s
        got = np.array(s, np.uint32)
        rt.lib().zkir_poseidon2_permute(got.ctypes.data)                    # the product's host permutation
        assert got.tolist() == want, s
    # the inverse: every round undone, from every round
    s = states[0]
    for k in range(len(ref.ROUNDS) + 1):
        assert ref.input_for(ref.state_entering(s, k), k) == s


def test_reference_extension_matches_oracle():
    rng = np.random.default_rng(2)
    cases = [rng.integers(0, P, 4).tolist() for _ in range(50)] + [[P - 1] * 4, [1, 0, 0, 0], [0, 0, 0, 1], [0, P - 1, 0, P - 1]]
    for a in cases:
        b = rng.integers(0, P, 4).tolist()
        assert ref.e_mul(a, b) == so.emul(a, b).tolist()
        assert ref.e_inv(a) == so.einv(a).tolist()
        assert ref.e_mul(a, ref.e_inv(a)) == [1, 0, 0, 0]


def test_reference_stage_map_matches_oracle_ntt_and_lde():
    rng = np.random.default_rng(3)
    for L in (1, 2, 3, 5, 7):
        n = 1 << L
        x = rng.integers(0, P, n).tolist()
        y = list(x)
        for s in range(L):
            y = ref.dif_stage(y, s)
        # after the L stages: N x the inverse transform, in bit-reversed order
        inv = so.ntt(np.array(x, np.uint32), inverse=True).tolist()
        rev = [int(format(i, f"0{L}b")[::-1], 2) for i in range(n)]
        assert [y[rev[k]] for k in range(n)] == [v * n % P for v in inv]
        z = list(y)                                                         # and the stages undone one by one
        for s in range(L - 1, -1, -1):
            z = ref.dif_stage(z, s, inverse=True)
        assert z == x
        assert ref.lde_naive(x) == so.lde(np.array(x, np.uint32), 1)[1].tolist()


# ---- every primitive of the host build --------------------------------------------------------------------------------------------------
def _check_cases(name, slots, got, uarg=0, with_contract=True):
    want = ap.expected(name, slots, uarg)
    bad = np.nonzero(got[:, 0] != want)[0]
    assert not len(bad), f"{name}: {len(bad)} words differ from the reference, first at {ap.as_args(name, slots[bad[0]])}: {int(got[bad[0], 0]):#x} != {int(want[bad[0]]):#x}"
    if with_contract and name != "mulhi_u32":
        for row, r in zip(slots, got[:, 0]):
            err = ref.check_result(name, ap.as_args(name, row), ap.as_result(name, r))
            assert err is None, err


PRIM_NAMES = [n for n in ref.PRIMS if n != "mulhi_u32"]


@pytest.mark.parametrize("name", PRIM_NAMES)
def test_host_primitive_edges(name):
    cases = ref.edge_cases(name)
    slots = ap.to_slots(name, cases)
    _check_cases(name, slots, ap.host_elementwise(name, slots))


@pytest.mark.parametrize("name", PRIM_NAMES)
def test_host_primitive_random(name):
    slots = ap.random_slots(name, N_RANDOM, np.random.default_rng(zlib.crc32(name.encode()) + 7))
    got = ap.host_elementwise(name, slots)
    _check_cases(name, slots, got, with_contract=False)
    sub = slots[:512]
    _check_cases(name, sub, got[:512])


def test_host_mulhi_u32():
    a_vals = ref.edge_values("mulhi_u32", 0)
    for b in ref.edge_values("mulhi_u32", 1) + [ref.reduce_wide_m(s) for s in (4, 6, 7)]:
        slots = ap.to_slots("mulhi_u32", [(a, 0) for a in a_vals])
        _check_cases("mulhi_u32", slots, ap.host_elementwise("mulhi_u32", slots, b), b)
    rng = np.random.default_rng(5)
    b = int(rng.integers(0, 1 << 32))
    slots = ap.random_slots("mulhi_u32", N_RANDOM, rng)
    _check_cases("mulhi_u32", slots, ap.host_elementwise("mulhi_u32", slots, b), b)


# ---- 96-bit sums -----------------------------------------------------------------------------------------------------------------------
# (terms, largest operand): the documented "up to 2^9 terms" of ANY 32-bit words, mode 4's 712-constraint quotient and the DEEP sums (canonical operands, a
# Montgomery coefficient times a value), the barycentric sums (BARY_MAX_TERMS = 2^11 products below p^2)
ACC96_SHAPES = [(512, ref.M32), (712, P - 1), (2048, P - 1), (1, ref.M32), (2, ref.M32), (511, ref.M32)]


def acc96_inputs(terms, top, n, rng):
    """n sequences of `terms` products: the first four at the top of the range (a carry out of the low 64 bits on every step once the first
    term is in, for 32-bit operands), the rest random below `top`; xs [n][terms] (vector operand), xs4 [terms][4] and ys [n][terms]"""
    ys = rng.integers(0, top, (n, terms), dtype=np.uint64, endpoint=True).astype(np.uint32)
    xs = rng.integers(0, top, (n, terms), dtype=np.uint64, endpoint=True).astype(np.uint32)
    xs4 = rng.integers(0, top, (terms, 4), dtype=np.uint64, endpoint=True).astype(np.uint32)
    ys[:4] = top
    xs[:4] = top
    xs[0] = xs4[:, 0]
    xs4[:, 0] = top
    xs4[:, 1] = top - 1
    ys[1, 1::2] = top - 1
    return xs, xs4, ys


def check_acc96(variant, xs, xs4, ys, got):
    n, terms = ys.shape
    for i in range(n):
        rows = [xs[i]] if variant == 0 else [xs[0]] if variant == 1 else [xs4[:, k] for k in range(4)]
        for k, xrow in enumerate(rows):
            lo, hi = ref.acc96_sum([int(v) for v in xrow], [int(v) for v in ys[i]])
            exact = sum(int(a) * int(b) for a, b in zip(xrow, ys[i]))
            assert lo + (hi << 64) == exact and hi < 1 << 9
            assert (int(got[i, k, 0]), int(got[i, k, 1])) == (lo, hi), f"acc96 variant {variant} sum {i}.{k}: 96-bit sum differs"
            r = int(got[i, k, 2])
            assert r == ref.acc96_div_R(lo, hi) and r < P and (r * ref.R - exact) % P == 0, f"acc96_div_R variant {variant} sum {i}.{k}"


@pytest.mark.parametrize("terms,top", ACC96_SHAPES)
def test_host_acc96(terms, top):
    rng = np.random.default_rng(terms)
    xs, xs4, ys = acc96_inputs(terms, top, 8, rng)
    for variant in range(3):
        x = xs if variant == 0 else np.ascontiguousarray(np.broadcast_to(xs[0], (terms,))) if variant == 1 else xs4
        check_acc96(variant, xs, xs4, ys, ap.host_acc96(variant, x, ys))


# ---- extension field, pow, inv ---------------------------------------------------------------------------------------------------------
def ext_cases(rng, n_random):
    E = [0, 1, 2, P - 2, P - 1, ref.R1, (P - 1) // 2]
    out = [[a, b, c, d] for a in E for b in (0, P - 1) for c in (0, 1) for d in E[:3] + [P - 1]]
    out += rng.integers(0, P, (n_random, 4)).tolist()
    return out


def run_ext(runner, rng, n_random):
    a = ext_cases(rng, n_random)
    b = [a[(i * 7 + 3) % len(a)] for i in range(len(a))]
    slots = np.zeros((len(a), 4), np.uint64)
    for i in range(len(a)):
        for k in range(4):
            slots[i, k] = a[i][k] | (b[i][k] << 32)
    for name, fn in (("e_mul_m", lambda x, y: ref.e_mul_m(x, y)), ("e_inv_m", lambda x, y: ref.e_inv_m(x))):
        got = runner(name, slots)
        for i in range(len(a)):
            r = [int(got[i, 0]) & ref.M32, int(got[i, 0]) >> 32, int(got[i, 1]) & ref.M32, int(got[i, 1]) >> 32]
            assert r == fn(a[i], b[i]), f"{name}({a[i]}, {b[i]})"
    exps = [0, 1, 2, 7, ref.INV7, P - 2, P - 1, P, (P - 1) // 2, (1 << 64) - 1, (1 << 63) + 5]
    xs = [0, 1, 2, P - 2, P - 1, ref.GEN, (P - 1) // 2] + rng.integers(0, P, max(n_random // 8, 1)).tolist()
    slots = np.array([[x, e, 0, 0] for x in xs for e in exps], np.uint64)
    got = runner("pow", slots)
    for (x, e, _, _), r in zip(slots.tolist(), got[:, 0].tolist()):
        assert r == ref.pow_contract(x, e), f"pow({x}, {e})"
    slots = np.array([[x, 0, 0, 0] for x in xs], np.uint64)
    got = runner("inv", slots)
    for x, r in zip(xs, got[:, 0].tolist()):
        assert r == ref.inv_contract(x) and (x == 0 or r * x % P == 1), f"inv({x})"


def test_host_extension_pow_inv():
    run_ext(lambda name, slots: ap.host_elementwise(name, slots), np.random.default_rng(9), 200)


# ---- Poseidon2, host formulations ------------------------------------------------------------------------------------------------------
def check_p2(states, canon, raw, fo, formulation, want=None):
    want = [ref.permute(s) for s in states] if want is None else want
    for i, s in enumerate(states):
        assert canon[i].tolist() == want[i], f"{formulation}: permutation of {s} differs from the reference"
        if raw is not None:
            for k in range(12):
                w = int(raw[i, k])
                assert w < P + 64 and (w - fo * want[i][k]) % P == 0, f"{formulation}: raw output word {k} = {w} of {s}"


def test_host_poseidon2_round_targeted():
    """permute_scaled (the hash kernels' formulation) and permute(), host builds, on inputs that make every round start from an extreme state"""
    sc = ap.scales()
    fo = ap.f_out(sc)
    cases = ap.round_targeted_inputs()
    states = [c[2] for c in cases] + ap.edge_states()
    want = [ref.permute(s) for s in states]
    arr = np.array(states, np.uint32)
    canon, raw = ap.host_p2(0, False, arr)
    check_p2(states, canon, raw, fo, "permute_scaled (host)", want)
    canon, raw = ap.host_p2(3, False, arr)
    check_p2(states, canon, None, fo, "permute (host)", want)
    # raw input words at the top of their documented ranges
    rows, canon_in = ap.raw_top_words(sc)
    canon, raw = ap.host_p2(0, True, np.array(rows, np.uint32))
    check_p2(canon_in, canon, raw, fo, "permute_scaled (host, raw words)")
