"""ctypes side of tests/hip/libzkir_arith_probe.so (tests/hip/arith_probe.hip) and the input sets the arithmetic edge tests share."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import bigint_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE = os.path.join(HERE, "hip", "libzkir_arith_probe.so")
_lib = None


def lib():
    """the probe library, built by zkir_amd.build (rebuilt here if it is missing); a missing library is a failure, never a skip"""
    global _lib
    if _lib is None:
        if not os.path.exists(PROBE):
            from zkir_amd import build as zbuild
            zbuild.build_probe()
        assert os.path.exists(PROBE), f"arith probe library missing: {PROBE}"
        L = C.CDLL(PROBE)
        V, U32, U64, I = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        L.zkir_probe_op_name.restype = C.c_char_p; L.zkir_probe_op_name.argtypes = [I]
        L.zkir_probe_elementwise.restype = I; L.zkir_probe_elementwise.argtypes = [I, I, V, U64, U32, V, V]
        L.zkir_probe_acc96.restype = I; L.zkir_probe_acc96.argtypes = [I, I, V, V, U32, U64, V, V]
        L.zkir_probe_p2_consts_size.restype = U64; L.zkir_probe_p2_consts_size.argtypes = []
        L.zkir_probe_p2_consts.restype = None; L.zkir_probe_p2_consts.argtypes = [V]
        L.zkir_probe_p2_scales.restype = None; L.zkir_probe_p2_scales.argtypes = [V]
        L.zkir_probe_p2.restype = I; L.zkir_probe_p2.argtypes = [I, I, I, V, V, U64, U32, V, V, V]
        _lib = L
    return _lib


def op_ids():
    out, k = {}, 0
    while (name := lib().zkir_probe_op_name(k)) is not None:
        out[name.decode()] = k
        k += 1
    return out


def scales():
    s = np.zeros(3, np.uint32)
    lib().zkir_probe_p2_scales(s.ctypes.data)
    return [int(x) for x in s]      # in_scale, out_scale, carry


def consts_bytes():
    b = np.zeros(lib().zkir_probe_p2_consts_size(), np.uint8)
    lib().zkir_probe_p2_consts(b.ctypes.data)
    return b


# ---- the host side of the entry points (numpy arrays) ---------------------------------------------------------------------------------
def host_elementwise(name, slots, uarg=0):
    """slots: uint64 [n][4] argument slots -> uint64 [n][2] results of the host build"""
    slots = np.ascontiguousarray(slots, np.uint64)
    out = np.zeros((len(slots), 2), np.uint64)
    assert lib().zkir_probe_elementwise(1, op_ids()[name], slots.ctypes.data, len(slots), uarg, out.ctypes.data, None) == 0
    return out


def host_acc96(variant, xs, ys):
    xs, ys = np.ascontiguousarray(xs, np.uint32), np.ascontiguousarray(ys, np.uint32)
    n, terms = ys.shape
    out = np.zeros((n, 4, 3), np.uint64)
    assert lib().zkir_probe_acc96(1, variant, xs.ctypes.data, ys.ctypes.data, terms, n, out.ctypes.data, None) == 0
    return out


def host_p2(form, raw, states):
    s = np.ascontiguousarray(states, np.uint32)
    canon, rawo = np.zeros_like(s), np.zeros_like(s)
    assert lib().zkir_probe_p2(1, form, int(raw), None, s.ctypes.data, len(s), 0, canon.ctypes.data, rawo.ctypes.data, None) == 0
    return canon, rawo


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def to_slots(name, cases):
    """argument tuples (signed ints for signed primitives) -> uint64 [n][4] slots (bit patterns of the argument widths); mulhi_u32 keeps its second
    argument out (it is the launch's uniform operand)"""
    bits = ref.ARG_BITS[name]
    out = np.zeros((len(cases), 4), np.uint64)
    for i, args in enumerate(cases):
        for k, (a, b) in enumerate(zip(args, bits)):
            out[i, k] = ref.u(a, b)
    return out


def random_slots(name, n, rng):
    """n seeded random argument vectors inside the primitive's domain, as uint64 [n][4] slots"""
    spec = ref.PRIMS[name]
    cols = []
    for k, (lo, hi) in enumerate(spec["domain"]):
        if name == "smont_mul_add" and k == 2:
            lo, hi = -(1 << 61), 1 << 61                    # |a b + c| < 2^62 + 2^61: inside the joint domain without a per-element test
        if lo < 0:
            v = rng.integers(lo, hi, n, dtype=np.int64).astype(np.uint64)
            if ref.ARG_BITS[name][k] == 32:
                v &= np.uint64(ref.M32)
        else:
            v = rng.integers(lo, hi - 1, n, dtype=np.uint64, endpoint=True)
        cols.append(v)
    if name == "mont_mul":                                  # one operand canonical
        swap = rng.integers(0, 2, n).astype(bool)
        cols[0] = np.where(swap, cols[0] % np.uint64(ref.P), cols[0])
        cols[1] = np.where(swap, cols[1], cols[1] % np.uint64(ref.P))
    out = np.zeros((n, 4), np.uint64)
    for k, c in enumerate(cols):
        out[:, k] = c
    return out


def expected(name, slots, uarg=0):
    """the reference's exact word for every row of slots (vectorized: the reference's functions run on numpy uint64 arrays)"""
    args = [slots[:, k].astype(np.uint64) for k in range(len(ref.PRIMS[name]["domain"]))]
    if name == "mulhi_u32":
        return np.asarray(ref.mulhi_u32(args[0], np.uint64(uarg)), np.uint64)
    with np.errstate(over="ignore"):
        return np.asarray(ref.EXACT[name](*args), np.uint64)


def as_args(name, row):
    """one row of slots -> the argument tuple as the domain reads it (signed ints for signed primitives)"""
    bits = ref.ARG_BITS[name]
    vals = [int(row[k]) for k in range(len(bits))]
    return tuple(ref.signed(v, b) if ref.PRIMS[name].get("signed") else v for v, b in zip(vals, bits))


def as_result(name, word):
    w = int(word)
    return ref.signed(w, ref.RESULT_BITS[name]) if ref.PRIMS[name].get("signed") else w


# Poseidon2 inputs ------------------------------------------------------------------------------------------------------------------------
def round_targets():
    """the states a round may be entered with: all 0, all 1, all p-1, all (p-1)/2, alternating 0 / p-1, one word p-1 (or 1) with the others 0"""
    P = ref.P
    out = [[0] * 12, [1] * 12, [P - 1] * 12, [(P - 1) // 2] * 12, [0, P - 1] * 6, [P - 1, 0] * 6]
    for i in range(12):
        for v in (P - 1, 1):
            t = [0] * 12
            t[i] = v
            out.append(t)
    return out


def round_targeted_inputs(rounds=None, targets=None):
    """(round, target, input) for every round k and target state: `input` makes the permutation enter round k with `target`"""
    targets = round_targets() if targets is None else targets
    rounds = range(len(ref.ROUNDS)) if rounds is None else rounds
    return [(k, t, ref.input_for(t, k)) for k in rounds for t in targets]


def edge_states():
    P = ref.P
    out = [[P - 1] * 12, [0] * 12, [1] * 12, list(range(12)), [P - 1, 0] * 6, [0, P - 1] * 6, [(P - 1) // 2] * 12, [P - 2] * 12, [1, P - 1] * 6]
    for i in range(12):
        t = [0] * 12
        t[i] = P - 1
        out.append(t)
    return out


def raw_top_words(scales_):
    """raw input words of permute_scaled at the top of the documented ranges (poseidon2.h: below 1.96 p for a word through `carry`, below p + 64 for
    an output word), mixed with 0, 1, p - 1, p; returns the rows of words and the canonical values they stand for (word = F_IN v, F_IN = in_scale / R)"""
    P = ref.P
    f_in_inv = ref.finv(scales_[0] * ref.RINV % P)
    tops = [196 * P // 100 - 1, 196 * P // 100 - 2, P + 63, P + 62, P, P - 1, 0, 1]
    rows = [[tops[(k + i) % len(tops)] for i in range(12)] for k in range(len(tops))]
    rows += [[tops[0]] * 12, [P + 63] * 12]
    return rows, [[w * f_in_inv % P for w in r] for r in rows]


def f_out(scales_):
    """F_OUT: the factor of the raw output words (out_scale = R / F_OUT)"""
    return ref.R * ref.finv(scales_[1]) % ref.P
