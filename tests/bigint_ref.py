"""Big-integer reference for the field arithmetic of zkir_amd/csrc/babybear.h and poseidon2.h.

Plain Python ints, no product or oracle code.  Three layers:

* the EXACT integer contract of every bb:: primitive: the word it returns, with the 32/64-bit wraparound of the C++ (and of the gfx950
  instructions its device path is written in) modelled explicitly.  Signed words are handled as their two's-complement bit patterns.
  Every function is written with +, -, *, &, >>, comparisons and sel() only, so the same code also runs elementwise on numpy uint64
  arrays (whose arithmetic wraps modulo 2^64 exactly like the C++): that is how the tests check large random samples;
* each primitive's documented input domain and output bound, as data (PRIMS) the tests iterate over;
* the textbook objects: the field, the quartic extension F[X]/(X^4 - 11), Poseidon2-12 and its inverse round by round, and the
  radix-2 inverse-DIF stage map of the LDE with its inverse.
"""
from __future__ import annotations

P = (1 << 31) - (1 << 27) + 1
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
R = 1 << 32
NEG_PINV = (-pow(P, -1, R)) % R
R1 = R % P
R2 = R * R % P
RINV = pow(R, -1, P)
GEN = 31
W_EXT = 11


def sel(c, x, y):
    """x where c else y (a C++ ?: on one word, or numpy.where on arrays)."""
    if isinstance(c, bool):
        return x if c else y
    import numpy as np
    return np.where(c, x, y)


def sext(x):
    """32-bit pattern -> 64-bit pattern of the same signed value."""
    return x | (((x >> 31) & 1) * 0xFFFFFFFF00000000)


def signed(x, bits=32):
    """Bit pattern -> Python int (plain ints only)."""
    return x - (1 << bits) if x >> (bits - 1) else x


def u(x, bits=32):
    """Python int -> bit pattern."""
    return x & ((1 << bits) - 1)


# ---- the exact contract of each bb:: primitive -----------------------------------------------------------------------------------
def add(a, b):
    s = (a + b) & M32
    d = (s - P) & M32
    return sel(d < s, d, s)


def sub(a, b):
    d = (a - b) & M32
    e = (d + P) & M32
    return sel(e < d, e, d)


def neg(a):
    return sel(a != 0, (P - a) & M32, 0 * a)


def reduce_2p(x):
    d = (x - P) & M32
    return sel(d < x, d, x)


def _mont_tail(t):
    """(t + m p) >> 32 for a 64-bit t, m = t * (-p^-1) mod 2^32: the shared last two instructions of every Montgomery reduction."""
    m = ((t & M32) * NEG_PINV) & M32
    return (((t + m * P) & M64) >> 32) & M32


def mont_mul_lazy(a, b):
    return _mont_tail(a * b)


def mont_mul(a, b):
    return reduce_2p(mont_mul_lazy(a, b))


def mont_mul_add_lazy(a, b, c):
    return _mont_tail((a * b + c) & M64)


def mont_reduce_wide(acc):
    return _mont_tail(acc)


def mad_wide(k, acc, x):
    return (acc + k * x) & M64


def mulhi_u32(a, b):
    return ((a * b) >> 32) & M32


def reduce_wide_m(s):
    return (1 << (32 + s)) // P


def reduce_wide(s, acc):
    q = mulhi_u32((acc >> s) & M32, reduce_wide_m(s))
    return reduce_2p(((acc & M32) - q * P) & M32)


def _smont_tail(t):
    m = ((t & M32) * NEG_PINV) & M32
    return (((t + ((sext(m) * P) & M64)) & M64) >> 32) & M32


def smont_mul(a, b):
    return _smont_tail((sext(a) * sext(b)) & M64)


def smont_mul_add(a, b, c):
    return _smont_tail((((sext(a) * sext(b)) & M64) + c) & M64)


def smont_reduce_wide(acc):
    return _smont_tail(acc)


def sacc_add(acc, x):
    return (acc + sext(x)) & M64


def smad(k, acc, x):
    return (acc + (k & M64) * sext(x)) & M64


def mad96(lo, hi, x, y):
    """one term of a 96-bit sum: (lo, hi) + x y; returns the new (lo, hi)"""
    t = x * y
    s = (lo + t) & M64
    return s, sel(s < t, hi + 1, hi) & M32


def acc96_div_R(lo, hi):
    l0, l1 = lo & M32, (lo >> 32) & M32
    r0 = _mont_tail(l0)
    return reduce_wide(6, (hi * R1 + l1 + r0) & M64)


def acc96_sum(xs, ys):
    """the 96-bit sequence of mad96 steps over plain ints; returns (lo, hi)"""
    lo, hi = 0, 0
    for x, y in zip(xs, ys):
        lo, hi = mad96(lo, hi, x, y)
    return lo, hi


# ---- domains and bounds, as babybear.h documents them ----------------------------------------------------------------------------
# Every entry: the arguments' domains (half-open integer ranges, or a joint predicate), the bound the comment promises for the result,
# and the value the result must be congruent to.  Words are unsigned bit patterns; signed domains are given as signed ranges.
EDGE_U32 = [0, 1, 2, P - 2, P - 1, P, P + 1, 2 * P - 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, M32]


def edges_in(lo, hi, extra=()):
    return sorted({x for x in EDGE_U32 + list(extra) if lo <= x < hi} | {lo, hi - 1})


def _s(lo, hi, extra=()):
    """signed edges inside [lo, hi): +-(p-1), +-p, +-(p+128), 0, +-1, the int32 extremes and the ends of the range"""
    c = {0, 1, -1, P - 1, -(P - 1), P, -P, P + 128, -(P + 128), (1 << 31) - 1, -(1 << 31), lo, hi - 1, *extra}
    return sorted(x for x in c if lo <= x < hi)


def _mont_congruent(a, b, r):
    return (r - a * b * RINV) % P == 0


def _within_half_p(exact, r):
    """a signed Montgomery reduction: r 2^32 - exact = m p with |m| <= 2^31 (babybear.h: "within p / 2 of acc / 2^32")"""
    return abs(r * R - exact) <= P << 31


# `ok(*args, r)`: the output bound babybear.h states, exactly (r as a signed int for signed primitives)
PRIMS = {
    "add": dict(domain=[(0, P), (0, P)], ok=lambda a, b, r: r < P, congruent=lambda a, b, r: (r - a - b) % P == 0),
    "sub": dict(domain=[(0, P), (0, P)], ok=lambda a, b, r: r < P, congruent=lambda a, b, r: (r - a + b) % P == 0),
    "neg": dict(domain=[(0, P)], ok=lambda a, r: r < P, congruent=lambda a, r: (r + a) % P == 0),
    "reduce_2p": dict(domain=[(0, 2 * P)], ok=lambda x, r: r < P, congruent=lambda x, r: (r - x) % P == 0),
    # "mont_mul() accepts ONE operand below 2p when the other is canonical"
    "mont_mul": dict(domain=[(0, 2 * P), (0, 2 * P)], joint=lambda a, b: a < P or b < P, ok=lambda a, b, r: r < P, congruent=_mont_congruent),
    # "a, b < p -> result < 1.469 p;  a < 1.469 p, b < p -> result < 1.689 p": result < a b / 2^32 + p
    "mont_mul_lazy": dict(domain=[(0, 1469 * P // 1000), (0, P)], ok=lambda a, b, r: r * R < a * b + P * R and r * 1000 < 1689 * P, congruent=_mont_congruent),
    # "a < 2p, b < p, c < 2^34: the result is below a*b/2^32 + p + 4 (< 2p)"
    "mont_mul_add_lazy": dict(domain=[(0, 2 * P), (0, P), (0, 1 << 34)], ok=lambda a, b, c, r: r * R < a * b + (P + 4) * R and r < 2 * P,
                              congruent=lambda a, b, c, r: (r - (a * b + c) * RINV) % P == 0),
    # "acc + 2^32 p < 2^64 is all it needs": result below acc / 2^32 + p
    "mont_reduce_wide": dict(domain=[(0, (1 << 64) - (P << 32))], ok=lambda acc, r: r * R < acc + P * R, congruent=lambda acc, r: (r - acc * RINV) % P == 0),
    # "acc < 2^(32+S) and acc < 200 p": canonical residue
    "reduce_wide4": dict(domain=[(0, min(1 << 36, 200 * P))], ok=lambda acc, r: r < P, congruent=lambda acc, r: (r - acc) % P == 0),
    "reduce_wide6": dict(domain=[(0, min(1 << 38, 200 * P))], ok=lambda acc, r: r < P, congruent=lambda acc, r: (r - acc) % P == 0),
    "reduce_wide7": dict(domain=[(0, min(1 << 39, 200 * P))], ok=lambda acc, r: r < P, congruent=lambda acc, r: (r - acc) % P == 0),
    # acc + K x modulo 2^64, any 64-bit acc and 32-bit x
    "mad_wide1": dict(domain=[(0, 1 << 64), (0, 1 << 32)], ok=lambda acc, x, r: True, congruent=lambda acc, x, r: (r - acc - x) % (1 << 64) == 0),
    "mad_wide2": dict(domain=[(0, 1 << 64), (0, 1 << 32)], ok=lambda acc, x, r: True, congruent=lambda acc, x, r: (r - acc - 2 * x) % (1 << 64) == 0),
    "mulhi_u32": dict(domain=[(0, 1 << 32), (0, 1 << 32)], ok=lambda a, b, r: True, congruent=lambda a, b, r: r == a * b >> 32),
    # signed residues, "for |a b| < 2^31 p the product is again in (-p, p)"; the S-box inputs reach p + 128 (poseidon2.h)
    "smont_mul": dict(domain=[(-P - 128, P + 129), (-P - 128, P + 129)], signed=True, joint=lambda a, b: abs(a * b) < (1 << 31) * P,
                      ok=lambda a, b, r: _within_half_p(a * b, r) and abs(r) < P, congruent=lambda a, b, r: (r - a * b * RINV) % P == 0),
    # (a b + c) / R, c a 64-bit addend read as signed; the 64-bit sum must not wrap: |a b + c| + 2^31 p < 2^63
    "smont_mul_add": dict(domain=[(-P, P), (-P, P), (-(1 << 62), 1 << 62)], signed=True, joint=lambda a, b, c: abs(a * b + c) + (P << 31) < (1 << 63),
                          ok=lambda a, b, c, r: _within_half_p(a * b + c, r), congruent=lambda a, b, c, r: (r - (a * b + c) * RINV) % P == 0),
    # "the reductions take |acc| < 2^62"
    "smont_reduce_wide": dict(domain=[(-(1 << 62) + 1, 1 << 62)], signed=True, ok=lambda acc, r: _within_half_p(acc, r),
                              congruent=lambda acc, r: (r - acc * RINV) % P == 0),
    # acc + x modulo 2^64, x sign-extended
    "sacc_add": dict(domain=[(-(1 << 63), 1 << 63), (-(1 << 31), 1 << 31)], signed=True, ok=lambda acc, x, r: True,
                     congruent=lambda acc, x, r: (r - acc - x) % (1 << 64) == 0),
}
SMAD_K = [-2, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]      # the multipliers int_round_a uses: inline constants up to 64, scalar registers above
for _k in SMAD_K:
    PRIMS[f"smad{_k}"] = dict(domain=[(-(1 << 63), 1 << 63), (-(1 << 31), 1 << 31)], signed=True, ok=lambda acc, x, r: True,
                              congruent=(lambda k: lambda acc, x, r: (r - acc - k * x) % (1 << 64) == 0)(_k))

# The exact word each name returns, on unsigned bit patterns (signed arguments are passed as u32 / u64 patterns)
EXACT = {
    "add": add, "sub": sub, "neg": neg, "reduce_2p": reduce_2p, "mont_mul": mont_mul, "mont_mul_lazy": mont_mul_lazy,
    "mont_mul_add_lazy": mont_mul_add_lazy, "mont_reduce_wide": mont_reduce_wide,
    "reduce_wide4": lambda acc: reduce_wide(4, acc), "reduce_wide6": lambda acc: reduce_wide(6, acc), "reduce_wide7": lambda acc: reduce_wide(7, acc),
    "mad_wide1": lambda acc, x: mad_wide(1, acc, x), "mad_wide2": lambda acc, x: mad_wide(2, acc, x), "mulhi_u32": mulhi_u32,
    "smont_mul": smont_mul, "smont_mul_add": smont_mul_add, "smont_reduce_wide": smont_reduce_wide, "sacc_add": sacc_add,
}
for _k in SMAD_K:
    EXACT[f"smad{_k}"] = (lambda k: lambda acc, x: smad(k, acc, x))(_k)

# result width in bits (for reading a signed result back)
RESULT_BITS = {n: 64 if n.startswith(("mad_wide", "sacc_add", "smad")) else 32 for n in PRIMS}
# argument widths in bits (signed arguments are handed over as patterns of this width)
ARG_BITS = {n: [64 if (n in ("mont_reduce_wide", "smont_reduce_wide") or n.startswith(("reduce_wide", "mad_wide", "sacc_add", "smad")) and i == 0)
                or (n in ("mont_mul_add_lazy", "smont_mul_add") and i == 2) else 32 for i in range(len(PRIMS[n]["domain"]))] for n in PRIMS}


def edge_values(name, i):
    """the edge set of argument i of a primitive, inside its domain"""
    lo, hi = PRIMS[name]["domain"][i]
    if name.startswith("reduce_wide"):
        vals = {hi - 1, hi - 2, lo, lo + 1}
        for k in range(0, hi // P + 2):
            vals |= {k * P + d for d in range(-3, 4)}
        return sorted(v for v in vals if lo <= v < hi)
    if PRIMS[name].get("signed"):
        if ARG_BITS[name][i] == 64:
            extra = [a * (1 << 32) + b for a in (0, 1, -1, P, -P, 1 << 29, -(1 << 29)) for b in (0, 1, -1, P - 1, -(P - 1))]
            return _s(lo, hi, extra + [1 << 62, -(1 << 62) + 1, (1 << 63) - 1, -(1 << 63), (P << 32) + P - 1, -(P << 32)])
        return _s(lo, hi)
    if ARG_BITS[name][i] == 64:
        extra = [(1 << 32) - 1, 1 << 32, (1 << 34) - 1, (1 << 38) - 1, P * P, (2 * P - 1) * (P - 1), (1 << 63), M64, (1 << 64) - (P << 32) - 1]
        extra += [k * P + d for k in (1, 2, 64, 199, 1 << 20) for d in (-1, 0, 1)]
        extra += [(P - 1) << 32 | M32, ((2 * P - 1) * (P - 1)) + (1 << 34) - 1]
        return edges_in(lo, hi, extra)
    return edges_in(lo, hi, [1469 * P // 1000 - 1, 1469 * P // 1000])


def edge_cases(name):
    """cross product of the argument edge sets, restricted to the joint domain"""
    import itertools
    spec = PRIMS[name]
    sets = [edge_values(name, i) for i in range(len(spec["domain"]))]
    joint = spec.get("joint", lambda *a: True)
    return [args for args in itertools.product(*sets) if joint(*args)]


def check_result(name, args, r):
    """the documented bound and congruence of a result (args and r as signed ints for signed primitives); an error string or None"""
    spec = PRIMS[name]
    if not spec["ok"](*args, r):
        return f"{name}{tuple(args)} = {r}: outside the documented bound"
    if not spec["congruent"](*args, r):
        return f"{name}{tuple(args)} = {r}: wrong residue"
    return None


# ---- field, extension ------------------------------------------------------------------------------------------------------------
def fpow(a, e):
    return pow(a % P, e, P)


def finv(a):
    return pow(a % P, P - 2, P)


def to_mont(a):
    return a * R % P


def from_mont(a):
    return a * RINV % P


def e_mul(a, b):
    """product in F[X]/(X^4 - 11), canonical coefficients"""
    c = [0] * 7
    for i in range(4):
        for j in range(4):
            c[i + j] += a[i] * b[j]
    return [(c[k] + W_EXT * (c[k + 4] if k + 4 < 7 else 0)) % P for k in range(4)]


def e_pow(a, e):
    r, b = [1, 0, 0, 0], list(a)
    while e:
        if e & 1:
            r = e_mul(r, b)
        b = e_mul(b, b)
        e >>= 1
    return r


def e_inv(a):
    """a^(p^4 - 2): the inverse of a nonzero element (X^4 - 11 is irreducible), 0 for 0"""
    return e_pow(a, P ** 4 - 2)


def e_mul_m(a, b):
    """bb::e_mul_m: Montgomery-form coefficients in and out, canonical"""
    return [to_mont(x) for x in e_mul([from_mont(x) for x in a], [from_mont(x) for x in b])]


def e_inv_m(a):
    return [to_mont(x) for x in e_inv([from_mont(x) for x in a])]


def pow_contract(a, e):
    """bb::pow: canonical in and out"""
    return fpow(a, e)


def inv_contract(a):
    return fpow(a, P - 2)


# ---- Poseidon2-12 ----------------------------------------------------------------------------------------------------------------
T, RF, RP = 12, 8, 22
INV7 = pow(7, -1, P - 1)
M4 = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]]


def splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return state, z ^ (z >> 31)


def _constants():
    s = int.from_bytes(b"ZKIR-P2-", "big")
    out = []
    while len(out) < RF * T + RP:
        s, z = splitmix64(s)
        v = z >> 33
        if v < P:
            out.append(v)
    ext = [out[r * T:(r + 1) * T] for r in range(RF)]
    return ext, out[RF * T:]


EXT_RC, INT_RC = _constants()
EXT_M = [[M4[i % 4][j % 4] * (2 if i // 4 == j // 4 else 1) for j in range(T)] for i in range(T)]
INT_DIAG = [P - 2] + [1 << (i - 1) for i in range(1, T)]
INT_M = [[(1 + (INT_DIAG[i] if i == j else 0)) % P for j in range(T)] for i in range(T)]


def mat_inv(m):
    n = len(m)
    a = [[x % P for x in row] + [int(i == j) for j in range(n)] for i, row in enumerate(m)]
    for c in range(n):
        piv = next(i for i in range(c, n) if a[i][c])
        a[c], a[piv] = a[piv], a[c]
        f = finv(a[c][c])
        a[c] = [x * f % P for x in a[c]]
        for i in range(n):
            if i != c and a[i][c]:
                g = a[i][c]
                a[i] = [(x - g * y) % P for x, y in zip(a[i], a[c])]
    return [row[n:] for row in a]


def mat_vec(m, v):
    return [sum(x * y for x, y in zip(row, v)) % P for row in m]


EXT_M_INV = mat_inv(EXT_M)
INT_M_INV = mat_inv(INT_M)

# the 30 rounds in order: ("full", r) for r = 0..3, ("partial", r) for r = 0..21, ("full", r) for r = 4..7
ROUNDS = [("full", r) for r in range(RF // 2)] + [("partial", r) for r in range(RP)] + [("full", r) for r in range(RF // 2, RF)]


def sbox(x):
    return pow(x, 7, P)


def sbox_inv(x):
    return pow(x, INV7, P)


def apply_round(s, k):
    kind, r = ROUNDS[k]
    if kind == "full":
        return mat_vec(EXT_M, [sbox((x + c) % P) for x, c in zip(s, EXT_RC[r])])
    return mat_vec(INT_M, [sbox((s[0] + INT_RC[r]) % P)] + list(s[1:]))


def invert_round(s, k):
    kind, r = ROUNDS[k]
    if kind == "full":
        return [(sbox_inv(x) - c) % P for x, c in zip(mat_vec(EXT_M_INV, s), EXT_RC[r])]
    v = mat_vec(INT_M_INV, s)
    return [(sbox_inv(v[0]) - INT_RC[r]) % P] + v[1:]


def permute(state, upto=len(ROUNDS)):
    """textbook Poseidon2-12 (the initial external layer, then rounds 0 .. upto-1); permute(x) is the full permutation"""
    s = mat_vec(EXT_M, [x % P for x in state])
    for k in range(upto):
        s = apply_round(s, k)
    return s


def state_entering(state, k):
    """the state that enters round k (before its constants are added) when `state` is permuted"""
    return permute(state, k)


def input_for(entering, k):
    """the permutation input whose state entering round k is `entering`"""
    s = [x % P for x in entering]
    for j in range(k - 1, -1, -1):
        s = invert_round(s, j)
    return mat_vec(EXT_M_INV, s)


def compress(l, r):
    return permute(list(l) + list(r) + [0] * 4)[:4]


# ---- the LDE's inverse DIF stages --------------------------------------------------------------------------------------------------
# ntt_stage_kernel<false> / lde_small_kernel: stage s of 2^L points pairs positions (p, p + h), h = 2^(L-1-s), p = hi 2^(L-s) + lo, lo < h, and maps
#   (a, b) -> (a + b, (a - b) w^(lo 2^s)),  w = w_N^-1   (canonical values; natural order in, bit-reversed order out after L stages)
def root_of_unity(log_n):
    w = fpow(GEN, 15)                # primitive 2^27-th root of unity
    for _ in range(log_n, 27):
        w = w * w % P
    return w


def dif_stage(x, s, inverse=False):
    """stage s of the inverse DIF transform on a list of canonical values (inverse=True: undo it)"""
    n = len(x)
    L = n.bit_length() - 1
    h = n >> (s + 1)
    winv = finv(root_of_unity(L))
    half = (P + 1) // 2
    y = list(x)
    for blk in range(0, n, 2 * h):
        for lo in range(h):
            w = fpow(winv, lo << s)
            a, b = x[blk + lo], x[blk + lo + h]
            if not inverse:
                y[blk + lo], y[blk + lo + h] = (a + b) % P, (a - b) * w % P
            else:
                d = b * finv(w) % P
                y[blk + lo], y[blk + lo + h] = (a + d) * half % P, (a - d) * half % P
    return y


def lde_naive(evals, log_blowup=1):
    """the LDE by definition: the polynomial of degree < N through (w_N^j, evals[j]), evaluated on GEN * <w_(N 2^log_blowup)> in natural order"""
    n = len(evals)
    L = n.bit_length() - 1
    w = root_of_unity(L)
    ninv = finv(n)
    winv = finv(w)
    coeffs = [sum(e * fpow(winv, j * k % n) for j, e in enumerate(evals)) * ninv % P for k in range(n)]
    m = n << log_blowup
    wm = root_of_unity(L + log_blowup)
    out = []
    for i in range(m):
        x = GEN * fpow(wm, i) % P
        acc, xp = 0, 1
        for c in coeffs:
            acc += c * xp
            xp = xp * x % P
        out.append(acc % P)
    return out
