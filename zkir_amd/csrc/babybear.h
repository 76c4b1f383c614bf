// babybear.h — Baby Bear field (p = 2^31 - 2^27 + 1) and its quartic extension F[X]/(X^4 - 11), host + device.
//
// Self-defined prover stages (absent from the reference, parity unpinned).  Values at rest in HBM and
// in proofs are CANONICAL (0 <= x < p).  Multiplication uses Montgomery reduction with R = 2^32:
//     mont_mul(a, b) = a * b * R^-1 mod p
// so a canonical value times a constant stored in Montgomery form (c*R) gives the canonical product directly, and
// data*data products are done on values converted with to_mont()/from_mont() inside a kernel.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BB_HD __host__ __device__ __forceinline__
#else
#define BB_HD inline
#endif

namespace bb {

constexpr uint32_t P = 0x78000001u;          // 2013265921
constexpr uint32_t NEG_PINV = 0x77FFFFFFu;   // -p^-1 mod 2^32
constexpr uint32_t R1 = 0x0FFFFFFEu;         // 2^32 mod p   (Montgomery form of 1)
constexpr uint32_t R2 = 0x45DDDDE3u;         // 2^64 mod p
constexpr uint32_t GEN = 31u;                // multiplicative generator, LDE coset shift
constexpr uint32_t ROOT27 = 0x1A427A41u;     // 31^15: primitive 2^27-th root of unity
constexpr uint32_t W_EXT = 11u;              // X^4 = 11

// add/sub as (op, op, unsigned min): the wrong candidate always wraps around 2^32 and loses the min
BB_HD uint32_t add(uint32_t a, uint32_t b) { const uint32_t s = a + b, d = s - P; return d < s ? d : s; }
BB_HD uint32_t sub(uint32_t a, uint32_t b) { const uint32_t d = a - b, e = d + P; return e < d ? e : d; }
BB_HD uint32_t neg(uint32_t a) { return a ? P - a : 0u; }
BB_HD uint32_t dbl(uint32_t a) { return add(a, a); }
BB_HD uint32_t mont_mul(uint32_t a, uint32_t b) {
  const uint64_t t = (uint64_t)a * b;
  const uint32_t m = (uint32_t)t * NEG_PINV;
  const uint32_t u = (uint32_t)((t + (uint64_t)m * P) >> 32);     // < 2p
  const uint32_t d = u - P;                                       // wraps above u when u < p
  return d < u ? d : u;                                           // min(u, u - p): 32-bit ops only
}
// ---- lazy helpers (gfx950: v_add/v_sub issue in ~2.3 cycles per wave, v_min/v_mul*/v_mad_u64 in ~4.2-4.5, measured with
// scripts/ubench_alu.hip; a modular add is add+add+min = 8.7 cycles, so hot loops skip the reduction where a value only
// feeds a Montgomery multiplication or a 64-bit accumulation) -------------------------------------------------------
// mont_mul() accepts ONE operand below 2p when the other is canonical: t + m*p < 2p^2 + 2^32 p < 2^64 and u < 2p still holds.
// add_lazy / sub_lazy: unreduced sum / difference of canonical values, below 2p — only ever that lazy operand of a product.
BB_HD uint32_t add_lazy(uint32_t a, uint32_t b) { return a + b; }
BB_HD uint32_t sub_lazy(uint32_t a, uint32_t b) { return a - b + P; }
BB_HD uint32_t reduce_2p(uint32_t x) { const uint32_t d = x - P; return d < x ? d : x; }       // [0, 2p) -> [0, p)
// Montgomery product WITHOUT the final conditional subtraction: result < a*b/2^32 + p.  With p/2^32 = 0.46875:
//   a, b < p            -> result < 1.469 p
//   a < 1.469 p, b < p  -> result < 1.689 p          (needs a*b + 2^32 p < 2^64 and the result below 2^32 = 2.133 p: both hold)
BB_HD uint32_t mont_mul_lazy(uint32_t a, uint32_t b) {
  const uint64_t t = (uint64_t)a * b;
  const uint32_t m = (uint32_t)t * NEG_PINV;
  return (uint32_t)((t + (uint64_t)m * P) >> 32);
}
// (a*b + c) / R mod p, lazy: the 64-bit multiply-add takes the addend for free, so mont(a, b) + c/R costs the three instructions
// of the product alone.  a < 2p, b < p, c < 2^34: a*b + c + 2^32 p < 2^64 and the result is below a*b/2^32 + p + 4 (< 2p).
BB_HD uint32_t mont_mul_add_lazy(uint32_t a, uint32_t b, uint64_t c) {
  const uint64_t t = (uint64_t)a * b + c;
  const uint32_t m = (uint32_t)t * NEG_PINV;
  return (uint32_t)((t + (uint64_t)m * P) >> 32);
}
// acc + K*x in 64 bits as ONE full-rate instruction on the device (v_mad_u64_u32 with an inline-constant multiplier);
// takes the 32-bit x as it is, no zero-extended register pair needed
template <int K>
BB_HD uint64_t mad_wide(uint64_t acc, uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint64_t r;
  asm("v_mad_u64_u32 %0, vcc, %1, %3, %2" : "=v"(r) : "v"(x), "v"(acc), "n"(K) : "vcc");
  return r;
#else
  return acc + (uint64_t)K * x;
#endif
}
BB_HD uint64_t acc_add(uint64_t acc, uint32_t x) { return mad_wide<1>(acc, x); }
// canonical residue of a small multiple of p held in 64 bits: acc < 2^(32+S) and acc < 200 p.  With M = floor(2^(32+S) / p)
// (34 for S = 4, 136 for S = 6) the estimate q = floor((acc >> S) * M / 2^32) never exceeds Q = floor(acc / p) and falls
// short of acc / p by less than Q * 0.0039 + 2^-20 < 1, so q is Q or Q - 1: the remainder candidate is below 2p and fits 32 bits.
// (The device multiply is spelled as an instruction: written in C++, LLVM proves acc >> S fits 32 bits, drops the truncation
// and then emits a 64 x 32-bit product with a dead high half: two extra instructions per reduction.)
BB_HD uint32_t mulhi_u32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r;
  asm("v_mul_hi_u32 %0, %1, %2" : "=v"(r) : "v"(a), "s"(b));
  return r;
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}
template <int S>
BB_HD uint32_t reduce_wide(uint64_t acc) {
  constexpr uint32_t M = (uint32_t)((1ull << (32 + S)) / P);
  const uint32_t q = mulhi_u32((uint32_t)(acc >> S), M);
  return reduce_2p((uint32_t)acc - q * P);
}
// ---- 96-bit accumulation of plain integer products (round 4: the constraint combination, the DEEP sums, the barycentric dot products) ----
// A sum of products  x_i * y_i  (x_i, y_i ANY 32-bit words: canonical, lazy, Montgomery ...) is formed as an exact 96-bit integer — one 64-bit
// multiply-add with carry-out plus one add-with-carry per term (a multiplier-class + a full-rate instruction, ~6.8 SIMD-cycles per wave64 against the
// ~17 of a lazy Montgomery product added into a 64-bit sum) — and reduced ONCE at the end.  acc96_div_R returns  (sum / 2^32) mod p, canonical: for
// Montgomery-form operands (x R, y R) that is the Montgomery form R * sum(x y) of the sum.  Up to 2^9 terms (hi < 2^9: the reduction's bound).
struct Acc96 { uint64_t lo; uint32_t hi; };
BB_HD Acc96 acc96_zero() { return Acc96{0, 0}; }
#if defined(__HIP_DEVICE_COMPILE__)
// x in a scalar register (a per-proof constant: alpha^c, gamma^k), y in a vector register
__device__ __forceinline__ void mad96_s(Acc96& a, uint32_t x, uint32_t y) {
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc" : "+v"(a.lo), "+v"(a.hi) : "s"(x), "v"(y) : "vcc");
}
// four sums at once (the coordinates of an extension-field coefficient times one value): ONE asm statement, so the compiler pads it with hazard
// nops once, not four times
__device__ __forceinline__ void mad96x4_s(Acc96* a, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t y) {
  asm("v_mad_u64_u32 %0, vcc, %8, %12, %0\n\tv_addc_co_u32 %4, vcc, 0, %4, vcc\n\t"
      "v_mad_u64_u32 %1, vcc, %9, %12, %1\n\tv_addc_co_u32 %5, vcc, 0, %5, vcc\n\t"
      "v_mad_u64_u32 %2, vcc, %10, %12, %2\n\tv_addc_co_u32 %6, vcc, 0, %6, vcc\n\t"
      "v_mad_u64_u32 %3, vcc, %11, %12, %3\n\tv_addc_co_u32 %7, vcc, 0, %7, vcc"
      : "+v"(a[0].lo), "+v"(a[1].lo), "+v"(a[2].lo), "+v"(a[3].lo), "+v"(a[0].hi), "+v"(a[1].hi), "+v"(a[2].hi), "+v"(a[3].hi)
      : "s"(x0), "s"(x1), "s"(x2), "s"(x3), "v"(y) : "vcc");
}
__device__ __forceinline__ void mad96(Acc96& a, uint32_t x, uint32_t y) {
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc" : "+v"(a.lo), "+v"(a.hi) : "v"(x), "v"(y) : "vcc");
}
#else
inline void mad96(Acc96& a, uint32_t x, uint32_t y) { const uint64_t t = (uint64_t)x * y, s = a.lo + t; a.hi += s < t; a.lo = s; }
inline void mad96_s(Acc96& a, uint32_t x, uint32_t y) { mad96(a, x, y); }
inline void mad96x4_s(Acc96* a, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t y) { mad96(a[0], x0, y); mad96(a[1], x1, y); mad96(a[2], x2, y); mad96(a[3], x3, y); }
#endif
BB_HD uint32_t acc96_div_R(const Acc96& a) {          // (hi 2^64 + lo) / 2^32 mod p = hi R + lo_hi + lo_lo / R; hi < 2^9
  const uint32_t l0 = (uint32_t)a.lo, l1 = (uint32_t)(a.lo >> 32);
  const uint32_t m = l0 * NEG_PINV;
  const uint32_t r0 = (uint32_t)(((uint64_t)l0 + (uint64_t)m * P) >> 32);      // l0 / R mod p, at most p
  return reduce_wide<6>((uint64_t)a.hi * R1 + l1 + r0);                         // < 2^37 + 2^33: inside reduce_wide<6>'s bounds (2^38, 200 p)
}

// acc / R mod p for a 64-bit acc (Montgomery reduction of a wide sum): two instructions against the six of reduce_wide; the result
// is below acc / 2^32 + p, i.e. "canonical + a little" for the acc < 2^38 sums of the Poseidon2 linear layers, and carries the factor
// 1/R, which the caller has to account for.  acc + 2^32 p < 2^64 is all it needs.
BB_HD uint32_t mont_reduce_wide(uint64_t acc) {
  const uint32_t m = (uint32_t)acc * NEG_PINV;
  return (uint32_t)((acc + (uint64_t)m * P) >> 32);
}
// ---- SIGNED Montgomery arithmetic (the Poseidon2 throughput kernels) ---------------------------------------------------------
// Operands are int32 residues in (-p, p).  With m = t * (-p^-1) mod 2^32 read as a SIGNED word, (t + m p) / 2^32 lies within p/2 of
// t / 2^32, so for |a b| < 2^31 p the product is again in (-p, p) (|r| < |a b| / 2^32 + p / 2 <= 0.469 p + 0.5 p) WITHOUT any
// conditional subtraction: chains of products (the x^7 S-box) cost their three multiplier instructions each and nothing else.
// The 64-bit sums are formed modulo 2^64 (no signed overflow in C++); only the high word of the exact multiple of 2^32 is kept.
BB_HD int32_t smont_mul(int32_t a, int32_t b) {
  const int64_t t = (int64_t)a * b;
  const int32_t m = (int32_t)((uint32_t)t * NEG_PINV);
  return (int32_t)(((uint64_t)t + (uint64_t)((int64_t)m * (int64_t)P)) >> 32);
}
// (a b + c) / R: c a 64-bit addend (|a b + c| / 2^32 + p / 2 bounds the result; c = p 2^32 + .. biases it into (0, 2p) for unsigned use)
BB_HD int32_t smont_mul_add(int32_t a, int32_t b, uint64_t c) {
  const uint64_t t = (uint64_t)((int64_t)a * b) + c;
  const int32_t m = (int32_t)((uint32_t)t * NEG_PINV);
  return (int32_t)((t + (uint64_t)((int64_t)m * (int64_t)P)) >> 32);
}
// acc / R for a signed 64-bit sum: within p / 2 of acc / 2^32
BB_HD int32_t smont_reduce_wide(int64_t acc) {
  const int32_t m = (int32_t)((uint32_t)acc * NEG_PINV);
  return (int32_t)(((uint64_t)acc + (uint64_t)((int64_t)m * (int64_t)P)) >> 32);
}
// acc + x with x sign-extended by the instruction (v_mad_i64_i32 with the inline multiplier 1)
BB_HD int64_t sacc_add(int64_t acc, int32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  int64_t r;
  asm("v_mad_i64_i32 %0, vcc, %1, 1, %2" : "=v"(r) : "v"(x), "v"(acc) : "vcc");
  return r;
#else
  return acc + x;
#endif
}
// ---- WIDE signed butterflies (the forward DIT passes of the LDE, ntt.hip) ------------------------------------------------------
// A DIT butterfly multiplies BEFORE it adds, so its sums can be formed in 64 bits by the multiply-add itself and reduced afterwards:
//     a + b w / R  =  (a ONE + b w) / R,   ONE = R mod p,
// one v_mad_i64_i32 per term and a 2-instruction signed Montgomery reduction per result, with no conditional subtraction anywhere.
// State words are int32 residues of ANY magnitude below 2^31 (canonical words included); twiddles are Montgomery-form and CENTRED,
// |w| <= (p - 1) / 2.  The products are spelled as instructions on the device: written as (int64_t)a * b + c, clang proves signs where it
// can and emits unsigned products plus corrections.
constexpr int32_t W_ONE = (int32_t)R1;              // 2^28 - 2
constexpr int32_t W_HALF = (int32_t)((P - 1) / 2);  // largest centred twiddle
BB_HD int64_t wmul(int32_t a, int32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  int64_t r;
  asm("v_mad_i64_i32 %0, vcc, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b) : "vcc");
  return r;
#else
  return (int64_t)a * b;
#endif
}
BB_HD int64_t wmad(int64_t acc, int32_t a, int32_t b) {       // acc + a b
#if defined(__HIP_DEVICE_COMPILE__)
  int64_t r;
  asm("v_mad_i64_i32 %0, vcc, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(acc) : "vcc");
  return r;
#else
  return (int64_t)((uint64_t)acc + (uint64_t)((int64_t)a * b));
#endif
}
// the same with a compile-time multiplier held in a scalar register (ONE, P)
template <int32_t K>
BB_HD int64_t wmulk(int32_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
  int64_t r;
  asm("v_mad_i64_i32 %0, vcc, %1, %2, 0" : "=v"(r) : "v"(a), "s"(K) : "vcc");
  return r;
#else
  return (int64_t)a * K;
#endif
}
template <int32_t K>
BB_HD int64_t wmadk(int64_t acc, int32_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
  int64_t r;
  asm("v_mad_i64_i32 %0, vcc, %1, %2, %3" : "=v"(r) : "v"(a), "s"(K), "v"(acc) : "vcc");
  return r;
#else
  return (int64_t)((uint64_t)acc + (uint64_t)((int64_t)a * K));
#endif
}
// acc / R: smont_reduce_wide with its multiply-add spelled out.  Needs |acc| < 2^63 - 2^31 p; |result| < |acc| / 2^32 + p / 2 + 1.
BB_HD int32_t wredc(int64_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int32_t m = (int32_t)((uint32_t)acc * NEG_PINV);
  return (int32_t)((uint64_t)wmadk<(int32_t)P>(acc, m) >> 32);
#else
  return smont_reduce_wide(acc);
#endif
}
// canonical [0, p) -> centred [-(p-1)/2, (p-1)/2], and (-p, p) -> canonical: add / min only, nothing a compiler turns into a select
BB_HD int32_t centre(uint32_t w) { const uint32_t u = w + (uint32_t)W_HALF, d = u - P; return (int32_t)((d < u ? d : u) - (uint32_t)W_HALF); }
BB_HD uint32_t wcanon(int32_t x) { const uint32_t u = (uint32_t)x, s = u + P; return s < u ? s : u; }
// mont_mul(a, b) centred, for canonical a, b: the bias (p-1)/2 rides in as the 64-bit addend of the product, so the one conditional subtraction a canonical
// product needs anyway lands in [0, p) around the bias.  a b + 2^32 (p-1)/2 + 2^32 p < 2^64, and the high word is in [(p-1)/2, 1.97 p).
// (The device products are spelled as instructions taking the 32-bit operands as they are: from (uint64_t)a * b the compiler hoists the zero-extended PAIR of a
// loop-invariant operand out of the loop and holds two registers for it.)
BB_HD int32_t mont_mul_centred(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint64_t t, u;
  asm("v_mad_u64_u32 %0, vcc, %1, %2, %3" : "=v"(t) : "v"(a), "v"(b), "s"((uint64_t)(uint32_t)W_HALF << 32) : "vcc");
  const uint32_t m = (uint32_t)t * NEG_PINV;
  asm("v_mad_u64_u32 %0, vcc, %1, %2, %3" : "=v"(u) : "v"(m), "s"(P), "v"(t) : "vcc");
  return (int32_t)(reduce_2p((uint32_t)(u >> 32)) - (uint32_t)W_HALF);
#else
  return (int32_t)(reduce_2p(mont_mul_add_lazy(a, b, (uint64_t)(uint32_t)W_HALF << 32)) - (uint32_t)W_HALF);
#endif
}
// one radix-2 DIT butterfly: (a, b) -> (a + b w / R, a - b w / R), nw = -w.  3 multiply-adds + 2 reductions = 7 instructions
BB_HD void dit2w(int32_t& a, int32_t& b, int32_t w, int32_t nw) {
  const int64_t A = wmulk<W_ONE>(a);
  const int32_t b0 = b;
  a = wredc(wmad(A, b0, w)); b = wredc(wmad(A, b0, nw));
}
// the radix-4 DIT quad (two stages; twiddles w1 = w2^2 of the first, w2 and w2i = w2 j of the second, n* their negations; outputs placed as dit4 in ntt.hip
// places them).  The first stage's sums of the EVEN pair stay 64-bit and are the addends of the second stage's products; those of the odd pair are reduced, because
// they are multiplied.  (All four first-stage terms in one sum would not close: the outputs would grow to 8 p.)  10 multiply-adds + 6 reductions = 22 instructions.
BB_HD void dit4w(int32_t& x0, int32_t& x1, int32_t& x2, int32_t& x3, int32_t w1, int32_t n1, int32_t w2, int32_t n2, int32_t w2i, int32_t n2i) {
  const int64_t X0 = wmulk<W_ONE>(x0), X2 = wmulk<W_ONE>(x2);
  const int64_t y0 = wmad(X0, x1, w1), y1 = wmad(X0, x1, n1);
  const int32_t y2 = wredc(wmad(X2, x3, w1)), y3 = wredc(wmad(X2, x3, n1));
  x0 = wredc(wmad(y0, y2, w2)); x2 = wredc(wmad(y0, y2, n2));
  x1 = wredc(wmad(y1, y3, w2i)); x3 = wredc(wmad(y1, y3, n2i));
}
// The same quad on TWO columns sharing their twiddles, as the kernels run it.  On the device the multiply-adds of a step are ONE asm statement for both columns (the
// compiler pads every asm statement with a hazard nop of its own: ten statements per column would cost ten), the columns alternating so that no instruction waits for
// the one before it; the low-word products of the reductions stay in C++, where the low half of a 64-bit sum is a sub-register.
// (The asm path exists on the device only: tests/test_gpu_lde_wide.py exercises it through stark.lde against the oracle; tests/cpp/wide_quad_test.cpp covers the C++ path.)
BB_HD void dit4w2(int32_t* a, int32_t* b, int32_t w1, int32_t n1, int32_t w2, int32_t n2, int32_t w2i, int32_t n2i) {
#if defined(__HIP_DEVICE_COMPILE__)
  int64_t ay0, ay1, at2, at3, by0, by1, bt2, bt3;
  asm("v_mad_i64_i32 %1, vcc, %8, %18, 0\n\tv_mad_i64_i32 %5, vcc, %12, %18, 0\n\t"              // X0 (in y1's registers)
      "v_mad_i64_i32 %3, vcc, %10, %18, 0\n\tv_mad_i64_i32 %7, vcc, %14, %18, 0\n\t"             // X2 (in t3's)
      "v_mad_i64_i32 %0, vcc, %9, %16, %1\n\tv_mad_i64_i32 %4, vcc, %13, %16, %5\n\t"            // y0 = X0 + x1 w1
      "v_mad_i64_i32 %2, vcc, %11, %16, %3\n\tv_mad_i64_i32 %6, vcc, %15, %16, %7\n\t"           // t2 = X2 + x3 w1
      "v_mad_i64_i32 %1, vcc, %9, %17, %1\n\tv_mad_i64_i32 %5, vcc, %13, %17, %5\n\t"            // y1 = X0 - x1 w1
      "v_mad_i64_i32 %3, vcc, %11, %17, %3\n\tv_mad_i64_i32 %7, vcc, %15, %17, %7"                 // t3 = X2 - x3 w1
      : "=&v"(ay0), "=&v"(ay1), "=&v"(at2), "=&v"(at3), "=&v"(by0), "=&v"(by1), "=&v"(bt2), "=&v"(bt3)
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]), "v"(w1), "v"(n1), "s"(W_ONE) : "vcc");
  {
    const int32_t m0 = (int32_t)((uint32_t)at2 * NEG_PINV), m1 = (int32_t)((uint32_t)bt2 * NEG_PINV), m2 = (int32_t)((uint32_t)at3 * NEG_PINV), m3 = (int32_t)((uint32_t)bt3 * NEG_PINV);
    asm("v_mad_i64_i32 %0, vcc, %4, %8, %0\n\tv_mad_i64_i32 %1, vcc, %5, %8, %1\n\tv_mad_i64_i32 %2, vcc, %6, %8, %2\n\tv_mad_i64_i32 %3, vcc, %7, %8, %3"
        : "+v"(at2), "+v"(bt2), "+v"(at3), "+v"(bt3) : "v"(m0), "v"(m1), "v"(m2), "v"(m3), "s"((int32_t)P) : "vcc");
  }
  const int32_t ay2 = (int32_t)((uint64_t)at2 >> 32), ay3 = (int32_t)((uint64_t)at3 >> 32), by2 = (int32_t)((uint64_t)bt2 >> 32), by3 = (int32_t)((uint64_t)bt3 >> 32);
  int64_t au0, au1, bu0, bu1;                                  // the sums of outputs 0 and 1; those of 2 and 3 replace y0 and y1
  asm("v_mad_i64_i32 %0, vcc, %8, %12, %4\n\tv_mad_i64_i32 %2, vcc, %10, %12, %6\n\t"
      "v_mad_i64_i32 %1, vcc, %9, %14, %5\n\tv_mad_i64_i32 %3, vcc, %11, %14, %7\n\t"
      "v_mad_i64_i32 %4, vcc, %8, %13, %4\n\tv_mad_i64_i32 %6, vcc, %10, %13, %6\n\t"
      "v_mad_i64_i32 %5, vcc, %9, %15, %5\n\tv_mad_i64_i32 %7, vcc, %11, %15, %7"
      : "=&v"(au0), "=&v"(au1), "=&v"(bu0), "=&v"(bu1), "+v"(ay0), "+v"(ay1), "+v"(by0), "+v"(by1)
      : "v"(ay2), "v"(ay3), "v"(by2), "v"(by3), "v"(w2), "v"(n2), "v"(w2i), "v"(n2i) : "vcc");
  {
    const int32_t m0 = (int32_t)((uint32_t)au0 * NEG_PINV), m1 = (int32_t)((uint32_t)bu0 * NEG_PINV), m2 = (int32_t)((uint32_t)au1 * NEG_PINV), m3 = (int32_t)((uint32_t)bu1 * NEG_PINV);
    const int32_t m4 = (int32_t)((uint32_t)ay0 * NEG_PINV), m5 = (int32_t)((uint32_t)by0 * NEG_PINV), m6 = (int32_t)((uint32_t)ay1 * NEG_PINV), m7 = (int32_t)((uint32_t)by1 * NEG_PINV);
    asm("v_mad_i64_i32 %0, vcc, %8, %16, %0\n\tv_mad_i64_i32 %1, vcc, %9, %16, %1\n\tv_mad_i64_i32 %2, vcc, %10, %16, %2\n\tv_mad_i64_i32 %3, vcc, %11, %16, %3\n\t"
        "v_mad_i64_i32 %4, vcc, %12, %16, %4\n\tv_mad_i64_i32 %5, vcc, %13, %16, %5\n\tv_mad_i64_i32 %6, vcc, %14, %16, %6\n\tv_mad_i64_i32 %7, vcc, %15, %16, %7"
        : "+v"(au0), "+v"(bu0), "+v"(au1), "+v"(bu1), "+v"(ay0), "+v"(by0), "+v"(ay1), "+v"(by1)
        : "v"(m0), "v"(m1), "v"(m2), "v"(m3), "v"(m4), "v"(m5), "v"(m6), "v"(m7), "s"((int32_t)P) : "vcc");
  }
  a[0] = (int32_t)((uint64_t)au0 >> 32); a[1] = (int32_t)((uint64_t)au1 >> 32); a[2] = (int32_t)((uint64_t)ay0 >> 32); a[3] = (int32_t)((uint64_t)ay1 >> 32);
  b[0] = (int32_t)((uint64_t)bu0 >> 32); b[1] = (int32_t)((uint64_t)bu1 >> 32); b[2] = (int32_t)((uint64_t)by0 >> 32); b[3] = (int32_t)((uint64_t)by1 >> 32);
#else
  dit4w(a[0], a[1], a[2], a[3], w1, n1, w2, n2, w2i, n2i);
  dit4w(b[0], b[1], b[2], b[3], w1, n1, w2, n2, w2i, n2i);
#endif
}
// ---- the same quad for a MULTIPLY-FIRST natural -> bit-reversed (Cooley-Tukey) transform: the inverse side of the LDE ---------------------
// Two stages on x0..x3 at distances 0, d, 2d, 3d: the first pairs (x0, x2) and (x1, x3) with w1, the second (x0, x1) with w2 and (x2, x3) with w2i = w2 j, w1 = w2^2
// (the twiddle belongs to the BLOCK, not to the position inside it).  That is dit4w's arithmetic with x1 and x2 exchanged on the way in and on the way out: the
// pair that is only added (x0, x2 here) keeps its first-stage sums 64-bit, the pair that is multiplied (x1, x3) has them reduced — the same sums as in dit4w, so its
// bounds hold as they are (restated below).
BB_HD void ct4w(int32_t& x0, int32_t& x1, int32_t& x2, int32_t& x3, int32_t w1, int32_t n1, int32_t w2, int32_t n2, int32_t w2i, int32_t n2i) {
  dit4w(x0, x2, x1, x3, w1, n1, w2, n2, w2i, n2i);
}
BB_HD void ct4w2(int32_t* a, int32_t* b, int32_t w1, int32_t n1, int32_t w2, int32_t n2, int32_t w2i, int32_t n2i) {
  int32_t p[4] = {a[0], a[2], a[1], a[3]}, q[4] = {b[0], b[2], b[1], b[3]};
  dit4w2(p, q, w1, n1, w2, n2, w2i, n2i);
  a[0] = p[0]; a[1] = p[2]; a[2] = p[1]; a[3] = p[3]; b[0] = q[0]; b[1] = q[2]; b[2] = q[1]; b[3] = q[3];
}
// x g / R for a word in (-p, p) and a CANONICAL Montgomery-form factor g (the coset scale g^k / N between the two sides): one signed product and one reduction,
// the result again in (-p, p) — no conditional subtraction, no canonicalisation before the forward rounds.
BB_HD int32_t wscale(int32_t x, uint32_t g) { return wredc(wmul(x, (int32_t)g)); }
// four words (a lane's four columns of one position) times one factor: on the device the products are one asm statement and the reductions' multiply-adds another
BB_HD void wscale4(int32_t* x, uint32_t g) {
#if defined(__HIP_DEVICE_COMPILE__)
  int64_t t0, t1, t2, t3;
  asm("v_mad_i64_i32 %0, vcc, %4, %8, 0\n\tv_mad_i64_i32 %1, vcc, %5, %8, 0\n\tv_mad_i64_i32 %2, vcc, %6, %8, 0\n\tv_mad_i64_i32 %3, vcc, %7, %8, 0"
      : "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(g) : "vcc");
  const int32_t m0 = (int32_t)((uint32_t)t0 * NEG_PINV), m1 = (int32_t)((uint32_t)t1 * NEG_PINV), m2 = (int32_t)((uint32_t)t2 * NEG_PINV), m3 = (int32_t)((uint32_t)t3 * NEG_PINV);
  asm("v_mad_i64_i32 %0, vcc, %4, %8, %0\n\tv_mad_i64_i32 %1, vcc, %5, %8, %1\n\tv_mad_i64_i32 %2, vcc, %6, %8, %2\n\tv_mad_i64_i32 %3, vcc, %7, %8, %3"
      : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3) : "v"(m0), "v"(m1), "v"(m2), "v"(m3), "s"((int32_t)P) : "vcc");
  x[0] = (int32_t)((uint64_t)t0 >> 32); x[1] = (int32_t)((uint64_t)t1 >> 32); x[2] = (int32_t)((uint64_t)t2 >> 32); x[3] = (int32_t)((uint64_t)t3 >> 32);
#else
  for (int i = 0; i < 4; i++) x[i] = wscale(x[i], g);
#endif
}
// The bounds, computed: magnitudes through one butterfly / quad from words of at most `x`.
constexpr uint64_t WREDC_IN_MAX = (1ull << 63) - ((uint64_t)P << 31);                    // what a reduction takes: |acc| + 2^31 p < 2^63
constexpr uint64_t wredc_out_bound(uint64_t acc) { return (acc >> 32) + 1 + P / 2 + 1; }  // |acc| / 2^32 rounded up, + p / 2 + 1
struct WBound { uint64_t acc, out; };                                                     // largest reduction input, largest output word
constexpr WBound dit2w_bound(uint64_t x) { const uint64_t a = x * (uint64_t)W_ONE + x * (uint64_t)W_HALF; return WBound{a, wredc_out_bound(a)}; }
constexpr WBound dit4w_bound(uint64_t x) {
  const uint64_t s1 = x * (uint64_t)W_ONE + x * (uint64_t)W_HALF;                         // y0, y1 (kept wide) and the sums reduced to y2, y3
  const uint64_t s2 = s1 + wredc_out_bound(s1) * (uint64_t)W_HALF;                        // second-stage sums
  return WBound{s2, wredc_out_bound(s2)};
}
static_assert(dit4w_bound(1ull << 31).acc < WREDC_IN_MAX && dit2w_bound(1ull << 31).acc < WREDC_IN_MAX, "every sum of a quad on int32 words is a legal reduction input");
static_assert(dit4w_bound(1ull << 31).out < (1ull << 31) && dit2w_bound(1ull << 31).out < (1ull << 31), "any quad output (and any canonical word) is a legal quad input");
static_assert(dit4w_bound(P).out < P && dit2w_bound(P).out < P, "closure: words in (-p, p) -- canonical ones included -- stay in (-p, p), which is what wcanon() takes");
// ct4w is dit4w on permuted arguments: the sums kept 64-bit are the first-stage sums of the pair that is only added, the sums reduced are those that are multiplied
constexpr WBound ct4w_bound(uint64_t x) { return dit4w_bound(x); }
constexpr WBound wscale_bound(uint64_t x) { const uint64_t a = x * (uint64_t)(P - 1); return WBound{a, wredc_out_bound(a)}; }      // canonical factor: at most p - 1
static_assert(ct4w_bound(1ull << 31).acc < WREDC_IN_MAX && ct4w_bound(1ull << 31).out < (1ull << 31), "every sum of an inverse quad on int32 words is a legal reduction input, every output a legal input");
static_assert(ct4w_bound(P).out < P, "closure of the inverse rounds: canonical words and words in (-p, p) stay in (-p, p)");
static_assert(wscale_bound(P).acc < WREDC_IN_MAX && wscale_bound(P).out < P, "the coset scale of a word in (-p, p) is a word in (-p, p): the forward rounds take it as it is");

BB_HD uint32_t to_mont(uint32_t a) { return mont_mul(a, R2); }
BB_HD uint32_t from_mont(uint32_t a) { return mont_mul(a, 1u); }
// canonical * canonical -> canonical (two reductions; for cold paths)
BB_HD uint32_t mul(uint32_t a, uint32_t b) { return mont_mul(mont_mul(a, b), R2); }
BB_HD uint32_t pow(uint32_t a, uint64_t e) {          // canonical in/out
  uint32_t r = R1, b = to_mont(a);
  while (e) { if (e & 1) r = mont_mul(r, b); b = mont_mul(b, b); e >>= 1; }
  return from_mont(r);
}
BB_HD uint32_t inv(uint32_t a) { return pow(a, P - 2); }
BB_HD uint32_t root_of_unity(int log_n) { uint32_t w = ROOT27; for (int i = log_n; i < 27; i++) w = mul(w, w); return w; }

// ---- quartic extension; every coefficient in the SAME form (all canonical or all Montgomery) ----------------
struct E4 { uint32_t c[4]; };
BB_HD E4 e_add(const E4& a, const E4& b) { return E4{{add(a.c[0], b.c[0]), add(a.c[1], b.c[1]), add(a.c[2], b.c[2]), add(a.c[3], b.c[3])}}; }
BB_HD E4 e_sub(const E4& a, const E4& b) { return E4{{sub(a.c[0], b.c[0]), sub(a.c[1], b.c[1]), sub(a.c[2], b.c[2]), sub(a.c[3], b.c[3])}}; }
// Montgomery-form product (inputs and output in Montgomery form).  w11m = 11*R mod p.
BB_HD E4 e_mul_m(const E4& a, const E4& b) {
  constexpr uint32_t W11M = (uint32_t)((11ull * R1) % P);
  const uint32_t a0 = a.c[0], a1 = a.c[1], a2 = a.c[2], a3 = a.c[3], b0 = b.c[0], b1 = b.c[1], b2 = b.c[2], b3 = b.c[3];
  const uint32_t t4 = add(add(mont_mul(a1, b3), mont_mul(a2, b2)), mont_mul(a3, b1));
  const uint32_t t5 = add(mont_mul(a2, b3), mont_mul(a3, b2));
  const uint32_t t6 = mont_mul(a3, b3);
  E4 r;
  r.c[0] = add(mont_mul(a0, b0), mont_mul(W11M, t4));
  r.c[1] = add(add(mont_mul(a0, b1), mont_mul(a1, b0)), mont_mul(W11M, t5));
  r.c[2] = add(add(add(mont_mul(a0, b2), mont_mul(a1, b1)), mont_mul(a2, b0)), mont_mul(W11M, t6));
  r.c[3] = add(add(mont_mul(a0, b3), mont_mul(a1, b2)), add(mont_mul(a2, b1), mont_mul(a3, b0)));
  return r;
}
// E4 (any form) times a base-field scalar given in Montgomery form -> same form as `a`
BB_HD E4 e_mul_fm(const E4& a, uint32_t bm) { return E4{{mont_mul(a.c[0], bm), mont_mul(a.c[1], bm), mont_mul(a.c[2], bm), mont_mul(a.c[3], bm)}}; }
BB_HD E4 e_to_mont(const E4& a) { return E4{{to_mont(a.c[0]), to_mont(a.c[1]), to_mont(a.c[2]), to_mont(a.c[3])}}; }
BB_HD E4 e_from_mont(const E4& a) { return E4{{from_mont(a.c[0]), from_mont(a.c[1]), from_mont(a.c[2]), from_mont(a.c[3])}}; }
BB_HD E4 e_one_m() { return E4{{R1, 0, 0, 0}}; }
BB_HD E4 e_zero() { return E4{{0, 0, 0, 0}}; }
// inverse in Montgomery form via the norm to the quadratic subfield F[Y]/(Y^2 - 11), Y = X^2:
//   a = A(Y) + X*B(Y), A = a0 + a2 Y, B = a1 + a3 Y;  a * (A - X B) = A^2 - Y B^2 =: N in F[Y]/(Y^2-11);  N^-1 = conj(N)/(n0^2 - 11 n1^2)
BB_HD E4 e_inv_m(const E4& a) {
  constexpr uint32_t W11M = (uint32_t)((11ull * R1) % P);
  const uint32_t a0 = a.c[0], a1 = a.c[1], a2 = a.c[2], a3 = a.c[3];
  // A^2 = (a0^2 + 11 a2^2) + (2 a0 a2) Y ;  B^2 = (a1^2 + 11 a3^2) + (2 a1 a3) Y ;  Y*B^2 = 11*(2 a1 a3) + (a1^2 + 11 a3^2) Y
  const uint32_t A0 = add(mont_mul(a0, a0), mont_mul(W11M, mont_mul(a2, a2))), A1 = dbl(mont_mul(a0, a2));
  const uint32_t B0 = add(mont_mul(a1, a1), mont_mul(W11M, mont_mul(a3, a3))), B1 = dbl(mont_mul(a1, a3));
  const uint32_t n0 = sub(A0, mont_mul(W11M, B1)), n1 = sub(A1, B0);
  const uint32_t d = sub(mont_mul(n0, n0), mont_mul(W11M, mont_mul(n1, n1)));          // norm to F, Montgomery form
  // d^-1 in Montgomery form: pow over Montgomery values
  uint32_t r = R1, b = d; uint32_t e = P - 2;
  while (e) { if (e & 1) r = mont_mul(r, b); b = mont_mul(b, b); e >>= 1; }
  const uint32_t i0 = mont_mul(n0, r), i1 = neg(mont_mul(n1, r));                       // N^-1 = (n0 - n1 Y) / d
  // a^-1 = (A - X B) * N^-1, with (A - X B) = a0 - a1 X + a2 X^2 - a3 X^3 and N^-1 = i0 + i1 X^2
  const E4 conj{{a0, neg(a1), a2, neg(a3)}};
  const E4 ninv{{i0, 0, i1, 0}};
  return e_mul_m(conj, ninv);
}

}  // namespace bb
