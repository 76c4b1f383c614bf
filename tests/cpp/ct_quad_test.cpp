// The multiply-first natural -> bit-reversed quad of babybear.h (ct4w / ct4w2: the LDE's inverse rounds) and the signed coset-scale product (wscale / wscale4),
// host side, against the canonical field arithmetic (bb::mul / bb::add / bb::sub) and against their documented bounds.  The words and twiddles are those of
// wide_quad_test.cpp.  Exits 0 and prints one summary line, or prints the first failure and exits 1.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../zkir_amd/csrc/babybear.h"

namespace {

typedef __int128 i128;
constexpr int32_t H = bb::W_HALF;
constexpr int64_t Pq = (int64_t)bb::P;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
int32_t rnd_word() { for (;;) { const int32_t v = (int32_t)(uint32_t)rnd(); if (v != INT32_MIN) return v; } }
int32_t rnd_twiddle() { return (int32_t)(rnd() % (uint64_t)(2 * (int64_t)H + 1)) - H; }

uint32_t canon(int64_t x) { int64_t r = x % Pq; if (r < 0) r += Pq; return (uint32_t)r; }
[[noreturn]] void fail(const char* what, const int32_t* x, const int32_t* w) {
  std::printf("FAIL %s: x = %d %d %d %d, w1 w2 w2i = %d %d %d\n", what, x[0], x[1], x[2], x[3], w[0], w[1], w[2]);
  std::exit(1);
}

uint64_t max_acc = 0;          // largest |reduction input| seen
uint64_t max_out = 0;          // largest |output word| seen
uint64_t n_quads = 0, n_scales = 0;

// a reduction whose input is re-derived exactly (128 bits) and held against the documented bound
int32_t checked_redc(i128 exact, int64_t acc, const int32_t* x, const int32_t* w) {
  if ((i128)acc != exact) fail("64-bit sum differs from the exact one (overflow)", x, w);
  const uint64_t mag = acc < 0 ? (uint64_t)(-acc) : (uint64_t)acc;
  if (mag >= bb::WREDC_IN_MAX) fail("reduction input out of bounds", x, w);
  if (mag > max_acc) max_acc = mag;
  const int32_t r = bb::wredc(acc);
  const int64_t lim = (int64_t)(mag >> 32) + 1 + Pq / 2 + 1;
  if ((int64_t)r >= lim || (int64_t)r <= -lim) fail("reduction output beyond |acc| / 2^32 + p / 2 + 1", x, w);
  if ((uint32_t)(((uint64_t)canon(r) << 32) % bb::P) != canon((int64_t)(exact % Pq))) fail("reduction is not acc / R", x, w);
  return r;
}

// one quad at positions 0, d, 2d, 3d of a block: stage one pairs (x0, x2) and (x1, x3) with w1, stage two (x0, x1) with w2 and (x2, x3) with w2i
void quad(const int32_t* x, const int32_t* w, int32_t* out) {
  n_quads++;
  // reference: canonical arithmetic; a Montgomery-form twiddle wm stands for the field element wm / R
  const uint32_t c0 = canon(x[0]), c1 = canon(x[1]), c2 = canon(x[2]), c3 = canon(x[3]);
  const uint32_t v1 = bb::from_mont(canon(w[0])), v2 = bb::from_mont(canon(w[1])), v2i = bb::from_mont(canon(w[2]));
  const uint32_t t2 = bb::mul(c2, v1), t3 = bb::mul(c3, v1);
  const uint32_t y0 = bb::add(c0, t2), y2 = bb::sub(c0, t2), y1 = bb::add(c1, t3), y3 = bb::sub(c1, t3);
  const uint32_t u1 = bb::mul(y1, v2), u3 = bb::mul(y3, v2i);
  const uint32_t want[4] = {bb::add(y0, u1), bb::sub(y0, u1), bb::add(y2, u3), bb::sub(y2, u3)};
  // the flow from the primitives, every accumulator against the exact integer: the sums of the pair that is only added (x0, x2) stay wide,
  // those of the pair that is multiplied (x1, x3) are reduced
  const int32_t n1 = -w[0], n2 = -w[1], n2i = -w[2];
  const int64_t X0 = bb::wmulk<bb::W_ONE>(x[0]), X1 = bb::wmulk<bb::W_ONE>(x[1]);
  const int64_t Y0 = bb::wmad(X0, x[2], w[0]), Y2 = bb::wmad(X0, x[2], n1);
  const i128 eY0 = (i128)x[0] * bb::W_ONE + (i128)x[2] * w[0], eY2 = (i128)x[0] * bb::W_ONE - (i128)x[2] * w[0];
  if ((i128)Y0 != eY0 || (i128)Y2 != eY2) fail("first-stage sums (added pair)", x, w);
  const int32_t s1 = checked_redc((i128)X1 + (i128)x[3] * w[0], bb::wmad(X1, x[3], w[0]), x, w);
  const int32_t s3 = checked_redc((i128)X1 - (i128)x[3] * w[0], bb::wmad(X1, x[3], n1), x, w);
  int32_t step[4];
  step[0] = checked_redc(eY0 + (i128)s1 * w[1], bb::wmad(Y0, s1, w[1]), x, w);
  step[1] = checked_redc(eY0 - (i128)s1 * w[1], bb::wmad(Y0, s1, n2), x, w);
  step[2] = checked_redc(eY2 + (i128)s3 * w[2], bb::wmad(Y2, s3, w[2]), x, w);
  step[3] = checked_redc(eY2 - (i128)s3 * w[2], bb::wmad(Y2, s3, n2i), x, w);
  int32_t a[4] = {x[0], x[1], x[2], x[3]};
  bb::ct4w(a[0], a[1], a[2], a[3], w[0], n1, w[1], n2, w[2], n2i);
  int32_t p[4] = {x[0], x[1], x[2], x[3]}, q[4] = {x[3], x[2], x[1], x[0]}, q1[4] = {x[3], x[2], x[1], x[0]};
  bb::ct4w2(p, q, w[0], n1, w[1], n2, w[2], n2i);
  bb::ct4w(q1[0], q1[1], q1[2], q1[3], w[0], n1, w[1], n2, w[2], n2i);
  for (int i = 0; i < 4; i++) {
    if (a[i] != step[i] || p[i] != a[i] || q[i] != q1[i]) fail("ct4w / ct4w2 differ from the checked flow", x, w);
    if (canon(a[i]) != want[i]) fail("quad output is not the field's", x, w);
    if (a[i] == INT32_MIN) fail("output is not a legal input", x, w);
    const uint64_t m = (uint64_t)(a[i] < 0 ? -(int64_t)a[i] : (int64_t)a[i]);
    if (m > max_out) max_out = m;
    out[i] = a[i];
  }
}

// the coset scale: a word of (-p, p) times a canonical Montgomery-form factor
void scale(int32_t x, uint32_t g) {
  n_scales++;
  const int32_t xs[4] = {x, 0, 0, 0}, gs[3] = {(int32_t)g, 0, 0};
  const int64_t acc = bb::wmul(x, (int32_t)g);
  const int32_t r = checked_redc((i128)x * (i128)g, acc, xs, gs);
  if (r != bb::wscale(x, g)) fail("wscale differs from the checked flow", xs, gs);
  if (r >= (int32_t)bb::P || r <= -(int32_t)bb::P) fail("scaled word outside (-p, p)", xs, gs);
  if (canon(r) != bb::mont_mul(canon(x), g)) fail("scaled word is not x g / R", xs, gs);
  int32_t v[4] = {x, -x, x, 0};
  bb::wscale4(v, g);
  if (v[0] != r || v[2] != r || v[1] != bb::wscale(-x, g) || v[3] != 0) fail("wscale4", xs, gs);
}

}  // namespace

int main() {
  int32_t out[4];
  // every combination of the edge words and edge twiddles
  const int32_t words[] = {0, 1, -1, (int32_t)(bb::P - 1), -(int32_t)(bb::P - 1), INT32_MAX, -INT32_MAX, INT32_MIN + 1};
  const int32_t tws[] = {0, 1, -1, H, -H};
  for (int32_t a : words) for (int32_t b : words) for (int32_t c : words) for (int32_t d : words)
    for (int32_t w1 : tws) for (int32_t w2 : tws) for (int32_t w2i : tws) {
      const int32_t x[4] = {a, b, c, d}, w[3] = {w1, w2, w2i};
      quad(x, w, out);
    }
  // seeded random quads: any int32 word but INT32_MIN, any centred twiddle
  for (int i = 0; i < 1000000; i++) {
    const int32_t x[4] = {rnd_word(), rnd_word(), rnd_word(), rnd_word()}, w[3] = {rnd_twiddle(), rnd_twiddle(), rnd_twiddle()};
    quad(x, w, out);
  }
  // 64 chained rounds fed with their own outputs, spans shrinking as in the transform (256, 64, 16, 4, 1 ...): random, and with the twiddles at their largest;
  // from the second round on the words are inside (-p, p).  Mode 3 starts from canonical words, as the kernels do: inside (-p, p) from the FIRST round on.
  for (int mode = 0; mode < 4; mode++) {
    std::vector<int32_t> st(1024);
    for (auto& v : st) v = mode == 0 ? rnd_word() : (mode == 1 ? INT32_MAX : (mode == 2 ? ((rnd() & 1) ? INT32_MAX : INT32_MIN + 1) : ((rnd() & 1) ? (int32_t)(bb::P - 1) : (int32_t)(rnd() % bb::P))));
    for (int round = 0; round < 64; round++) {
      const int d = 256 >> (2 * (round % 5));
      for (int g = 0; g < 1024; g++) {
        if ((g / d) % 4) continue;
        int32_t x[4] = {st[g], st[g + d], st[g + 2 * d], st[g + 3 * d]}, w[3];
        for (int i = 0; i < 3; i++) w[i] = mode == 0 ? rnd_twiddle() : ((mode == 1 || (rnd() & 1)) ? H : -H);
        quad(x, w, out);
        for (int i = 0; i < 4; i++) {
          if ((round >= 1 || mode == 3) && (out[i] >= (int32_t)bb::P || out[i] <= -(int32_t)bb::P)) fail("chained word outside (-p, p)", x, w);
          st[g + i * d] = out[i];
        }
      }
    }
    // what the last inverse round hands on is scaled: every word of the final state times edge and random factors
    const uint32_t gedge[] = {0u, 1u, bb::R1, (uint32_t)H, (uint32_t)H + 1, bb::P - 2, bb::P - 1};
    for (int32_t v : st) {
      if (v >= (int32_t)bb::P || v <= -(int32_t)bb::P) continue;
      for (uint32_t g : gedge) scale(v, g);
      scale(v, (uint32_t)(rnd() % bb::P));
    }
  }
  // the scale on the edge words of (-p, p) and on seeded random ones
  const int32_t sw[] = {0, 1, -1, H, -H, (int32_t)(bb::P - 1), -(int32_t)(bb::P - 1)};
  const uint32_t sg[] = {0u, 1u, bb::R1, (uint32_t)H, (uint32_t)H + 1, bb::P - 2, bb::P - 1};
  for (int32_t x : sw) for (uint32_t g : sg) scale(x, g);
  for (int i = 0; i < 1000000; i++) scale((int32_t)(rnd() % (2ull * bb::P - 1)) - (int32_t)(bb::P - 1), (uint32_t)(rnd() % bb::P));
  std::printf("OK %" PRIu64 " quads, %" PRIu64 " scales, max |acc| = %.4f * 2^62, max |out| = %.4f p\n", n_quads, n_scales, (double)max_acc / 4611686018427387904.0, (double)max_out / (double)bb::P);
  return 0;
}
