// The wide signed butterflies of babybear.h (dit4w / dit4w2 / dit2w and their primitives), host side, against the canonical field arithmetic
// (bb::mul / bb::add / bb::sub) and against their documented bounds.  Exits 0 and prints one summary line, or prints the first failure and exits 1.
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
uint64_t n_quads = 0;

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

// one quad: the field reference, the step-by-step flow with every sum checked, dit4w and dit4w2
void quad(const int32_t* x, const int32_t* w, int32_t* out) {
  n_quads++;
  // reference: canonical arithmetic; a Montgomery-form twiddle wm stands for the field element wm / R
  const uint32_t c0 = canon(x[0]), c1 = canon(x[1]), c2 = canon(x[2]), c3 = canon(x[3]);
  const uint32_t v1 = bb::from_mont(canon(w[0])), v2 = bb::from_mont(canon(w[1])), v2i = bb::from_mont(canon(w[2]));
  const uint32_t t1 = bb::mul(c1, v1), t3 = bb::mul(c3, v1);
  const uint32_t y0 = bb::add(c0, t1), y1 = bb::sub(c0, t1), y2 = bb::add(c2, t3), y3 = bb::sub(c2, t3);
  const uint32_t u2 = bb::mul(y2, v2), u3 = bb::mul(y3, v2i);
  const uint32_t want[4] = {bb::add(y0, u2), bb::add(y1, u3), bb::sub(y0, u2), bb::sub(y1, u3)};
  // the flow of dit4w from its primitives, every accumulator against the exact integer
  const int32_t n1 = -w[0], n2 = -w[1], n2i = -w[2];
  const int64_t X0 = bb::wmulk<bb::W_ONE>(x[0]), X2 = bb::wmulk<bb::W_ONE>(x[2]);
  if ((i128)X0 != (i128)x[0] * bb::W_ONE || bb::wmul(x[2], bb::W_ONE) != X2) fail("wmul / wmulk", x, w);
  const int64_t Y0 = bb::wmad(X0, x[1], w[0]), Y1 = bb::wmad(X0, x[1], n1);
  const i128 eY0 = (i128)X0 + (i128)x[1] * w[0], eY1 = (i128)X0 - (i128)x[1] * w[0];
  if ((i128)Y0 != eY0 || (i128)Y1 != eY1) fail("first-stage sums (even pair)", x, w);
  const int32_t s2 = checked_redc((i128)X2 + (i128)x[3] * w[0], bb::wmad(X2, x[3], w[0]), x, w);
  const int32_t s3 = checked_redc((i128)X2 - (i128)x[3] * w[0], bb::wmad(X2, x[3], n1), x, w);
  int32_t step[4];
  step[0] = checked_redc(eY0 + (i128)s2 * w[1], bb::wmad(Y0, s2, w[1]), x, w);
  step[2] = checked_redc(eY0 - (i128)s2 * w[1], bb::wmad(Y0, s2, n2), x, w);
  step[1] = checked_redc(eY1 + (i128)s3 * w[2], bb::wmad(Y1, s3, w[2]), x, w);
  step[3] = checked_redc(eY1 - (i128)s3 * w[2], bb::wmad(Y1, s3, n2i), x, w);
  int32_t a[4] = {x[0], x[1], x[2], x[3]};
  bb::dit4w(a[0], a[1], a[2], a[3], w[0], n1, w[1], n2, w[2], n2i);
  int32_t p[4] = {x[0], x[1], x[2], x[3]}, q[4] = {x[3], x[2], x[1], x[0]}, q1[4] = {x[3], x[2], x[1], x[0]};
  bb::dit4w2(p, q, w[0], n1, w[1], n2, w[2], n2i);
  bb::dit4w(q1[0], q1[1], q1[2], q1[3], w[0], n1, w[1], n2, w[2], n2i);
  for (int i = 0; i < 4; i++) {
    if (a[i] != step[i] || p[i] != a[i] || q[i] != q1[i]) fail("dit4w / dit4w2 differ from the checked flow", x, w);
    if (canon(a[i]) != want[i]) fail("quad output is not the field's", x, w);
    if (a[i] == INT32_MIN) fail("output is not a legal input", x, w);
    const uint64_t m = (uint64_t)(a[i] < 0 ? -(int64_t)a[i] : (int64_t)a[i]);
    if (m > max_out) max_out = m;
    out[i] = a[i];
  }
}

void small_helpers() {
  const int32_t none[4] = {0, 0, 0, 0};
  const uint32_t edge[] = {0u, 1u, (uint32_t)H - 1, (uint32_t)H, (uint32_t)H + 1, (uint32_t)H + 2, bb::P - 2, bb::P - 1};
  std::vector<uint32_t> vals(edge, edge + 8);
  for (int i = 0; i < 100000; i++) vals.push_back((uint32_t)(rnd() % bb::P));
  for (uint32_t v : vals) {
    const int32_t c = bb::centre(v);
    if (c > H || c < -H || canon(c) != v) fail("centre", none, none);
    if (bb::wcanon(c) != v || bb::wcanon((int32_t)v) != v || bb::wcanon((int32_t)v - (int32_t)bb::P) != v) fail("wcanon", none, none);
  }
  for (size_t i = 0; i + 1 < vals.size(); i++) {
    const int32_t c = bb::mont_mul_centred(vals[i], vals[i + 1]);
    if (c > H || c < -H || canon(c) != bb::mont_mul(vals[i], vals[i + 1])) fail("mont_mul_centred", none, none);
  }
  for (int i = 0; i < 200000; i++) {                           // radix-2 butterfly
    int32_t a = rnd_word(), b = rnd_word();
    const int32_t w = i < 8 ? (i & 1 ? H : -H) : rnd_twiddle();
    if (i < 8) { a = (i & 2) ? INT32_MAX : INT32_MIN + 1; b = (i & 4) ? INT32_MAX : INT32_MIN + 1; }
    const uint32_t t = bb::mul(canon(b), bb::from_mont(canon(w))), wa = bb::add(canon(a), t), wb = bb::sub(canon(a), t);
    const i128 e0 = (i128)a * bb::W_ONE + (i128)b * w, e1 = (i128)a * bb::W_ONE - (i128)b * w;
    const i128 lim = (i128)bb::WREDC_IN_MAX;
    if (e0 >= lim || e0 <= -lim || e1 >= lim || e1 <= -lim) fail("dit2w: reduction input out of bounds", none, none);
    bb::dit2w(a, b, w, -w);
    if (canon(a) != wa || canon(b) != wb || a == INT32_MIN || b == INT32_MIN) fail("dit2w", none, none);
  }
}

}  // namespace

int main() {
  small_helpers();
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
  // 64 chained rounds fed with their own outputs: random, and with the twiddles at their largest; from the second round on the words are inside (-p, p)
  for (int mode = 0; mode < 3; mode++) {
    std::vector<int32_t> st(1024);
    for (auto& v : st) v = mode == 0 ? rnd_word() : (mode == 1 ? INT32_MAX : ((rnd() & 1) ? INT32_MAX : INT32_MIN + 1));
    for (int round = 0; round < 64; round++) {
      const int d = 1 << (2 * (round % 4));                    // quads of span 1, 4, 16, 64: the words mix
      for (int g = 0; g < 1024; g++) {
        if ((g / d) % 4) continue;
        int32_t x[4] = {st[g], st[g + d], st[g + 2 * d], st[g + 3 * d]}, w[3];
        for (int i = 0; i < 3; i++) w[i] = mode == 0 ? rnd_twiddle() : ((mode == 1 || (rnd() & 1)) ? H : -H);
        quad(x, w, out);
        for (int i = 0; i < 4; i++) {
          // round index 1 is the second round
          if (round >= 1 && (out[i] >= (int32_t)bb::P || out[i] <= -(int32_t)bb::P)) fail("chained word outside (-p, p) after the second round", x, w);
          st[g + i * d] = out[i];
        }
      }
    }
  }
  std::printf("OK %" PRIu64 " quads, max |acc| = %.4f * 2^62, max |out| = %.4f p\n", n_quads, (double)max_acc / 4611686018427387904.0, (double)max_out / (double)bb::P);
  return 0;
}
