// arith_probe.hip — test probe: the bb:: primitives and the Poseidon2 formulations of zkir_amd/csrc/babybear.h / poseidon2.h, run elementwise
// on the device AND on the host, so that tests/test_arith_edges.py / test_gpu_arith_edges.py can compare every returned word with the
// big-integer reference (tests/bigint_ref.py).  The headers are included unchanged and this file is compiled with stark.hip's flags, so the
// device code paths (the inline-asm ones included) are the ones the product kernels inline.  Not part of libzkir_amd.so.
//
// Entry points (extern "C"; `on_host` != 0: plain host pointers, the host build of the same functions; otherwise device pointers, launched on
// `hip_stream`; 0 = success, else the hipError_t of the launch):
//   zkir_probe_op_name(op)                          the name of elementwise op `op` (nullptr past the last)
//   zkir_probe_elementwise(op, in, n, uarg, out)    in: n x 4 u64 argument slots, out: n x 2 u64 result slots (layout: tests/test_arith_edges.py)
//   zkir_probe_acc96(variant, xs, ys, terms, n, out) n sums of `terms` products through mad96 (0), mad96_s (1) or mad96x4_s (2); out: n x 4 x 3 u64
//                                                   (lo, hi, acc96_div_R) per sum; variant 0: xs n x terms, 1: xs terms, 2: xs terms x 4 (uniform)
//   zkir_probe_p2(form, raw, consts, in, n, out_canon, out_raw)
//                                                   n permutations of 12 words: form 0 permute_scaled, 1 permute_quad_scaled, 2 permute_row16_scaled,
//                                                   3 permute (Montgomery form); raw = 0: canonical words in, else raw input words of the formulation
//   zkir_probe_p2_consts(out) / zkir_probe_p2_consts_size() / zkir_probe_p2_scales(out[3] = in_scale, out_scale, carry)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../zkir_amd/csrc/babybear.h"
#include "../../zkir_amd/csrc/poseidon2.h"

namespace {

constexpr int NT = 256;
constexpr int SMAD_K[] = {-2, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024};
const char* const OP_NAMES[] = {"add", "sub", "neg", "reduce_2p", "mont_mul", "mont_mul_lazy", "mont_mul_add_lazy", "mont_reduce_wide",
                                "reduce_wide4", "reduce_wide6", "reduce_wide7", "mad_wide1", "mad_wide2", "mulhi_u32", "smont_mul", "smont_mul_add",
                                "smont_reduce_wide", "sacc_add", "smad-2", "smad1", "smad2", "smad4", "smad8", "smad16", "smad32", "smad64", "smad128",
                                "smad256", "smad512", "smad1024", "e_mul_m", "e_inv_m", "pow", "inv"};
constexpr int N_OPS = sizeof(OP_NAMES) / sizeof(OP_NAMES[0]);

template <int I>
BB_HD uint64_t smad_k(uint64_t acc, uint32_t x) { return (uint64_t)p2::smad<SMAD_K[I]>((int64_t)acc, (int32_t)x); }

// one element: a[0..3] the argument slots, r[0..1] the results.  mulhi_u32's second operand is `uarg` (the instruction takes it in a scalar register).
// E4 ops: coefficient k of the first operand in the low half of a[k], of the second in the high half; result coefficients 2j, 2j+1 in r[j].
BB_HD void eval_op(int op, const uint64_t* a, uint32_t uarg, uint64_t* r) {
  const uint32_t x = (uint32_t)a[0], y = (uint32_t)a[1];
  r[1] = 0;
  switch (op) {
    case 0: r[0] = bb::add(x, y); break;
    case 1: r[0] = bb::sub(x, y); break;
    case 2: r[0] = bb::neg(x); break;
    case 3: r[0] = bb::reduce_2p(x); break;
    case 4: r[0] = bb::mont_mul(x, y); break;
    case 5: r[0] = bb::mont_mul_lazy(x, y); break;
    case 6: r[0] = bb::mont_mul_add_lazy(x, y, a[2]); break;
    case 7: r[0] = bb::mont_reduce_wide(a[0]); break;
    case 8: r[0] = bb::reduce_wide<4>(a[0]); break;
    case 9: r[0] = bb::reduce_wide<6>(a[0]); break;
    case 10: r[0] = bb::reduce_wide<7>(a[0]); break;
    case 11: r[0] = bb::mad_wide<1>(a[0], y); break;
    case 12: r[0] = bb::mad_wide<2>(a[0], y); break;
    case 13: r[0] = bb::mulhi_u32(x, uarg); break;
    case 14: r[0] = (uint32_t)bb::smont_mul((int32_t)x, (int32_t)y); break;
    case 15: r[0] = (uint32_t)bb::smont_mul_add((int32_t)x, (int32_t)y, a[2]); break;
    case 16: r[0] = (uint32_t)bb::smont_reduce_wide((int64_t)a[0]); break;
    case 17: r[0] = (uint64_t)bb::sacc_add((int64_t)a[0], (int32_t)y); break;
    case 18: r[0] = smad_k<0>(a[0], y); break;
    case 19: r[0] = smad_k<1>(a[0], y); break;
    case 20: r[0] = smad_k<2>(a[0], y); break;
    case 21: r[0] = smad_k<3>(a[0], y); break;
    case 22: r[0] = smad_k<4>(a[0], y); break;
    case 23: r[0] = smad_k<5>(a[0], y); break;
    case 24: r[0] = smad_k<6>(a[0], y); break;
    case 25: r[0] = smad_k<7>(a[0], y); break;
    case 26: r[0] = smad_k<8>(a[0], y); break;
    case 27: r[0] = smad_k<9>(a[0], y); break;
    case 28: r[0] = smad_k<10>(a[0], y); break;
    case 29: r[0] = smad_k<11>(a[0], y); break;
    case 30:
    case 31: {
      const bb::E4 ea{{(uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3]}};
      const bb::E4 eb{{(uint32_t)(a[0] >> 32), (uint32_t)(a[1] >> 32), (uint32_t)(a[2] >> 32), (uint32_t)(a[3] >> 32)}};
      const bb::E4 e = op == 30 ? bb::e_mul_m(ea, eb) : bb::e_inv_m(ea);
      r[0] = e.c[0] | (uint64_t)e.c[1] << 32;
      r[1] = e.c[2] | (uint64_t)e.c[3] << 32;
      break;
    }
    case 32: r[0] = bb::pow(x, a[1]); break;
    case 33: r[0] = bb::inv(x); break;
    default: r[0] = ~0ull; r[1] = ~0ull;
  }
}

__global__ __launch_bounds__(NT) void elementwise_kernel(int op, const uint64_t* __restrict__ in, uint64_t n, uint32_t uarg, uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  uint64_t a[4], r[2];
  for (int k = 0; k < 4; k++) a[k] = in[4 * i + k];
  eval_op(op, a, uarg, r);
  out[2 * i] = r[0];
  out[2 * i + 1] = r[1];
}

// 96-bit sums; the scalar-operand variants read their x from the same address in every lane (a uniform load: scalar registers, as in the kernels)
template <int V>
__device__ __forceinline__ void acc96_lane(const uint32_t* __restrict__ xs, const uint32_t* __restrict__ ys, uint32_t terms, uint64_t i, bb::Acc96* acc) {
  for (int k = 0; k < 4; k++) acc[k] = bb::acc96_zero();
  for (uint32_t t = 0; t < terms; t++) {
    const uint32_t y = ys[i * terms + t];
    if (V == 0) bb::mad96(acc[0], xs[i * terms + t], y);
    else if (V == 1) bb::mad96_s(acc[0], xs[t], y);
    else bb::mad96x4_s(acc, xs[4 * t], xs[4 * t + 1], xs[4 * t + 2], xs[4 * t + 3], y);
  }
}
template <int V>
__global__ __launch_bounds__(NT) void acc96_kernel(const uint32_t* __restrict__ xs, const uint32_t* __restrict__ ys, uint32_t terms, uint64_t n, uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
  const uint64_t li = i < n ? i : n - 1;                          // every lane runs (uniform x loads), only the real ones store
  bb::Acc96 acc[4];
  acc96_lane<V>(xs, ys, terms, li, acc);
  if (i >= n) return;
  for (int k = 0; k < 4; k++) {
    out[12 * i + 3 * k] = acc[k].lo;
    out[12 * i + 3 * k + 1] = acc[k].hi;
    out[12 * i + 3 * k + 2] = bb::acc96_div_R(acc[k]);
  }
}

BB_HD uint32_t p2_in(uint32_t w, int raw, const p2::Consts& c) { return raw ? w : bb::mont_mul_lazy(w, c.in_scale); }

// form 0: one permutation per lane; form 3: permute() on Montgomery words
__global__ __launch_bounds__(NT) void p2_lane_kernel(int form, int raw, const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ in, uint64_t n,
                                                     uint32_t* __restrict__ out_canon, uint32_t* __restrict__ out_raw) {
  const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const p2::Consts& c = *cp;
  uint32_t s[p2::T];
  if (form == 0) {
    for (int k = 0; k < p2::T; k++) s[k] = p2_in(in[12 * i + k], raw, c);
    p2::permute_scaled(s, c);
    for (int k = 0; k < p2::T; k++) { out_raw[12 * i + k] = s[k]; out_canon[12 * i + k] = bb::mont_mul(s[k], c.out_scale); }
  } else {
    for (int k = 0; k < p2::T; k++) s[k] = raw ? in[12 * i + k] : bb::to_mont(in[12 * i + k]);
    p2::permute(s, c);
    for (int k = 0; k < p2::T; k++) { out_raw[12 * i + k] = s[k]; out_canon[12 * i + k] = bb::from_mont(s[k]); }
  }
}

// form 1: one permutation per quad (lane l of the quad holds words l, 4 + l, 8 + l); every lane of the launch runs, lanes past n on a copy of the
// last permutation's input, so that every quad is whole
__global__ __launch_bounds__(NT) void p2_quad_kernel(int raw, const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ in, uint64_t n,
                                                     uint32_t* __restrict__ out_canon, uint32_t* __restrict__ out_raw) {
  const uint64_t g = (uint64_t)blockIdx.x * NT + threadIdx.x, i = g >> 2;
  const int l = (int)(g & 3);
  const uint64_t ii = i < n ? i : n - 1;
  const p2::Consts& c = *cp;
  uint32_t s[3];
  for (int b = 0; b < 3; b++) s[b] = p2_in(in[12 * ii + 4 * b + l], raw, c);
  p2::permute_quad_scaled(s, l, c);
  if (i >= n) return;
  for (int b = 0; b < 3; b++) { out_raw[12 * i + 4 * b + l] = s[b]; out_canon[12 * i + 4 * b + l] = bb::mont_mul(s[b], c.out_scale); }
}

// form 2: one permutation per row of 16 lanes (lane l < 12 holds word l); lanes 12-15 are handed `junk` ("anything"), which must not reach a real word
__global__ __launch_bounds__(NT) void p2_row16_kernel(int raw, const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ in, uint64_t n, uint32_t junk,
                                                      uint32_t* __restrict__ out_canon, uint32_t* __restrict__ out_raw) {
  const uint64_t g = (uint64_t)blockIdx.x * NT + threadIdx.x, i = g >> 4;
  const int l = (int)(g & 15);
  const uint64_t ii = i < n ? i : n - 1;
  const p2::Consts& c = *cp;
  const uint32_t s = l < p2::T ? p2_in(in[12 * ii + l], raw, c) : junk ^ (uint32_t)(g * 0x9E3779B9u);
  const uint32_t o = p2::permute_row16_scaled(s, l, c);
  if (i >= n || l >= p2::T) return;
  out_raw[12 * i + l] = o;
  out_canon[12 * i + l] = bb::mont_mul(o, c.out_scale);
}

const p2::Consts& host_consts() {
  static const p2::Consts c = [] { p2::Consts k; p2::generate(k); return k; }();
  return c;
}

inline unsigned blocks(uint64_t lanes) { return (unsigned)((lanes + NT - 1) / NT); }
// the thread's last HIP error is sticky and shared with every other library of the process (torch among them): cleared before a launch, read after it,
// so that the status returned is this launch's own
inline void clear_error() { (void)hipGetLastError(); }

}  // namespace

extern "C" {

const char* zkir_probe_op_name(int op) { return op >= 0 && op < N_OPS ? OP_NAMES[op] : nullptr; }

int zkir_probe_elementwise(int on_host, int op, const uint64_t* in, uint64_t n, uint32_t uarg, uint64_t* out, void* hip_stream) {
  if (on_host) {
    for (uint64_t i = 0; i < n; i++) eval_op(op, in + 4 * i, uarg, out + 2 * i);
    return 0;
  }
  if (n == 0) return 0;
  clear_error();
  hipLaunchKernelGGL(elementwise_kernel, dim3(blocks(n)), dim3(NT), 0, (hipStream_t)hip_stream, op, in, n, uarg, out);
  return (int)hipGetLastError();
}

int zkir_probe_acc96(int on_host, int variant, const uint32_t* xs, const uint32_t* ys, uint32_t terms, uint64_t n, uint64_t* out, void* hip_stream) {
  if (on_host) {
    for (uint64_t i = 0; i < n; i++) {
      bb::Acc96 acc[4] = {bb::acc96_zero(), bb::acc96_zero(), bb::acc96_zero(), bb::acc96_zero()};
      for (uint32_t t = 0; t < terms; t++) {
        const uint32_t y = ys[i * terms + t];
        if (variant == 0) bb::mad96(acc[0], xs[i * terms + t], y);
        else if (variant == 1) bb::mad96_s(acc[0], xs[t], y);
        else bb::mad96x4_s(acc, xs[4 * t], xs[4 * t + 1], xs[4 * t + 2], xs[4 * t + 3], y);
      }
      for (int k = 0; k < 4; k++) { out[12 * i + 3 * k] = acc[k].lo; out[12 * i + 3 * k + 1] = acc[k].hi; out[12 * i + 3 * k + 2] = bb::acc96_div_R(acc[k]); }
    }
    return 0;
  }
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)hip_stream;
  clear_error();
  if (variant == 0) hipLaunchKernelGGL(acc96_kernel<0>, dim3(blocks(n)), dim3(NT), 0, s, xs, ys, terms, n, out);
  else if (variant == 1) hipLaunchKernelGGL(acc96_kernel<1>, dim3(blocks(n)), dim3(NT), 0, s, xs, ys, terms, n, out);
  else hipLaunchKernelGGL(acc96_kernel<2>, dim3(blocks(n)), dim3(NT), 0, s, xs, ys, terms, n, out);
  return (int)hipGetLastError();
}

uint64_t zkir_probe_p2_consts_size(void) { return sizeof(p2::Consts); }
void zkir_probe_p2_consts(void* out) { std::memcpy(out, &host_consts(), sizeof(p2::Consts)); }
void zkir_probe_p2_scales(uint32_t out[3]) { out[0] = host_consts().in_scale; out[1] = host_consts().out_scale; out[2] = host_consts().carry; }

// consts: a device copy of zkir_probe_p2_consts()'s bytes (ignored on the host); junk: what lanes 12-15 of form 2 hold
int zkir_probe_p2(int on_host, int form, int raw, const void* consts, const uint32_t* in, uint64_t n, uint32_t junk, uint32_t* out_canon, uint32_t* out_raw,
                  void* hip_stream) {
  if (on_host) {
    const p2::Consts& c = host_consts();
    for (uint64_t i = 0; i < n; i++) {
      uint32_t s[p2::T];
      if (form == 0) {
        for (int k = 0; k < p2::T; k++) s[k] = p2_in(in[12 * i + k], raw, c);
        p2::permute_scaled(s, c);
        for (int k = 0; k < p2::T; k++) { out_raw[12 * i + k] = s[k]; out_canon[12 * i + k] = bb::mont_mul(s[k], c.out_scale); }
      } else if (form == 3) {
        for (int k = 0; k < p2::T; k++) s[k] = raw ? in[12 * i + k] : bb::to_mont(in[12 * i + k]);
        p2::permute(s, c);
        for (int k = 0; k < p2::T; k++) { out_raw[12 * i + k] = s[k]; out_canon[12 * i + k] = bb::from_mont(s[k]); }
      } else {
        return (int)hipErrorInvalidValue;                                      // the quad / row16 formulations exist on the device only
      }
    }
    return 0;
  }
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)hip_stream;
  const p2::Consts* cp = (const p2::Consts*)consts;
  clear_error();
  if (form == 0 || form == 3) hipLaunchKernelGGL(p2_lane_kernel, dim3(blocks(n)), dim3(NT), 0, s, form, raw, cp, in, n, out_canon, out_raw);
  else if (form == 1) hipLaunchKernelGGL(p2_quad_kernel, dim3(blocks(4 * n)), dim3(NT), 0, s, raw, cp, in, n, out_canon, out_raw);
  else if (form == 2) hipLaunchKernelGGL(p2_row16_kernel, dim3(blocks(16 * n)), dim3(NT), 0, s, raw, cp, in, n, junk, out_canon, out_raw);
  else return (int)hipErrorInvalidValue;
  return (int)hipGetLastError();
}

}  // extern "C"
