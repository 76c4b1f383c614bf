// ntt.hip — Baby Bear NTT passes and the coset low-degree extension on gfx950 (part of the self-defined prover stages, DESIGN.md §8;
// oracle: so::lde / so::ntt in oracle/stark_oracle.cpp).  Split from stark.hip because the two want different instruction
// scheduling: these kernels are LDS/register-pressure sensitive (default scheduler), the hash kernels want maximum ILP.
//
// Matrix layout ("B8", include/zkir_amd.h): columns are grouped in blocks of 8; block b of a matrix with n rows is the array
// [n][8] of u32, i.e. every row position holds 32 contiguous bytes = two uint4 (columns 8b..8b+3 and 8b+4..8b+7).  Every kernel here
// moves and computes on uint4: one lane carries FOUR columns of one position, so the index arithmetic and — what matters, the
// kernels being VALU-bound — the twiddle bookkeeping (3 of the 7 Montgomery products per radix-4 quad were twiddle derivations
// when a lane carried one column) are shared by four (strided passes: eight) columns.
//
// Per block: inverse NTT over H as a MULTIPLY-FIRST Cooley-Tukey transform (natural -> bit-reversed: the twiddle of a butterfly belongs to
// its block, see "the inverse side" below), coset scale g^k / N, zero-interleave, forward DIT NTT over the 2N coset (bit-reversed -> natural);
// both sides run the wide signed radix-4 quad of babybear.h on int32 residues in (-p, p).  LDS-staged passes: strided passes move tiles of 2^B rows x 2^C positions (2^C * 32 bytes
// consecutive per tile row keep loads coalesced); the last 10 inverse stages, the scaling and the first 11 forward stages are
// fused in one contiguous-chunk kernel.  HBM traffic per element and column: 8 B per strided pass, 12 B for the fused middle.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <mutex>
#include <type_traits>

#include "../../include/zkir_amd.h"
#include "../../include/zkir_amd_experimental.h"
#include "babybear.h"
#include "host.h"

namespace {

constexpr int NT = 256;
__device__ __forceinline__ uint32_t bitrev(uint32_t x, int bits) { return bits == 0 ? 0u : __brev(x) >> (32 - bits); }

// compile-time loop: the body sees its index as a constant, so small per-lane arrays stay in registers
template <int K, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (K < N) { f(std::integral_constant<int, K>{}); static_for<K + 1, N>(f); }
}

using u32x4 = uint32_t __attribute__((ext_vector_type(4)));          // plain vector for values that only travel (prefetch registers)
__device__ __forceinline__ u32x4 ld4(const uint4* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ void st4(uint4* p, u32x4 v) { *reinterpret_cast<u32x4*>(p) = v; }

// LDS hand-off INSIDE a wave: the next round reads only what this wave itself wrote (LDS operations of one wave execute in issue
// order; the wait makes the writes complete, the clobber keeps the compiler from moving LDS accesses across).  Where it applies it
// replaces a workgroup barrier: the waves of a workgroup then drift apart, and one wave's LDS latency is covered by another's arithmetic
// instead of all of them waiting at the same instruction.
__device__ __forceinline__ void wave_sync_lds() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// ---- both sides in WIDE SIGNED arithmetic, four columns at a time (babybear.h: dit4w / ct4w / dit2w / wscale) ----------------------
// Representation contract, private to lde_run: words enter canonical — a legal word of (-p, p) — and stay int32 residues in (-p, p) from the
// first inverse round through the coset scale to the last forward round; twiddles are centred.  The LAST forward kernel of a chain
// (`canon` != 0) brings its results back to [0, p) on the way out; nothing is canonicalised in between (`in` is scratch and holds signed words).
struct WTw { int32_t w, n; };                                                  // a centred twiddle and its negation
__device__ __forceinline__ WTw wtw(int32_t w) { return WTw{w, -w}; }
// forward (DIT) radix-4 quad: stages with twiddles w1 = w2^2 (first stage), w2 / w2i = w2 * j (second stage); outputs in positions
// (0, 2, 1, 3) order of the classic DIT flow: o0 -> i0, o1 -> i0 + d, o2 -> i0 + 2d, o3 -> i0 + 3d
__device__ __forceinline__ void dit4w4(uint4& x0, uint4& x1, uint4& x2, uint4& x3, WTw w1, WTw w2, WTw w2i) {
#define ZKIR_Q(c, e) { int32_t a[4] = {(int32_t)x0.c, (int32_t)x1.c, (int32_t)x2.c, (int32_t)x3.c}, b[4] = {(int32_t)x0.e, (int32_t)x1.e, (int32_t)x2.e, (int32_t)x3.e}; \
                       bb::dit4w2(a, b, w1.w, w1.n, w2.w, w2.n, w2i.w, w2i.n); \
                       x0.c = (uint32_t)a[0]; x1.c = (uint32_t)a[1]; x2.c = (uint32_t)a[2]; x3.c = (uint32_t)a[3]; x0.e = (uint32_t)b[0]; x1.e = (uint32_t)b[1]; x2.e = (uint32_t)b[2]; x3.e = (uint32_t)b[3]; }
  // two columns at a time: the scheduler would otherwise interleave all four chains and hold their 64-bit sums at once
  ZKIR_Q(x, y) __builtin_amdgcn_sched_barrier(0); ZKIR_Q(z, w)
#undef ZKIR_Q
}
// ---- the inverse side: stage s = 0 .. L-1 has span h = N / 2^(s+1); block j < 2^s holds the pairs (a, b) = (x[2hj + i], x[2hj + i + h]) -> (a + w b, a - w b) with
// w = w_N^-(brv_s(j) N / 2^(s+1)): multiply first, so the sums ride in the multiply-adds exactly as on the forward side.  A radix-4 round (stages s, s+1 on x0..x3 at
// distances 0, d, 2d, 3d, d = h / 2) needs w2 = the twiddle of stage s+1's block 2j, w1 = w2^2 and w2i = w2 j (j the inverse 4th root).  For a pass that starts at
// stage s0, a block index at local stage b is hi 2^b + j (hi: the s0 high bits a tile / chunk / lane group fixes), brv(hi 2^b + j) = brv_b(j) 2^s0 + brv_s0(hi), and
//     w2 = small_inv[brv_b(j) << (8 - b)]  *  tw_inv[brv_s0(hi) << (L - s0 - b - 2)]
// — a root of order 2^(b+2) <= 1024 that depends on (lane, round) only, times a factor that is UNIFORM over the tile or chunk (1 for s0 = 0).  The data movement
// (natural -> bit-reversed, shrinking spans) is that of the add-first transform this replaces, so tiles, LDS indices and the wave-local rounds are unchanged.
// Every inverse kernel lde_run can pick for log_n >= 10 is of this one factorisation: the arrays between stages differ from the add-first ones by twiddle factors.
__device__ __forceinline__ void ct4w4(uint4& x0, uint4& x1, uint4& x2, uint4& x3, WTw w1, WTw w2, WTw w2i) { dit4w4(x0, x2, x1, x3, w1, w2, w2i); }
// the three twiddles of an inverse round from the (lane, round) root `sm` and the uniform factor `f` (both canonical Montgomery form); `unit`: f = 1
__device__ __forceinline__ void ct_twiddles(uint32_t sm, uint32_t f, bool unit, uint32_t j4_m, WTw& w1, WTw& w2, WTw& w2i) {
  uint32_t w2u;
  if (unit) { w2u = sm; w2 = wtw(bb::centre(sm)); }
  else { w2 = wtw(bb::mont_mul_centred(sm, f)); w2u = bb::wcanon(w2.w); }
  w1 = wtw(bb::mont_mul_centred(w2u, w2u)); w2i = wtw(bb::mont_mul_centred(w2u, j4_m));
}
__device__ __forceinline__ uint4 scale4(uint4 v, uint32_t g) {
  int32_t x[4] = {(int32_t)v.x, (int32_t)v.y, (int32_t)v.z, (int32_t)v.w};
  bb::wscale4(x, g);
  return make_uint4((uint32_t)x[0], (uint32_t)x[1], (uint32_t)x[2], (uint32_t)x[3]);
}
__device__ __forceinline__ void dit2w4(uint4& a, uint4& b, WTw w) {
#define ZKIR_Q(c) { int32_t p = (int32_t)a.c, q = (int32_t)b.c; bb::dit2w(p, q, w.w, w.n); a.c = (uint32_t)p; b.c = (uint32_t)q; }
  ZKIR_Q(x) ZKIR_Q(y) ZKIR_Q(z) ZKIR_Q(w)
#undef ZKIR_Q
}
__device__ __forceinline__ uint4 canon4(uint4 v) { return make_uint4(bb::wcanon((int32_t)v.x), bb::wcanon((int32_t)v.y), bb::wcanon((int32_t)v.z), bb::wcanon((int32_t)v.w)); }

// ---- one radix-2 stage straight through global memory (odd stage counts only; one lane = one butterfly of four columns) -----
template <bool DIT>
__global__ __launch_bounds__(NT) void ntt_stage_kernel(uint4* __restrict__ data, uint64_t blk_u4, int L, int s0, const uint32_t* __restrict__ tw, int canon) {
  uint4* x = data + (uint64_t)blockIdx.y * blk_u4;
  const uint64_t item = (uint64_t)blockIdx.x * NT + threadIdx.x;              // (pair t, half h)
  const uint32_t n = 1u << L;
  if (item >= (uint64_t)n) return;                                             // n/2 pairs x 2 halves
  const uint32_t t = (uint32_t)(item >> 1), h = (uint32_t)(item & 1);
  uint32_t p, stride, w;
  if (DIT) { stride = 1u << s0; const uint32_t hi = t >> s0, lo = t & (stride - 1); p = (hi << (s0 + 1)) + lo; w = tw[lo << (L - s0 - 1)]; }
  else { stride = n >> (s0 + 1); const uint32_t hi = t / stride, lo = t % stride; p = hi * (n >> s0) + lo; w = tw[bitrev(hi, s0) << (L - s0 - 1)]; }   // the block's twiddle
  uint4 a = x[(uint64_t)p * 2 + h], b = x[(uint64_t)(p + stride) * 2 + h];
  dit2w4(a, b, wtw(bb::centre(w)));                                            // both directions multiply first: (a + w b, a - w b)
  if (DIT && canon) { a = canon4(a); b = canon4(b); }
  x[(uint64_t)p * 2 + h] = a; x[(uint64_t)(p + stride) * 2 + h] = b;
}

// ---- EXPERIMENT (round 4, profiles/HISTORY.md): the first inverse pass GENERATING its input instead of reading it — blocks 0 and 1 of the main trace (cycle, pc limbs,
// the instruction's fields, the limbs of R1, R2 and R3's first: nothing but loads of the row's own trace words) are computed in the load stage from the
// 372-B trace, so main_trace_kernel need not write them and this pass need not read them back.  Words as stark.hip: main_trace_row writes them.
struct TraceSrc01 { zkir_trace_columns t; uint64_t n_real; };
__device__ __forceinline__ u32x4 trace_quad01(const TraceSrc01& q, uint32_t blk, uint32_t half, uint64_t i) {
  const bool pad = i >= q.n_real;
  const uint64_t src = pad ? q.n_real - 1 : i;
  u32x4 r;
  if (blk == 0 && half == 0) {
    const uint64_t pcv = q.t.pc[src];
    r.x = (uint32_t)((q.t.cycle[src] + (i - src)) % bb::P); r.y = (uint32_t)(pcv & 0xFFFFF); r.z = (uint32_t)((pcv >> 20) & 0xFFFFF); r.w = (uint32_t)(pcv >> 40);
  } else if (blk == 0) {
    const uint32_t w = q.t.instruction[src];
    r.x = w & 0x7F; r.y = (w >> 7) & 0xF; r.z = (w >> 11) & 0xF; r.w = (w >> 15) & 0xF;
  } else {
    auto limbs = [&](int g, uint32_t out[3]) {
      const uint64_t o = (uint64_t)g * q.t.reg_stride + src;
      const uint64_t v = q.t.registers[o];
      const int bits = q.t.reg_state[o] ? 30 : 20;
      const uint64_t mask = (1ull << bits) - 1;
      out[0] = (uint32_t)(v & mask); out[1] = (uint32_t)((v >> bits) & mask); out[2] = (uint32_t)(v >> (2 * bits));
    };
    uint32_t a[3], b[3];
    if (half == 0) { limbs(1, a); r.x = q.t.instruction[src] >> 19; r.y = a[0]; r.z = a[1]; r.w = a[2]; }
    else { limbs(2, a); limbs(3, b); r.x = a[0]; r.y = a[1]; r.z = a[2]; r.w = b[0]; }
  }
  return r;
}

// ---- strided radix-4 pass: 2R radix-2 stages (R register-resident radix-4 rounds) over tiles of 2^(2R) rows x 2^C positions, in
// place, one column block per blockIdx.y.  With R = 5 a single pass covers ten stages (tile 1024 x 2 positions x 32 B = 64 KiB of
// LDS), so a 2^20-row matrix needs ONE strided pass on each side of the fused middle kernel.  A lane owns one quad of positions and
// runs it for both halves of the block (eight columns) with one set of twiddles: a read of a compact table (root of order <= 1024 /
// 2048) times a per-lane running power (forward) or a per-tile uniform factor (inverse; 1 in a pass that starts at stage 0, which then
// reads nothing but the tile); the other stage's twiddle is its square and the odd pair's is its product with a 4th root.
// LDS holds the two halves as separate planes so that consecutive lanes touch consecutive 16-byte words.
template <bool DIT, int R, int C, int NTH, bool FUSED = false>
__global__ __launch_bounds__(NTH) void ntt_strided_r4_kernel(uint4* __restrict__ data, uint64_t blk_u4, uint32_t tiles_per_block, uint32_t total, int L, int s0,
                                                              const uint32_t* __restrict__ tw, const uint32_t* __restrict__ small, int log_small, uint32_t j4_m, int canon, TraceSrc01 fsrc = TraceSrc01{},
                                                              uint32_t* zflags = nullptr, uint32_t epoch = 0, int produce = 0) {
  constexpr int B = 2 * R;
  constexpr uint32_t POS = 1u << (B + C), QUADS = POS / 4, CMASK = (1u << C) - 1, PLANE = POS + 4;       // +4: the two planes start in different banks
  constexpr uint32_t MOVES = 2 * POS / NTH;
  static_assert(QUADS % NTH == 0 && NTH % (1 << C) == 0 && (2 * POS) % NTH == 0, "tile / thread geometry");
  extern __shared__ uint4 lds4[];                                              // [2][PLANE]
  const uint32_t n = 1u << L;
  const uint32_t stride_mid = DIT ? (1u << s0) : (n >> (s0 + B));
  const uint32_t lo_tiles = stride_mid >> C;
  // Persistent workgroups: each walks the (block, tile) work list with a stride of the grid and keeps the NEXT tile's 16-byte loads
  // in flight (registers) while it runs the radix-4 rounds of the current one — with one or two workgroups per CU (64-128 KiB of LDS
  // each) nothing else would hide the global-memory latency of a tile load behind arithmetic.
  auto geometry = [&](uint32_t w, uint4*& x, uint32_t& base, uint32_t& lo0, uint32_t& hi) {
    const uint32_t tile = w % tiles_per_block;
    x = data + (uint64_t)(w / tiles_per_block) * blk_u4;
    hi = tile / lo_tiles;
    lo0 = (tile % lo_tiles) << C;
    base = (DIT ? (hi << (s0 + B)) : hi * (n >> s0)) + lo0;
  };
  static_assert(QUADS == NTH, "one quad per lane and round");
  u32x4 pre[MOVES];
  uint4* x; uint32_t base, lo0, hi;
  // All-zero column blocks (zflags != nullptr; the word of block b holds `epoch` once some tile of it was seen non-zero by THIS lde_run): every pass is linear, tile
  // by tile, so a zero tile stays a zero tile.  The chain's first inverse pass (`produce`) is the one that reads `in`: it finds out, tile by tile, skips the rounds and the
  // copy-out of a zero tile (in place: the tile already holds zeros) and stamps the block of every other tile.  The kernels launched after it read the stamps ONCE, before
  // their first prefetch, into a wave-uniform bit mask (at most 64 blocks: host.h) and step past the tiles of unstamped blocks in their walk over the work list: the
  // middle kernel has written zeros there, and zero is canonical.
  uint64_t live = ~0ull;
  if (zflags && !produce) { const uint32_t l = threadIdx.x & 63; live = __ballot(l < total / tiles_per_block && zflags[l] == epoch); }
  auto next_live = [&](uint32_t ww) { while (ww < total && !((live >> (ww / tiles_per_block)) & 1)) ww += gridDim.x; return ww; };
  uint32_t w = next_live(blockIdx.x);
  if (w >= total) return;
  // vmcnt retires IN ORDER: a table read issued after the next tile's prefetch would make its s_waitcnt drain the whole prefetch
  // before the first round starts (rocm 7.2 emitted s_waitcnt vmcnt(0) in round 0 for exactly that) — so nothing is read from global
  // memory between the issue of a prefetch and its use.  The compact-table factors depend on (lane, round) only: read ONCE per
  // workgroup; the tile-dependent factors of the NEXT tile (forward: the power tw[lo << ..]; inverse, s0 > 0: one uniform factor per round) are
  // fetched as the last loads of that tile's prefetch.
  uint32_t sm[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int b = 2 * r;
    const uint32_t qq = threadIdx.x >> C;
    if (!DIT) sm[r] = small[bitrev(qq >> (B - 2 - b), b) << (log_small - (b + 2))];          // root of order 2^(b+2), exponent brv_b(block inside the tile)
    else sm[r] = small[(qq & ((1u << b) - 1)) << (log_small - (b + 2))];
  }
  const bool unit = s0 == 0;                                                   // inverse: the tile factor is 1
  uint32_t tf_next[R] = {};                                                    // inverse, s0 > 0: tw[brv_s0(hi) << (L - s0 - 2r - 2)]
  auto tile_factors = [&](uint32_t hi_t) {
    if (DIT || unit) return;
    const uint32_t e = bitrev(hi_t, s0);
#pragma unroll
    for (int r = 0; r < R; r++) tf_next[r] = tw[e << (L - s0 - 2 * r - 2)];
  };
  geometry(w, x, base, lo0, hi);
  static_for<0, (int)MOVES>([&](auto kc) {                                     // tile rows are 2^C consecutive positions = 2^(C+1) uint4
    constexpr uint32_t k = decltype(kc)::value;
    const uint32_t e = threadIdx.x + k * NTH, row = e >> (C + 1), wv = e & ((2u << C) - 1);
    if constexpr (FUSED) pre[k] = trace_quad01(fsrc, w / tiles_per_block, wv & 1, (uint64_t)base + (uint64_t)row * stride_mid + (wv >> 1));
    else pre[k] = ld4(&x[((uint64_t)base + (uint64_t)row * stride_mid) * 2 + wv]);
  });
  uint32_t tw_cur = 0;
  if (DIT) tw_cur = tw[(lo0 + (threadIdx.x & CMASK)) << (L - s0 - B)];
  tile_factors(hi);
  for (;;) {
    uint32_t nz = 0;                                           // produce: the OR of the lane's words of this tile
    static_for<0, (int)MOVES>([&](auto kc) {
      constexpr uint32_t k = decltype(kc)::value;
      const uint32_t e = threadIdx.x + k * NTH, row = e >> (C + 1), wv = e & ((2u << C) - 1);
      st4(&lds4[(wv & 1) * PLANE + ((row << C) | (wv >> 1))], pre[k]);
      if (produce) nz |= (pre[k].x | pre[k].y) | (pre[k].z | pre[k].w);
    });
    uint32_t tp[R];                                            // forward: per-lane power used by round r; inverse: this tile's uniform factor of round r
    if (DIT) {                                                 // round r needs w^(lo << (L-1-s0-(2r+1))): finest at r = R-1, each earlier round is its 4th power
      uint32_t u = tw_cur;
#pragma unroll
      for (int r = R - 1; r >= 0; r--) { tp[r] = u; u = bb::mont_mul(u, u); u = bb::mont_mul(u, u); }
    } else {
#pragma unroll
      for (int r = 0; r < R; r++) tp[r] = tf_next[r];
    }
    bool dense = true;
    if (produce) {
      dense = __syncthreads_or(nz != 0) != 0;                  // the barrier in front of round 0, with the tile test riding on it
      if (dense && threadIdx.x == 0) zflags[w / tiles_per_block] = epoch;          // (every non-zero tile of the block stores the same word)
    } else {
      __syncthreads();
    }
    const uint32_t wn = next_live(w + gridDim.x);
    uint4* xn = x; uint32_t base_n = base, lo0_n = lo0, hi_n = hi;
    if (wn < total) {                                          // next tile: loads issued now, consumed after this tile's rounds
      geometry(wn, xn, base_n, lo0_n, hi_n);
      static_for<0, (int)MOVES>([&](auto kc) {
        constexpr uint32_t k = decltype(kc)::value;
        const uint32_t e = threadIdx.x + k * NTH, row = e >> (C + 1), wv = e & ((2u << C) - 1);
        if constexpr (FUSED) pre[k] = trace_quad01(fsrc, wn / tiles_per_block, wv & 1, (uint64_t)base_n + (uint64_t)row * stride_mid + (wv >> 1));
        else pre[k] = ld4(&xn[((uint64_t)base_n + (uint64_t)row * stride_mid) * 2 + wv]);
      });
      if (DIT) tw_cur = tw[(lo0_n + (threadIdx.x & CMASK)) << (L - s0 - B)];
      tile_factors(hi_n);
    }
    if (dense) {
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int b = 2 * r;
#pragma unroll
      for (uint32_t k = 0; k < QUADS / NTH; k++) {
        uint32_t q = threadIdx.x + k * NTH;
        // (the LDS addresses are recomputed each round — a handful of full-rate instructions; hoisted out of the tile loop, as the compiler would have
        //  them, the ten of them push the 1024-lane instance past its 128 registers.  The empty asm only hides q's origin from the optimiser; what it buys depends
        //  on the compiler, so the register counts of profiles/*_isa_hist.txt are to be re-read after a toolchain change)
        asm volatile("" : "+v"(q));
        const uint32_t lo_l = q & CMASK, qq = q >> C;
        uint4* pl0 = lds4; uint4* pl1 = lds4 + PLANE;
        if constexpr (!DIT) {
          const int lg = B - 2 - b;                            // log2(h2) in row units
          const uint32_t h2 = 1u << lg, mid_lo = qq & (h2 - 1), mid_hi = qq >> lg;
          const uint32_t i0 = ((((mid_hi << (lg + 2)) | mid_lo)) << C) | lo_l, d = h2 << C;
          WTw w1, w2, w2i;                                     // the BLOCK's twiddles: (lane, round) root x the tile's uniform factor
          ct_twiddles(sm[r], tp[r], unit, j4_m, w1, w2, w2i);
          // the wide quad holds 64-bit sums: one half at a time keeps the kernel inside 128 registers
          uint4 x0 = pl0[i0], x1 = pl0[i0 + d], x2 = pl0[i0 + 2 * d], x3 = pl0[i0 + 3 * d];
          ct4w4(x0, x1, x2, x3, w1, w2, w2i);
          pl0[i0] = x0; pl0[i0 + d] = x1; pl0[i0 + 2 * d] = x2; pl0[i0 + 3 * d] = x3;
          __builtin_amdgcn_sched_barrier(0);
          uint4 y0 = pl1[i0], y1 = pl1[i0 + d], y2 = pl1[i0 + 2 * d], y3 = pl1[i0 + 3 * d];
          ct4w4(y0, y1, y2, y3, w1, w2, w2i);
          pl1[i0] = y0; pl1[i0 + d] = y1; pl1[i0 + 2 * d] = y2; pl1[i0 + 3 * d] = y3;
        } else {
          const uint32_t dm = 1u << b, mid_lo = qq & (dm - 1), mid_hi = qq >> b;
          const uint32_t i0 = ((((mid_hi << (b + 2)) | mid_lo)) << C) | lo_l, d = dm << C;
          const WTw w2 = wtw(bb::mont_mul_centred(tp[r], sm[r]));               // centred; its canonical form derives the other two
          const uint32_t w2u = bb::wcanon(w2.w);
          const WTw w1 = wtw(bb::mont_mul_centred(w2u, w2u)), w2i = wtw(bb::mont_mul_centred(w2u, j4_m));
          // the wide quad holds 64-bit sums: one half at a time keeps the kernel inside 128 registers
          uint4 x0 = pl0[i0], x1 = pl0[i0 + d], x2 = pl0[i0 + 2 * d], x3 = pl0[i0 + 3 * d];
          dit4w4(x0, x1, x2, x3, w1, w2, w2i);
          pl0[i0] = x0; pl0[i0 + d] = x1; pl0[i0 + 2 * d] = x2; pl0[i0 + 3 * d] = x3;
          __builtin_amdgcn_sched_barrier(0);
          uint4 y0 = pl1[i0], y1 = pl1[i0 + d], y2 = pl1[i0 + 2 * d], y3 = pl1[i0 + 3 * d];
          dit4w4(y0, y1, y2, y3, w1, w2, w2i);
          pl1[i0] = y0; pl1[i0 + d] = y1; pl1[i0 + 2 * d] = y2; pl1[i0 + 3 * d] = y3;
        }
      }
      // A wave's 64 quads (2^(6-C) values of qq) cover one contiguous "home block" of 4 * 2^(6-C) rows in every round whose quad span
      // fits it: inverse rounds with log2(h2) <= 6 - C (the spans shrink: every later round fits too), DIT rounds with b <= 6 - C.  Between two such
      // rounds the data never leaves the wave.
      const bool wave_local = !DIT ? (r + 1 < R && B - 2 - b <= 6 - C) : (r + 1 < R && b + 2 <= 6 - C);
      if (wave_local) wave_sync_lds(); else __syncthreads();
    }
#pragma unroll
    for (uint32_t k = 0; k < MOVES; k++) {
      const uint32_t e = threadIdx.x + k * NTH, row = e >> (C + 1), wv = e & ((2u << C) - 1);
      uint4 v = lds4[(wv & 1) * PLANE + ((row << C) | (wv >> 1))];
      if (DIT && canon) v = canon4(v);                       // the chain's last forward pass: (-p, p) -> [0, p)
      x[((uint64_t)base + (uint64_t)row * stride_mid) * 2 + wv] = v;
    }
    }                                                          // (a zero tile of the producing pass: no rounds, nothing to store)
    if (wn >= total) break;
    w = wn; x = xn; base = base_n; lo0 = lo0_n; hi = hi_n;
    // (no barrier here: a lane refills exactly the LDS words it has just copied out — the copy-in and copy-out loops share one slot map —
    //  and the barrier after the refill orders everything before the first round; after a skipped zero tile nothing has read LDS at all)
  }
}

// ---- register-only pass of S = 2 or 3 stages (radix 4 / 8), no LDS: what is left over once the ten-stage LDS passes are taken
// (stage counts of 12 = 10 + 2, 13 = 10 + 3, 11 = 8 + 3 ...).  One lane = one (position, half-block) = four columns; it loads its 2^S
// rows (16 bytes each, consecutive lanes on consecutive 16-byte words), runs the S stages in registers and stores them back: 8 B per
// element of HBM traffic for S stages, where the tiny-tile LDS pass (2 stages) followed by the single-stage pass moved 16 B for 3.
// Twiddles: one table read (the finest stage's; inverse: the factor of the lane's block hi) and its squares, times the constant 4th / 8th roots.
template <bool DIT, int S>
__global__ __launch_bounds__(NT) void ntt_reg_kernel(uint4* __restrict__ data, uint64_t blk_u4, int L, int s0, const uint32_t* __restrict__ tw, uint32_t r4_m, uint32_t r8_m,
                                                       uint32_t r8_3_m, int canon) {
  constexpr int E = 1 << S;
  const uint32_t n = 1u << L;
  uint4* x = data + (uint64_t)blockIdx.y * blk_u4;
  const uint64_t item = (uint64_t)blockIdx.x * NT + threadIdx.x;               // (group t, half h)
  if (item >= ((uint64_t)n >> S) * 2) return;
  const uint32_t t = (uint32_t)(item >> 1), h = (uint32_t)(item & 1);
  const uint32_t d = DIT ? (1u << s0) : (n >> (s0 + S));                       // row distance between the lane's elements
  const uint32_t hi = t / d, lo = t % d;
  const uint64_t base = ((uint64_t)hi * d * E + lo) * 2 + h;
  uint4 v[E];
#pragma unroll
  for (int k = 0; k < E; k++) v[k] = x[base + (uint64_t)k * d * 2];
  if (!DIT) {
    // inverse (multiply first, natural -> bit-reversed): stage j pairs (k, k + E/2^(j+1)) inside blocks of E/2^j; the block m of local stage j has the twiddle
    // T_j * rho_{2^(j+1)}^-brv_j(m), T_j = w^-(brv_s0(hi) << (L - s0 - j - 1)) — one read for the last stage's T, the earlier ones are its squares
    const uint32_t Tf = tw[bitrev(hi, s0) << (L - s0 - S)];
    const uint32_t Tm = bb::mont_mul(Tf, Tf);
    if (S == 3) {                                              // stages 0 and 1 as wide quads on (0, 2, 4, 6) and (1, 3, 5, 7), stage 2 as wide radix-2 butterflies
      const WTw t0 = wtw(bb::mont_mul_centred(Tm, Tm)), tm = wtw(bb::centre(Tm)), m1 = wtw(bb::mont_mul_centred(Tm, r4_m));
#pragma unroll
      for (int g = 0; g < 2; g++) ct4w4(v[g], v[g + 2], v[g + 4], v[g + 6], t0, tm, m1);
      // blocks m = 0..3 of the last stage: rho_8^-brv_2(m) = 1, j, rho_8, rho_8^3
      const WTw wf[4] = {wtw(bb::centre(Tf)), wtw(bb::mont_mul_centred(Tf, r4_m)), wtw(bb::mont_mul_centred(Tf, r8_m)), wtw(bb::mont_mul_centred(Tf, r8_3_m))};
#pragma unroll
      for (int m = 0; m < 4; m++) dit2w4(v[2 * m], v[2 * m + 1], wf[m]);
    } else {
      ct4w4(v[0], v[1], v[2], v[3], wtw(bb::centre(Tm)), wtw(bb::centre(Tf)), wtw(bb::mont_mul_centred(Tf, r4_m)));
    }
  } else {
    // DIT: stage j pairs (k, k + 2^j); twiddle of the pair with low index kl = U_j * rho_{2^(j+1)}^kl, U_(S-1) = w^(lo << (L - s0 - S)), U_(j-1) = U_j^2
    const uint32_t Uf = tw[lo << (L - s0 - S)];
    const uint32_t Um = bb::mont_mul(Uf, Uf);
    if (S == 3) {                                              // stages 0 and 1 as wide quads, stage 2 as wide radix-2 butterflies
      const WTw u0 = wtw(bb::mont_mul_centred(Um, Um)), um = wtw(bb::centre(Um)), m1 = wtw(bb::mont_mul_centred(Um, r4_m));
#pragma unroll
      for (int g = 0; g < 8; g += 4) dit4w4(v[g], v[g + 1], v[g + 2], v[g + 3], u0, um, m1);
      const WTw wf[4] = {wtw(bb::centre(Uf)), wtw(bb::mont_mul_centred(Uf, r8_m)), wtw(bb::mont_mul_centred(Uf, r4_m)), wtw(bb::mont_mul_centred(Uf, r8_3_m))};
#pragma unroll
      for (int k = 0; k < 4; k++) dit2w4(v[k], v[k + 4], wf[k]);
    } else {
      dit4w4(v[0], v[1], v[2], v[3], wtw(bb::centre(Um)), wtw(bb::centre(Uf)), wtw(bb::mont_mul_centred(Uf, r4_m)));
    }
    if (canon) {
#pragma unroll
      for (int k = 0; k < E; k++) v[k] = canon4(v[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < E; k++) x[base + (uint64_t)k * d * 2] = v[k];
}

// CUs of the CURRENT device, cached per device id (one process may drive several GPUs)
inline unsigned cu_count() {
  static std::mutex mu;
  static unsigned cached[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256u;
  std::lock_guard<std::mutex> lk(mu);
  if (!cached[dev]) { hipDeviceProp_t p; cached[dev] = hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0 ? (unsigned)p.multiProcessorCount : 256u; }
  return cached[dev];
}
inline int persist() { static const int v = getenv("ZKIR_NTT_PERSIST") ? atoi(getenv("ZKIR_NTT_PERSIST")) : 1; return v; }

template <bool DIT, int R, int C, int NTH, bool FUSED = false>
void launch_strided_r4(uint32_t* data, uint64_t n, uint32_t n_blocks, int L, int s0, const uint32_t* tw, const uint32_t* small, int log_small, uint32_t j4_m, hipStream_t s,
                       const TraceSrc01* fsrc = nullptr, int canon = 0, uint32_t* zflags = nullptr, uint32_t epoch = 0, int produce = 0) {
  constexpr size_t lds = 16u * 2 * ((1u << (2 * R + C)) + 4);
  auto k = ntt_strided_r4_kernel<DIT, R, C, NTH, FUSED>;
  static std::atomic<uint64_t> attr_done{0};                                   // one bit per device id: the attribute is per (function, device)
  int dev = 0; (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  if (!(attr_done.load(std::memory_order_relaxed) & bit)) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr_done.fetch_or(bit); }
  const uint32_t tiles = (uint32_t)(n >> (2 * R + C)), total = tiles * n_blocks;
  const unsigned per_cu = (unsigned)((160u << 10) / lds) > 0 ? (unsigned)((160u << 10) / lds) : 1u;       // workgroups resident per CU (LDS-limited)
  unsigned grid = persist() ? cu_count() * (per_cu > 8 ? 8 : per_cu) : total;
  if (grid > total) grid = total;
  hipLaunchKernelGGL(k, dim3(grid), dim3(NTH), lds, s, (uint4*)data, 2 * n, tiles, total, L, s0, tw, small, log_small, j4_m, canon, fsrc ? *fsrc : TraceSrc01{}, zflags, epoch, produce);
}

inline int strided_c() { static const int c = getenv("ZKIR_NTT_C") ? atoi(getenv("ZKIR_NTT_C")) : 2; return c; }

// `stages` radix-2 stages starting at s0 in as few passes over the data as possible: LDS radix-4 passes of 10 / 8 / 6 / 4 stages and
// register passes of 3 / 2 stages (13 = 10 + 3, 12 = 10 + 2, 11 = 8 + 3, 9 = 6 + 3, 7 = 4 + 3, 5 = 3 + 2); a lone stage only for 1
// Zero-block flags (see ntt_strided_r4_kernel): with `produce` the chain's FIRST kernel is asked to find out which blocks are non-zero — only an LDS pass can; where a
// register pass comes first nobody finds out and the flags are dropped for the whole chain.  Returns the flag slot the kernels after this chain may read (or nullptr).
// The register and single-stage passes ignore the flags: they turn zeros into zeros.
template <bool DIT>
uint32_t* run_strided_stages(uint32_t* data, uint64_t n, uint32_t n_blocks, int L, int s0, int stages, const uint32_t* tw, const uint32_t* small, int log_small, uint32_t j4_m,
                             uint32_t r8_m, uint32_t r8_3_m, hipStream_t s, uint32_t* zflags = nullptr, uint32_t epoch = 0, bool produce = false) {
  bool first = true;
  while (stages > 0) {
    int take;
    if (stages >= 10 && stages != 11) take = 10;
    else if (stages == 11) take = 8;
    else if (stages == 9) take = 6;
    else if (stages == 7) take = 4;
    else if (stages == 5) take = 3;
    else take = stages;                                          // 8, 6, 4, 3, 2, 1
    const int canon = DIT && take == stages;                     // the chain's last forward kernel hands out canonical words
    int pr = 0;
    if (produce && first) { if (take >= 4) pr = 1; else zflags = nullptr; }
    first = false;
    switch (take) {
      case 10:
        // tile rows of 4 positions = 128 contiguous bytes (a full cache line; 128 KiB of LDS, one workgroup of 16 waves per CU) or of
        // 2 positions = 64 bytes (64 KiB, two workgroups of 8 waves): ZKIR_NTT_C picks (benchmarking), default from the measurements
        if (strided_c() == 2) launch_strided_r4<DIT, 5, 2, 1024>(data, n, n_blocks, L, s0, tw, small, log_small, j4_m, s, nullptr, canon, zflags, epoch, pr);
        else launch_strided_r4<DIT, 5, 1, 512>(data, n, n_blocks, L, s0, tw, small, log_small, j4_m, s, nullptr, canon, zflags, epoch, pr);
        break;
      case 8: launch_strided_r4<DIT, 4, 3, 512>(data, n, n_blocks, L, s0, tw, small, log_small, j4_m, s, nullptr, canon, zflags, epoch, pr); break;
      case 6: launch_strided_r4<DIT, 3, 4, 256>(data, n, n_blocks, L, s0, tw, small, log_small, j4_m, s, nullptr, canon, zflags, epoch, pr); break;
      case 4: launch_strided_r4<DIT, 2, 5, 128>(data, n, n_blocks, L, s0, tw, small, log_small, j4_m, s, nullptr, canon, zflags, epoch, pr); break;
      case 3:
        hipLaunchKernelGGL((ntt_reg_kernel<DIT, 3>), dim3((unsigned)(((n >> 3) * 2 + NT - 1) / NT), n_blocks), dim3(NT), 0, s, (uint4*)data, 2 * n, L, s0, tw, j4_m, r8_m, r8_3_m, canon);
        break;
      case 2:
        hipLaunchKernelGGL((ntt_reg_kernel<DIT, 2>), dim3((unsigned)(((n >> 2) * 2 + NT - 1) / NT), n_blocks), dim3(NT), 0, s, (uint4*)data, 2 * n, L, s0, tw, j4_m, r8_m, r8_3_m, canon);
        break;
      default:
        hipLaunchKernelGGL(ntt_stage_kernel<DIT>, dim3((unsigned)((n + NT - 1) / NT), n_blocks), dim3(NT), 0, s, (uint4*)data, 2 * n, L, s0, tw, canon);
        break;
    }
    s0 += take; stages -= take;
  }
  return zflags;
}

// ---- fused middle for N < 1024 (tests, tiny traces): the whole transform of one column block in LDS, column by column, radix 2 ----
//   g_lo[k & 1023] * g_hi[k >> 10] = g^k * N^-1   (two-level power table, Montgomery form)
__global__ __launch_bounds__(NT) void lde_small_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int L, const uint32_t* __restrict__ small_inv,
                                                        const uint32_t* __restrict__ small_fwd, const uint32_t* __restrict__ g_lo, const uint32_t* __restrict__ g_hi) {
  extern __shared__ uint32_t lds[];                            // 2N words
  const uint32_t n = 1u << L;
  const uint32_t* x = in + (uint64_t)blockIdx.x * n * 8;
  uint32_t* y = out + (uint64_t)blockIdx.x * 2 * n * 8;
  for (int c = 0; c < 8; c++) {
    for (uint32_t e = threadIdx.x; e < n; e += NT) lds[e] = x[(uint64_t)e * 8 + c];
    __syncthreads();
    for (int b = 0; b < L; b++) {                              // inverse DIF stages, half = 2^(L-1-b)
      const int hb = L - 1 - b;
      const uint32_t half = 1u << hb;
      for (uint32_t q = threadIdx.x; q < (n >> 1); q += NT) {
        const uint32_t r_lo = q & (half - 1), r_hi = q >> hb;
        const uint32_t ia = (r_hi << (hb + 1)) | r_lo, ib = ia + half;
        const uint32_t a = lds[ia], bv = lds[ib];
        lds[ia] = bb::add(a, bv); lds[ib] = bb::mont_mul(bb::sub(a, bv), small_inv[r_lo << b]);
      }
      __syncthreads();
    }
    // scale + zero-interleave: position p holds coefficient k = bitrev_L(p); DIT stage 0 duplicates
    uint32_t v[2];
    int cnt = 0;
    for (uint32_t e = threadIdx.x; e < n; e += NT) { const uint32_t k = bitrev(e, L); v[cnt++] = bb::mont_mul(bb::mont_mul(lds[e], g_lo[k & 1023]), g_hi[k >> 10]); }
    __syncthreads();
    cnt = 0;
    for (uint32_t e = threadIdx.x; e < n; e += NT) { lds[2 * e] = v[cnt]; lds[2 * e + 1] = v[cnt]; cnt++; }
    __syncthreads();
    for (int s = 1; s <= L; s++) {                             // forward DIT stages 1..L of the size-2N transform
      const uint32_t half = 1u << s;
      for (uint32_t q = threadIdx.x; q < n; q += NT) {
        const uint32_t r_lo = q & (half - 1), r_hi = q >> s;
        const uint32_t ia = (r_hi << (s + 1)) | r_lo, ib = ia + half;
        const uint32_t a = lds[ia], t = bb::mont_mul(lds[ib], small_fwd[r_lo << (L - s)]);
        lds[ia] = bb::add(a, t); lds[ib] = bb::sub(a, t);
      }
      __syncthreads();
    }
    for (uint32_t e = threadIdx.x; e < 2 * n; e += NT) y[(uint64_t)e * 8 + c] = lds[e];
    __syncthreads();
  }
}

// ---- fused middle, N >= 1024: the last 10 inverse stages (multiply-first, s0 = L - 10: hi = the chunk) on a contiguous chunk of 1024 positions of the size-N block, the coset
// scale g^k / N (k = bit-reversal of the position), zero-interleave, and the first 11 forward-DIT stages of the size-2N transform,
// written as the 2048-position chunk of `out`.  Register-resident radix-4 rounds: 5 + 5 LDS round trips for the 21 stages, one
// twiddle read per quad (inverse: times the chunk's uniform factor of the round; the others are its square and its product with a 4th root of
// unity), shared by the four columns a lane carries.  LDS: A = both halves of the chunk (32 KiB; later the forward buffer of half 1), Bf = the forward buffer of half 0 (32 KiB):
// 64 KiB per workgroup, two workgroups per CU.
constexpr int MID_NT = 512;
__global__ __launch_bounds__(MID_NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void lde_middle_r4_kernel(const uint4* __restrict__ in, uint4* __restrict__ out, uint32_t chunks_per_block, uint32_t total, int L,
                                                                const uint32_t* __restrict__ tw_inv, const uint32_t* __restrict__ small_inv, const uint32_t* __restrict__ small_fwd,
                                                                const uint32_t* __restrict__ g_lo, const uint32_t* __restrict__ g_hi, uint32_t j4_inv_m, uint32_t j4_fwd_m, int canon,
                                                                const uint32_t* __restrict__ zflags, uint32_t epoch) {
  constexpr int Bm = 10;
  constexpr uint32_t APL = 1024;
  __shared__ uint4 A[2 * APL];
  __shared__ uint4 Bf[2048];
  const uint32_t n = 1u << L, t = threadIdx.x;
  // All-zero column blocks (zflags != nullptr: the stamps of the chain's first inverse pass, see ntt_strided_r4_kernel; read once, before the first prefetch): the chunk
  // of an unstamped block is not fetched — its 2048 positions of `out` (which holds whatever the last call left there) are written as zeros, both planes of a position
  // from one lane, the store shape of a computed chunk.  The walk zero-fills such chunks on its way to the next chunk that has to be computed.
  uint64_t live = ~0ull;
  if (zflags) { const uint32_t l = t & 63; live = __ballot(l < total / chunks_per_block && zflags[l] == epoch); }
  auto next_live = [&](uint32_t ww) {
    for (; ww < total && !((live >> (ww / chunks_per_block)) & 1); ww += gridDim.x) {
      uint4* yz = out + (uint64_t)(ww / chunks_per_block) * n * 4 + ((uint64_t)(ww % chunks_per_block) << (Bm + 2));
#pragma unroll
      for (int k = 0; k < 4; k++) { const uint32_t e = t + k * MID_NT; yz[2 * e] = make_uint4(0, 0, 0, 0); yz[2 * e + 1] = make_uint4(0, 0, 0, 0); }
    }
    return ww;
  };
  // persistent workgroups with the next chunk's loads in flight during the 15 rounds of the current one (see the strided kernel)
  uint32_t w = next_live(blockIdx.x);
  if (w >= total) return;
  // vmcnt retires in order (see the strided kernel): no global read between the issue of the next chunk's prefetch and its use.
  // The compact-table twiddles of the ten rounds depend on (lane, round) only: read once per workgroup.  The coset scale of the lane's four
  // positions and the five uniform factors of the inverse rounds depend on the chunk: they come with the chunk's prefetch, as its last loads, and are
  // consumed (gs, cf) at the top of the chunk, BEFORE the next prefetch is issued.
  uint32_t tw_i[5], tw_f[5];
#pragma unroll
  for (int r = 0; r < 5; r++) {
    const int lg = 8 - 2 * r;
    tw_i[r] = small_inv[bitrev((t & 255) >> lg, 2 * r) << lg];                 // w_(2^(2r+2))^-brv_2r(block inside the chunk)
    const int sft = 2 * r + 1;
    tw_f[r] = small_fwd[(t & ((1u << sft) - 1)) << (Bm - sft - 1)];            // w_2048^(lo << (9-s)): twiddle of stage s+1
  }
  u32x4 pre[4];
  uint32_t cf_next[5];                                         // tw_inv[brv_(L-10)(chunk) << (8 - 2r)]: the chunk's factor of inverse round r
  uint32_t glo[4], ghi[4];                                     // factors of g^k / N for the lane's four positions 4q .. 4q + 3 of the last inverse round, k = bitrev_L(position)
  auto fetch = [&](uint32_t ww) {                              // one chunk's loads, in the order they are consumed: the 1024 positions, then the scale factors
    const uint4* x = in + ((uint64_t)(ww / chunks_per_block) * n + ((uint64_t)(ww % chunks_per_block) << Bm)) * 2;
#pragma unroll
    for (int k = 0; k < 4; k++) pre[k] = ld4(&x[t + k * MID_NT]);
    const uint32_t p0 = ((ww % chunks_per_block) << Bm) + 4 * (t & 255);
#pragma unroll
    for (int i = 0; i < 4; i++) { const uint32_t k = bitrev(p0 + i, L); glo[i] = g_lo[k & 1023]; ghi[i] = g_hi[k >> 10]; }
    const uint32_t ce = bitrev(ww % chunks_per_block, L - Bm);
#pragma unroll
    for (int r = 0; r < 5; r++) cf_next[r] = tw_inv[ce << (8 - 2 * r)];
  };
  fetch(w);
  for (;;) {
    const uint32_t base = (w % chunks_per_block) << Bm;
    uint4* y = out + (uint64_t)(w / chunks_per_block) * n * 4;
#pragma unroll
    for (int k = 0; k < 4; k++) { const uint32_t e = t + k * MID_NT; st4(&A[(e & 1) * APL + (e >> 1)], pre[k]); }
    uint32_t gs[4];
#pragma unroll
    for (int i = 0; i < 4; i++) gs[i] = bb::mont_mul(glo[i], ghi[i]);
    uint32_t cf[5];
#pragma unroll
    for (int r = 0; r < 5; r++) cf[r] = cf_next[r];
    __syncthreads();
    const uint32_t wn = next_live(w + gridDim.x);               // (the zero-fill stores of skipped chunks go out BEFORE the prefetch is issued)
    if (wn < total) fetch(wn);
    // ---- inverse, rounds r = 0..4: stages (2r, 2r+1) of the chunk, spans h1 = 2^(9-2r), h2 = h1/2; lane = (quad q, half h); block = hi ----
    {
      const uint32_t q = t & 255;
      uint4* a = A + (t >> 8) * APL;
#pragma unroll
      for (int r = 0; r < 5; r++) {
        const int lg = 8 - 2 * r;                              // log2(h2)
        const uint32_t h2 = 1u << lg, lo = q & (h2 - 1), hi = q >> lg;
        const uint32_t i0 = (hi << (lg + 2)) | lo;
        WTw c1, c2, c2i;
        ct_twiddles(tw_i[r], cf[r], false, j4_inv_m, c1, c2, c2i);
        uint4 x0 = a[i0], x1 = a[i0 + h2], x2 = a[i0 + 2 * h2], x3 = a[i0 + 3 * h2];
        ct4w4(x0, x1, x2, x3, c1, c2, c2i);
        if (r == 4) {                                          // last round (positions 4q..4q+3, i0 = 4q): the coset scale g^k / N, one signed product per word
          x0 = scale4(x0, gs[0]); x1 = scale4(x1, gs[1]); x2 = scale4(x2, gs[2]); x3 = scale4(x3, gs[3]);
        }
        a[i0] = x0; a[i0 + h2] = x1; a[i0 + 2 * h2] = x2; a[i0 + 3 * h2] = x3;
        // rounds 1..4 stay inside the wave's own 256 positions of its plane (q = 64 v .. 64 v + 63): only round 0 hands data to other waves
        if (r >= 1 && r < 4) wave_sync_lds(); else __syncthreads();
      }
    }
    // ---- forward DIT of the zero-interleaved chunk (2048 positions), one half of the block at a time: stage 0 is a copy, rounds do
    //      stages (s, s+1), s = 1,3,5,7,9; lane = quad t of 512 ----
    // Half 0 runs its forward rounds in Bf; half 1 then runs them in A itself (A is dead once round 0 of half 1 has read it — one
    // extra barrier between that round's loads and stores), so that both halves of a position are stored TOGETHER: 32 contiguous
    // bytes per lane whose two 16-byte stores meet in L2.  Stored one half at a time, 10 us apart, every 32-byte sector reached HBM
    // twice, half-filled: WRITE_SIZE showed 2.40 GB per launch against 1.28 GB algorithmic (profiles/r02i_bench_commit_pmc_traffic.txt).
#pragma unroll 1
    for (int h = 0; h < 2; h++) {
      const uint4* a = A + h * APL;
      uint4* F = h == 0 ? Bf : A;
#pragma unroll
      for (int r = 0; r < 5; r++) {
        const int s = 2 * r + 1;
        const uint32_t lo = t & ((1u << s) - 1), hi = t >> s;
        const uint32_t i0 = (hi << (s + 2)) | lo, d = 1u << s;
        const uint32_t w2 = tw_f[r];                            // w_2048^(lo << (9-s)): twiddle of stage s+1
        const WTw c2 = wtw(bb::centre(w2)), c1 = wtw(bb::mont_mul_centred(w2, w2)), c2i = wtw(bb::mont_mul_centred(w2, j4_fwd_m));
        uint4 x0, x1, x2, x3;
        if (r == 0) {                                          // after stage 0: F[j] = A[j >> 1]
          x0 = a[i0 >> 1]; x1 = a[(i0 + d) >> 1]; x2 = a[(i0 + 2 * d) >> 1]; x3 = a[(i0 + 3 * d) >> 1];
          __syncthreads();                                     // half 1 overwrites what it has just read
        } else { x0 = F[i0]; x1 = F[i0 + d]; x2 = F[i0 + 2 * d]; x3 = F[i0 + 3 * d]; }
        dit4w4(x0, x1, x2, x3, c1, c2, c2i);
        F[i0] = x0; F[i0 + d] = x1; F[i0 + 2 * d] = x2; F[i0 + 3 * d] = x3;
        // rounds 0..2 (spans up to 128) stay inside the wave's own 256 positions [256 v, 256 v + 256) of F; rounds 3 and 4 cross waves
        if (r < 2) wave_sync_lds(); else __syncthreads();
      }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t e = t + k * MID_NT;
      uint4 v0 = Bf[e], v1 = A[e];
      if (canon) { v0 = canon4(v0); v1 = canon4(v1); }        // log_n = 10: no strided forward pass follows
      y[((uint64_t)2 * base + e) * 2] = v0; y[((uint64_t)2 * base + e) * 2 + 1] = v1;
    }
    __syncthreads();
    if (wn >= total) break;
    w = wn;
  }
}


// ---- blow-up 4 and 8 (log_blowup b = 2, 3): the same pass structure with M = N 2^b output rows.  Coefficient k of the padded input sits at position brv_L(k) << b of the
// bit-reversed size-M array, so forward stages 0 .. b-1 only replicate every coefficient 2^b times and stages b .. b+9 stay inside a chunk of 1024 * 2^b output positions.
// For a fixed residue r of the output position mod 2^b those ten stages touch only positions of that residue: the chunk is 2^b INDEPENDENT 1024-point transforms of the SAME
// 1024 scaled coefficients, one per coset 31 w_M^r <w_N>, and the twiddle of local stage s at position c of residue r is w_(2^(s+1))^(c mod 2^s) * w_(2^(s+b+1))^r.
//
// lde_middle_blowup_kernel<LB>: the inverse half is that of lde_middle_r4_kernel (A = both column planes of the chunk, 32 KiB) except for the hand-off after its last round: a
// wave-local wait where the shipped kernel has a workgroup barrier, because forward round 0 here reads only the lane's own positions 4q .. 4q + 3.  The
// forward half then runs ONE RESIDUE AT A TIME, both planes together, in F (32 KiB): 64 KiB per workgroup and two workgroups per CU at every b, where a whole b = 3 chunk
// (2 x 128 KiB) could not be resident at all.  A lane owns (quad q, plane h) as on the inverse side; round 0 reads A (which every residue needs again) and writes F.  A lane's
// twiddle of round rho for residue r is its residue-0 twiddle times w_(2^(2 rho + b + 2))^r: a running product, five multiplications per lane and residue, no table read
// inside the chunk loop (the prefetch discipline of the strided kernel: nothing is read from global memory between the issue of the next chunk's prefetch and its use).
// Rounds 0 .. 3 (spans up to 64) stay inside a wave's own 256 positions of its plane; only round 4 crosses waves.
// Stores: output position (c << b) | r takes both planes from one lane, 32 contiguous bytes = one full sector per lane (half-filled sectors reach HBM twice: see the
// comment in lde_middle_r4_kernel); the lanes of a wave are 32 << b bytes apart, and the 2^b residues of a 128-byte line are written within one chunk's time.
template <int LB>
__global__ __launch_bounds__(MID_NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void lde_middle_blowup_kernel(const uint4* __restrict__ in, uint4* __restrict__ out, uint32_t chunks_per_block, uint32_t total, int L,
                                                                const uint32_t* __restrict__ tw_inv, const uint32_t* __restrict__ small_inv, const uint32_t* __restrict__ small_fwd,
                                                                const uint32_t* __restrict__ g_lo, const uint32_t* __restrict__ g_hi, uint32_t j4_inv_m, uint32_t j4_fwd_m, int canon) {
  static_assert(LB == 2 || LB == 3, "blow-up 4 or 8 (blow-up 2: lde_middle_r4_kernel)");
  constexpr int Bm = 10;
  constexpr uint32_t APL = 1024;
  __shared__ uint4 A[2 * APL];
  __shared__ uint4 F[2 * APL];
  const uint32_t n = 1u << L, t = threadIdx.x;
  uint32_t w = blockIdx.x;
  if (w >= total) return;
  uint32_t tw_i[5], tw_f[5], step[5];
#pragma unroll
  for (int r = 0; r < 5; r++) {
    const int lg = 8 - 2 * r;
    tw_i[r] = small_inv[bitrev((t & 255) >> lg, 2 * r) << lg];                 // w_(2^(2r+2))^-brv_2r(block inside the chunk)
    const int s = 2 * r;                                                       // forward round r = local stages (s, s + 1); small_fwd has order 2^(10 + LB)
    tw_f[r] = small_fwd[((t & 255) & ((1u << s) - 1)) << (LB + lg)];           // w_(2^(s+2))^lo: stage s + 1 at residue 0
    step[r] = small_fwd[1u << lg];                                             // w_(2^(s+LB+2)): from one residue to the next
  }
  u32x4 pre[4];
  uint32_t cf_next[5];                                         // tw_inv[brv_(L-10)(chunk) << (8 - 2r)]: the chunk's factor of inverse round r
  uint32_t glo[4], ghi[4];                                     // factors of g^k / N for the lane's four positions 4q .. 4q + 3 of the last inverse round, k = bitrev_L(position)
  auto fetch = [&](uint32_t ww) {                              // one chunk's loads, in the order they are consumed: the 1024 positions, then the scale factors
    const uint4* x = in + ((uint64_t)(ww / chunks_per_block) * n + ((uint64_t)(ww % chunks_per_block) << Bm)) * 2;
#pragma unroll
    for (int k = 0; k < 4; k++) pre[k] = ld4(&x[t + k * MID_NT]);
    const uint32_t p0 = ((ww % chunks_per_block) << Bm) + 4 * (t & 255);
#pragma unroll
    for (int i = 0; i < 4; i++) { const uint32_t k = bitrev(p0 + i, L); glo[i] = g_lo[k & 1023]; ghi[i] = g_hi[k >> 10]; }
    const uint32_t ce = bitrev(ww % chunks_per_block, L - Bm);
#pragma unroll
    for (int r = 0; r < 5; r++) cf_next[r] = tw_inv[ce << (8 - 2 * r)];
  };
  fetch(w);
  const uint32_t q = t & 255;
  uint4* a = A + (t >> 8) * APL;                               // the lane's plane, both sides
  uint4* f = F + (t >> 8) * APL;
  for (;;) {
    const uint32_t base = (w % chunks_per_block) << Bm;
    uint4* y = out + ((uint64_t)(w / chunks_per_block) * n << (LB + 1));
#pragma unroll
    for (int k = 0; k < 4; k++) { const uint32_t e = t + k * MID_NT; st4(&A[(e & 1) * APL + (e >> 1)], pre[k]); }
    uint32_t gs[4];
#pragma unroll
    for (int i = 0; i < 4; i++) gs[i] = bb::mont_mul(glo[i], ghi[i]);
    uint32_t cf[5];
#pragma unroll
    for (int r = 0; r < 5; r++) cf[r] = cf_next[r];
    __syncthreads();
    const uint32_t wn = w + gridDim.x;
    if (wn < total) fetch(wn);
    // ---- inverse, rounds r = 0..4 (lde_middle_r4_kernel) ----
#pragma unroll
    for (int r = 0; r < 5; r++) {
      const int lg = 8 - 2 * r;                                // log2(h2)
      const uint32_t h2 = 1u << lg, lo = q & (h2 - 1), hi = q >> lg;
      const uint32_t i0 = (hi << (lg + 2)) | lo;
      WTw c1, c2, c2i;
      ct_twiddles(tw_i[r], cf[r], false, j4_inv_m, c1, c2, c2i);
      uint4 x0 = a[i0], x1 = a[i0 + h2], x2 = a[i0 + 2 * h2], x3 = a[i0 + 3 * h2];
      ct4w4(x0, x1, x2, x3, c1, c2, c2i);
      if (r == 4) { x0 = scale4(x0, gs[0]); x1 = scale4(x1, gs[1]); x2 = scale4(x2, gs[2]); x3 = scale4(x3, gs[3]); }
      a[i0] = x0; a[i0 + h2] = x1; a[i0 + 2 * h2] = x2; a[i0 + 3 * h2] = x3;
      // rounds 1..4 stay inside the wave's own 256 positions of its plane; round 4's results are read next by forward round 0 of the SAME wave (positions 4q .. 4q + 3)
      if (r >= 1) wave_sync_lds(); else __syncthreads();
    }
    // ---- forward, one residue at a time: the 1024-point DIT of A on the coset of residue res, both planes, in F ----
    uint32_t twl[5];                                           // the lane's twiddle of round r at the current residue
#pragma unroll
    for (int r = 0; r < 5; r++) twl[r] = tw_f[r];
#pragma unroll 1
    for (uint32_t res = 0; res < (1u << LB); res++) {
#pragma unroll
      for (int r = 0; r < 5; r++) {
        const int s = 2 * r;
        const uint32_t lo = q & ((1u << s) - 1), hi = q >> s;
        const uint32_t i0 = (hi << (s + 2)) | lo, d = 1u << s;
        const uint32_t w2 = twl[r];
        const WTw c2 = wtw(bb::centre(w2)), c1 = wtw(bb::mont_mul_centred(w2, w2)), c2i = wtw(bb::mont_mul_centred(w2, j4_fwd_m));
        twl[r] = bb::mont_mul(w2, step[r]);
        uint4 x0, x1, x2, x3;
        if (r == 0) { x0 = a[i0]; x1 = a[i0 + 1]; x2 = a[i0 + 2]; x3 = a[i0 + 3]; }           // the replicated coefficients: every residue starts from A
        else { x0 = f[i0]; x1 = f[i0 + d]; x2 = f[i0 + 2 * d]; x3 = f[i0 + 3 * d]; }
        dit4w4(x0, x1, x2, x3, c1, c2, c2i);
        f[i0] = x0; f[i0 + d] = x1; f[i0 + 2 * d] = x2; f[i0 + 3 * d] = x3;
        // rounds 0..3 (spans up to 64) stay inside the wave's own 256 positions [256 v, 256 v + 256) of its plane of F; round 4 crosses waves
        if (r < 3) wave_sync_lds(); else __syncthreads();
      }
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const uint32_t c = t + k * MID_NT;
        uint4 v0 = F[c], v1 = F[APL + c];
        if (canon) { v0 = canon4(v0); v1 = canon4(v1); }      // log_n = 10: no strided forward pass follows
        const uint64_t o = ((((uint64_t)base + c) << LB) | res) * 2;
        y[o] = v0; y[o + 1] = v1;
      }
      __syncthreads();                                         // F is rewritten by the next residue's round 0, A by the next chunk
    }
    if (wn >= total) break;
    w = wn;
  }
}

// ---- N < 1024 at blow-up 2^b, b = 2, 3: lde_small_kernel with 2^b copies of every scaled coefficient and forward stages b .. L+b-1 of the size-M transform
//      (small_fwd: w_(2^(L+b))^k, k < 2^(L+b-1); LDS: M words, at most 16 KiB) ----
__global__ __launch_bounds__(NT) void lde_small_blowup_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int L, int lb, const uint32_t* __restrict__ small_inv,
                                                               const uint32_t* __restrict__ small_fwd, const uint32_t* __restrict__ g_lo, const uint32_t* __restrict__ g_hi) {
  extern __shared__ uint32_t lds[];                            // M words
  const uint32_t n = 1u << L, m = n << lb;
  const uint32_t* x = in + (uint64_t)blockIdx.x * n * 8;
  uint32_t* y = out + (uint64_t)blockIdx.x * m * 8;
  for (int c = 0; c < 8; c++) {
    for (uint32_t e = threadIdx.x; e < n; e += NT) lds[e] = x[(uint64_t)e * 8 + c];
    __syncthreads();
    for (int b = 0; b < L; b++) {                              // inverse DIF stages, half = 2^(L-1-b)
      const int hb = L - 1 - b;
      const uint32_t half = 1u << hb;
      for (uint32_t q = threadIdx.x; q < (n >> 1); q += NT) {
        const uint32_t r_lo = q & (half - 1), r_hi = q >> hb;
        const uint32_t ia = (r_hi << (hb + 1)) | r_lo, ib = ia + half;
        const uint32_t a = lds[ia], bv = lds[ib];
        lds[ia] = bb::add(a, bv); lds[ib] = bb::mont_mul(bb::sub(a, bv), small_inv[r_lo << b]);
      }
      __syncthreads();
    }
    // scale + replicate: position p holds coefficient k = bitrev_L(p); DIT stages 0 .. lb-1 copy it to positions (p << lb) .. (p << lb) + 2^lb - 1
    uint32_t v[2];                                             // n <= 512: at most two positions per lane
    int cnt = 0;
    for (uint32_t e = threadIdx.x; e < n; e += NT) { const uint32_t k = bitrev(e, L); v[cnt++] = bb::mont_mul(bb::mont_mul(lds[e], g_lo[k & 1023]), g_hi[k >> 10]); }
    __syncthreads();
    cnt = 0;
    for (uint32_t e = threadIdx.x; e < n; e += NT) { for (uint32_t i = 0; i < (1u << lb); i++) lds[(e << lb) + i] = v[cnt]; cnt++; }
    __syncthreads();
    for (int s = lb; s < L + lb; s++) {                        // forward DIT stages lb .. L+lb-1 of the size-M transform
      const uint32_t half = 1u << s;
      for (uint32_t q = threadIdx.x; q < (m >> 1); q += NT) {
        const uint32_t r_lo = q & (half - 1), r_hi = q >> s;
        const uint32_t ia = (r_hi << (s + 1)) | r_lo, ib = ia + half;
        const uint32_t a = lds[ia], tt = bb::mont_mul(lds[ib], small_fwd[r_lo << (L + lb - 1 - s)]);
        lds[ia] = bb::add(a, tt); lds[ib] = bb::sub(a, tt);
      }
      __syncthreads();
    }
    for (uint32_t e = threadIdx.x; e < m; e += NT) y[(uint64_t)e * 8 + c] = lds[e];
    __syncthreads();
  }
}

}  // namespace

namespace zkir {

// in: n_blocks x [N][8] canonical evaluations over H (natural order; used as scratch and overwritten!), out: n_blocks x [N << t.log_blowup][8]
void lde_run(const LdeTables& t, uint32_t* in, uint32_t n_blocks, uint32_t* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int L = t.log_n;
  const uint32_t N = 1u << L;
  static const uint32_t j4_inv_m = bb::to_mont(bb::inv(bb::root_of_unity(2))), j4_fwd_m = bb::to_mont(bb::root_of_unity(2));
  static const uint32_t r8_fwd = bb::root_of_unity(3), r8_inv = bb::inv(r8_fwd);
  static const uint32_t r8_inv_m = bb::to_mont(r8_inv), r8_inv3_m = bb::to_mont(bb::mul(bb::mul(r8_inv, r8_inv), r8_inv));
  static const uint32_t r8_fwd_m = bb::to_mont(r8_fwd), r8_fwd3_m = bb::to_mont(bb::mul(bb::mul(r8_fwd, r8_fwd), r8_fwd));
  const int LB = t.log_blowup;
  if (LB != 1) {                                                 // blow-up 4 / 8: the same three steps with their own middle (and small) kernel; the strided kernels are generic
    if (L < 10) {
      hipLaunchKernelGGL(lde_small_blowup_kernel, dim3(n_blocks), dim3(NT), (4u << (L + LB)), s, in, out, L, LB, t.small_inv, t.small_fwd, t.g_lo, t.g_hi);
      return;
    }
    run_strided_stages<false>(in, N, n_blocks, L, 0, L - 10, t.tw_inv, t.small_inv, 10, j4_inv_m, r8_inv_m, r8_inv3_m, s);
    const uint32_t chunks = N >> 10, total = chunks * n_blocks;
    unsigned grid = persist() ? cu_count() * 2 : total;                     // 64 KiB of LDS: two workgroups per CU
    if (grid > total) grid = total;
    auto mid = LB == 2 ? lde_middle_blowup_kernel<2> : lde_middle_blowup_kernel<3>;
    hipLaunchKernelGGL(mid, dim3(grid), dim3(MID_NT), 0, s, (const uint4*)in, (uint4*)out, chunks, total, L, t.tw_inv, t.small_inv, t.small_fwd, t.g_lo, t.g_hi, j4_inv_m, j4_fwd_m, L == 10);
    // forward DIT strided stages 10 + b .. L + b - 1 of the size-M transform (tw_fwd: w_M^k, small_fwd: order 2^(10 + b))
    run_strided_stages<true>(out, (uint64_t)N << LB, n_blocks, L + LB, 10 + LB, L - 10, t.tw_fwd, t.small_fwd, 10 + LB, j4_fwd_m, r8_fwd_m, r8_fwd3_m, s);
    return;
  }
  if (L < 10) {
    hipLaunchKernelGGL(lde_small_kernel, dim3(n_blocks), dim3(NT), (8u << L), s, in, out, L, t.small_inv, t.small_fwd, t.g_lo, t.g_hi);
    return;
  }
  // inverse strided stages 0 .. L-11 (multiply-first; the compact table then has order 1024).  The caller's flag slot (host.h) is used where the chain's first kernel is an
  // LDS pass (log_n >= 14, != 15) and the blocks fit the kernels' 64-bit mask; otherwise every kernel gets a null pointer and runs exactly as without the slot.
  uint32_t* zf = t.zero_slot && t.zero_epoch && n_blocks <= ZERO_FLAG_BLOCKS ? t.zero_slot : nullptr;
  zf = run_strided_stages<false>(in, N, n_blocks, L, 0, L - 10, t.tw_inv, t.small_inv, 10, j4_inv_m, r8_inv_m, r8_inv3_m, s, zf, t.zero_epoch, zf != nullptr);
  {
    const uint32_t chunks = N >> 10, total = chunks * n_blocks;
    unsigned grid = persist() ? cu_count() * 2 : total;                     // 64 KiB of LDS: two workgroups per CU
    if (grid > total) grid = total;
    hipLaunchKernelGGL(lde_middle_r4_kernel, dim3(grid), dim3(MID_NT), 0, s, (const uint4*)in, (uint4*)out, chunks, total, L, t.tw_inv, t.small_inv, t.small_fwd, t.g_lo, t.g_hi,
                       j4_inv_m, j4_fwd_m, L == 10, (const uint32_t*)zf, t.zero_epoch);
  }
  // forward DIT strided stages 11 .. L of the size-2N transform
  run_strided_stages<true>(out, (uint64_t)2 * N, n_blocks, L + 1, 11, L - 10, t.tw_fwd, t.small_fwd, 11, j4_fwd_m, r8_fwd_m, r8_fwd3_m, s, zf, t.zero_epoch);
}


// EXPERIMENT (profiles/r04*_lde_tile_variants.txt): ONE strided pass at stage 0 over n_blocks blocks of 2^log_n rows with a chosen tile geometry — the timing of the
// tilings side by side on the same data (the values are a partial transform: only the time means anything);
// a forward pass is launched without `canon`, so it leaves signed words in (-p, p), not field elements).
//   0: 10 stages, 1024 rows x 4 positions (128-byte rows), 128 KiB, 1024 lanes: one workgroup per CU   (what lde_run uses)
//   1: 10 stages, 1024 rows x 2 positions (64-byte rows),   64 KiB,  512 lanes: two per CU
//   2:  8 stages,  256 rows x 8 positions (256-byte rows),  64 KiB,  512 lanes: two per CU
//   3:  8 stages,  256 rows x 4 positions (128-byte rows),  32 KiB,  256 lanes: four or five per CU
//   4:  6 stages,   64 rows x 16 positions,                 32 KiB,  256 lanes
bool strided_variant_run(const LdeTables& t, uint32_t* data, uint32_t n_blocks, int variant, bool dit, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int L = dit ? t.log_n + 1 : t.log_n;
  if (t.log_n < 20) return false;
  const uint64_t n = (uint64_t)1 << L;
  static const uint32_t j4_inv_m = bb::to_mont(bb::inv(bb::root_of_unity(2))), j4_fwd_m = bb::to_mont(bb::root_of_unity(2));
  const uint32_t* tw = dit ? t.tw_fwd : t.tw_inv; const uint32_t* sm = dit ? t.small_fwd : t.small_inv;
  const int ls = dit ? 11 : 10; const uint32_t j4 = dit ? j4_fwd_m : j4_inv_m; const int s0 = dit ? 11 : 0;
#define ZKIR_VARIANT(R, C, NTH) do { if (dit) launch_strided_r4<true, R, C, NTH>(data, n, n_blocks, L, s0, tw, sm, ls, j4, s); else launch_strided_r4<false, R, C, NTH>(data, n, n_blocks, L, s0, tw, sm, ls, j4, s); } while (0)
  switch (variant) {
    case 0: ZKIR_VARIANT(5, 2, 1024); break;
    case 1: ZKIR_VARIANT(5, 1, 512); break;
    case 2: ZKIR_VARIANT(4, 3, 512); break;
    case 3: ZKIR_VARIANT(4, 2, 256); break;
    case 4: ZKIR_VARIANT(3, 4, 256); break;
    default: return false;
  }
#undef ZKIR_VARIANT
  return true;
}

// EXPERIMENT: the same extension with blocks 0 and 1 of `in` NOT read by the first inverse pass — generated from the trace instead (trace_quad01).  Only for
// traces whose first inverse pass is the ten-stage one (log_n >= 20, log_n != 21); returns false (nothing launched) otherwise.
bool lde_run_fused01(const LdeTables& t, const zkir_trace_columns* trace, uint64_t n_real, uint32_t* in, uint32_t n_blocks, uint32_t* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int L = t.log_n;
  if (L < 20 || L == 21 || n_blocks < 3 || strided_c() != 2) return false;
  const uint32_t N = 1u << L;
  static const uint32_t j4_inv_m = bb::to_mont(bb::inv(bb::root_of_unity(2))), j4_fwd_m = bb::to_mont(bb::root_of_unity(2));
  static const uint32_t r8_fwd = bb::root_of_unity(3), r8_inv = bb::inv(r8_fwd);
  static const uint32_t r8_inv_m = bb::to_mont(r8_inv), r8_inv3_m = bb::to_mont(bb::mul(bb::mul(r8_inv, r8_inv), r8_inv));
  static const uint32_t r8_fwd_m = bb::to_mont(r8_fwd), r8_fwd3_m = bb::to_mont(bb::mul(bb::mul(r8_fwd, r8_fwd), r8_fwd));
  const TraceSrc01 src{*trace, n_real};
  launch_strided_r4<false, 5, 2, 1024, true>(in, N, 2, L, 0, t.tw_inv, t.small_inv, 10, j4_inv_m, s, &src);                         // blocks 0, 1: generated
  launch_strided_r4<false, 5, 2, 1024>(in + (uint64_t)2 * N * 8, N, n_blocks - 2, L, 0, t.tw_inv, t.small_inv, 10, j4_inv_m, s);     // the others: read
  if (L - 10 > 10) run_strided_stages<false>(in, N, n_blocks, L, 10, L - 20, t.tw_inv, t.small_inv, 10, j4_inv_m, r8_inv_m, r8_inv3_m, s);
  {
    const uint32_t chunks = N >> 10, total = chunks * n_blocks;
    unsigned grid = persist() ? cu_count() * 2 : total;
    if (grid > total) grid = total;
    hipLaunchKernelGGL(lde_middle_r4_kernel, dim3(grid), dim3(MID_NT), 0, s, (const uint4*)in, (uint4*)out, chunks, total, L, t.tw_inv, t.small_inv, t.small_fwd, t.g_lo, t.g_hi,
                       j4_inv_m, j4_fwd_m, L == 10, nullptr, 0u);
  }
  run_strided_stages<true>(out, (uint64_t)2 * N, n_blocks, L + 1, 11, L - 10, t.tw_fwd, t.small_fwd, 11, j4_fwd_m, r8_fwd_m, r8_fwd3_m, s);
  return true;
}

}  // namespace zkir
