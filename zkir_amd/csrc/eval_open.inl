// eval_open.inl — zkir_batch_eval_prove and zkir_eval_prove (include/zkir_amd.h): AN EVALUATION PROOF OF ONE OR SEVERAL COMMITMENTS OF ONE HEIGHT, at any rate the context
// serves (log_blowup 1, 2, 3).  Included by stark.hip at file scope after lowdeg.inl, whose sections 2 - 4 (fri.inl's FRI commit phase and grinding, the queries: lowdeg_fri_and_queries) it
// runs unchanged over its own codeword with a list of opened matrices.
//
// Statement: n_mats (1 .. 4) B8 matrices of the context's size (zkir_lde_launch's output: canonical words over 31 <w_M>, M = N << b), each under its own tree
// (zkir_merkle_commit_launch's), have every column close to a polynomial of degree < N, and matrix m's columns take the proof's values at those of the n_points (1 or 2)
// shared, caller-chosen points z_i of E4 outside the base field that mask_m selects.  The evaluations are the barycentric sums over the rows j 2^b (the sub-coset 31 <w_N>),
// whatever a matrix holds.  The gamma exponent e runs consecutively: for i over the points, for m over the matrices with bit i of mask_m set, in order, for k < width_m;
// A_i(x) = sum gamma^e col_{m,k}(x), a_i = sum gamma^e y[i][m][k] over the selected (m, k) of point i, F(x_j) = sum_i (a_i - A_i(x_j)) / (z_i - x_j) over all M rows.
//
// TWO HEADERS STATE IT (verify.cpp).  'ZKBE' (zkir_batch_eval_prove; spec of every word: tests/batch_eval_ref.py) carries n_mats at word 4 and a (width, mask)
// pair per matrix after word 8.  'ZKEV' (zkir_eval_prove; spec: tests/eval_ref.py) is the batch of ONE matrix, which the rule "every point is used by some matrix" forces to
// a full mask: it carries the width at word 4 and no pairs.  From the roots on — points, evaluations, FRI part, queries — the two are one format, and one prover
// (eval_prove_impl) writes both.
//
// What a batch shares: ONE inverse table and weights table (eval_weights_kernel, one E4 inversion per (point, row) whatever the number of matrices), ONE pass that writes the
// codeword, one FRI commit phase, one grind, one set of query rows.  What stays per matrix: the evaluations (eval_dot_kernel with NP = the number of points the matrix is
// opened at and the weight rows of exactly those points) and the opening records.  The codeword pass is eval_quotient_kernel for one matrix and batch_quotient_kernel for
// several (eval_launch_quotient): the only place where the number of matrices changes the device work.
//
// THE INVERSES ARE TABLED, NOT RECOMPUTED: eval_weights_kernel writes 1 / (z_i - x_j) for all M rows once (16 n_points bytes a row), and the quotient kernels read them back.
// An E4 inversion is ~60 dependent Montgomery products (the base-field power p - 2) — about what the quotient kernel spends on 150 columns of one point — so recomputing it
// per row would put the one HBM-bound pass of the proof at its ALU limit; the table adds 32 n_points bytes of traffic to a row that reads 32 ceil(width / 8) (5 - 10 % at
// 152 columns).  The table is the proof's largest workspace next to the codeword: 16 n_points M bytes.
namespace {

constexpr uint32_t EVAL_MAGIC = 0x56454B5Au, BATCH_MAGIC = 0x45424B5Au, EVAL_VERSION = 1;   // 'ZKEV', 'ZKBE'
constexpr uint32_t EVAL_MAX_POINTS = 2, BATCH_MAX_MATS = OPEN_MAX_MATS, BATCH_MAX_TOTAL_WIDTH = LOWDEG_MAX_WIDTH;
// eval_quotient_kernel, batch_quotient_kernel: each of their 96-bit sums takes one product gamma^e[t] * v per column of every matrix opened at its point, at most
// BATCH_MAX_TOTAL_WIDTH terms, as lowdeg_combine_kernel's do
static_assert(bb::P < (1u << 31) && BATCH_MAX_TOTAL_WIDTH / 4 <= (1u << 9), "eval_quotient_kernel, batch_quotient_kernel: a 96-bit sum's top word stays below 2^9");

struct EvalPoints { E4 z_m[EVAL_MAX_POINTS]; };        // the points, Montgomery
struct EvalScales { E4 s_m[EVAL_MAX_POINTS]; };        // ((z_i / 31)^N - 1) / N, Montgomery
struct EvalClaims { E4 a[EVAL_MAX_POINTS]; };          // a_i = sum_k gamma^(i width + k) y[i][k], canonical

// ---- 1 / (z_i - x_j) for all M rows (dinv[i M + j]) and x_j / (z_i - x_j) for the sub-coset's N rows j 2^b (wts[i N + j]); Montgomery E4 -----------------------------------
// One lane per (point, row), one E4 inversion each: the points are arbitrary, nothing is shared between them.  Either table may be absent (the test entries want one of
// them): without dinv only the sub-coset's rows are inverted.
__global__ __launch_bounds__(NT) void eval_weights_kernel(uint32_t log_M, uint32_t b, uint32_t n_points, const uint32_t* __restrict__ tw_fwd, EvalPoints pts, E4* __restrict__ wts,
                                                         E4* __restrict__ dinv) {
  const uint64_t M = 1ull << log_M, idx = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= (uint64_t)n_points * M) return;
  const uint32_t i = (uint32_t)(idx >> log_M);
  const uint64_t j = idx & (M - 1);
  const bool sub = (j & ((1u << b) - 1)) == 0;
  if (!dinv && !sub) return;
  const uint32_t wj = j < M / 2 ? tw_fwd[j] : bb::neg(tw_fwd[j - M / 2]);        // R w_M^j: the table holds the first half, the second is its negation
  const uint32_t x = bb::mont_mul(wj, bb::to_mont(bb::GEN));
  E4 d = i ? pts.z_m[1] : pts.z_m[0];
  d.c[0] = bb::sub(d.c[0], x);
  const E4 di = bb::e_inv_m(d);
  if (dinv) dinv[(uint64_t)i * M + j] = di;
  if (wts && sub) wts[(uint64_t)i * (M >> b) + (j >> b)] = bb::e_mul_fm(di, x);
}

// ---- partial[(i 8 n_blocks + col) n_chunks + chunk] = sum over the chunk's sub-coset rows r of mat[col][r 2^b] * wts[i][r]  (CANONICAL E4) ------------------------------------
// bary_dot_kernel's shape with the rate as a parameter: grid = chunks x B8 blocks; a QUAD of lanes takes one row of a block, every lane of it the row's 32 bytes and ONE
// coordinate t = lane & 3 of the n_points weights, and keeps 8 columns x NP exact 96-bit sums (bb::mad96).  The row stride is 2^b and every offset is 64-bit (block 18 of 2^27
// rows starts past 2^32 words).  The words are canonical and the weights Montgomery (R e): the reduction's division by R leaves the canonical sum, so the partial sums and
// their total are canonical and eval_sum_kernel's one Montgomery product with R scale leaves the canonical evaluation.
// Terms per 96-bit sum: a lane takes per / EVAL_ROWS rows of its chunk, and eval_chunks keeps that at or below BARY_MAX_TERMS (acc96_div_R's bound).
constexpr uint32_t EVAL_ROWS = NT / 4;                         // rows a workgroup takes per iteration
inline uint32_t eval_chunks(uint64_t N) {
  return N > 64ull * EVAL_ROWS * BARY_MAX_TERMS ? (uint32_t)(N / (EVAL_ROWS * BARY_MAX_TERMS)) : N >= 1024 * NT ? 256 : N >= 64 * NT ? 64 : N >= 16 * NT ? 16 : 1;
}
constexpr uint32_t EVAL_MAX_CHUNKS = (uint32_t)((1ull << 26) / (EVAL_ROWS * BARY_MAX_TERMS));      // at log_n = 26
// rows a lane takes = N / n_chunks / EVAL_ROWS: BARY_MAX_TERMS exactly above 2^23 rows; below, the largest N of each range over its chunk count (1, 16, 64, 256 chunks)
static_assert(EVAL_MAX_CHUNKS == 512 && (16ull * NT) / EVAL_ROWS <= BARY_MAX_TERMS && (64ull * NT / 16) / EVAL_ROWS <= BARY_MAX_TERMS &&
              (1024ull * NT / 64) / EVAL_ROWS <= BARY_MAX_TERMS && (64ull * EVAL_ROWS * BARY_MAX_TERMS / 256) / EVAL_ROWS <= BARY_MAX_TERMS,
              "eval_chunks: at most BARY_MAX_TERMS rows per lane in every range of N");
template <int NP>
struct EvalRow { uint4 xa, xb; uint32_t w[NP]; };
template <int NP>
__device__ __forceinline__ EvalRow<NP> eval_load(const uint4* __restrict__ v4, const uint32_t* __restrict__ w32, uint64_t N, uint32_t b, uint64_t r, uint32_t t) {
  EvalRow<NP> x;
#pragma unroll
  for (int i = 0; i < NP; i++) x.w[i] = w32[4 * ((uint64_t)i * N + r) + t];
  x.xa = v4[(r << b) * 2]; x.xb = v4[(r << b) * 2 + 1];
  return x;
}
template <int NP>
__device__ __forceinline__ void eval_mads(const EvalRow<NP>& r, bb::Acc96 (*a)[NP]) {
  const uint32_t x[8] = {r.xa.x, r.xa.y, r.xa.z, r.xa.w, r.xb.x, r.xb.y, r.xb.z, r.xb.w};
#pragma unroll
  for (int c = 0; c < 8; c++)
#pragma unroll
    for (int i = 0; i < NP; i++) bb::mad96(a[c][i], r.w[i], x[c]);
}
template <int NP>
__global__ __launch_bounds__(NT, BARY_WAVES) void eval_dot_kernel(const uint32_t* __restrict__ mat, uint32_t width, uint64_t N, uint32_t b, const E4* __restrict__ wts, E4* __restrict__ partial,
                                                                uint32_t n_chunks, uint32_t log_per) {
  __shared__ uint32_t red[NT / 64][8][NP][4];
  const uint32_t blk = blockIdx.y, n_blocks = gridDim.y, chunk = blockIdx.x;
  const uint4* __restrict__ v4 = reinterpret_cast<const uint4*>(mat) + (uint64_t)blk * (N << b) * 2;
  const uint32_t* __restrict__ w32 = reinterpret_cast<const uint32_t*>(wts);
  const uint64_t per = 1ull << log_per, lo = (uint64_t)chunk << log_per;             // N / n_chunks, a power of two
  const uint32_t t = threadIdx.x & 3, rq = threadIdx.x >> 2;
  bb::Acc96 a[8][NP];
#pragma unroll
  for (int c = 0; c < 8; c++)
#pragma unroll
    for (int i = 0; i < NP; i++) a[c][i] = bb::acc96_zero();
  uint64_t r = lo + rq;
  if (per >= 2 * EVAL_ROWS) {
    // every lane makes the same per / EVAL_ROWS iterations (a power of two): two rows in flight while two are multiplied, as in bary_dot_kernel
    const uint32_t n_it = (uint32_t)(per / EVAL_ROWS);
    EvalRow<NP> r0 = eval_load<NP>(v4, w32, N, b, r, t), r1 = eval_load<NP>(v4, w32, N, b, r + EVAL_ROWS, t);
    for (uint32_t it = 0; it < n_it; it += 2) {
      const uint64_t rn = it + 2 < n_it ? r + 2 * EVAL_ROWS : r;             // (the last pair is loaded twice: nothing is read outside the chunk)
      const EvalRow<NP> n0 = eval_load<NP>(v4, w32, N, b, rn, t), n1 = eval_load<NP>(v4, w32, N, b, rn + EVAL_ROWS, t);
      eval_mads<NP>(r0, a); eval_mads<NP>(r1, a);
      r0 = n0; r1 = n1; r = rn;
    }
  } else {
    for (; r < lo + per; r += EVAL_ROWS) eval_mads<NP>(eval_load<NP>(v4, w32, N, b, r, t), a);      // fewer rows than a workgroup takes: the other quads hold zero sums
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 8; c++)
#pragma unroll
    for (int i = 0; i < NP; i++) {
      uint32_t s = bb::acc96_div_R(a[c][i]);
      for (int off = 32; off >= 4; off >>= 1) s = bb::add(s, __shfl_down(s, off, 64));      // lanes of one coordinate: lane & 3 is kept by every step
      if (lane < 4) red[wv][c][i][lane] = s;
    }
  __syncthreads();
  if (threadIdx.x < 32 * NP) {
    const uint32_t c = threadIdx.x / (4 * NP), i = (threadIdx.x >> 2) % NP, tt = threadIdx.x & 3;
    uint32_t s = red[0][c][i][tt];
    for (int k = 1; k < NT / 64; k++) s = bb::add(s, red[k][c][i][tt]);
    if (blk * 8 + c < width) partial[((uint64_t)i * 8 * n_blocks + blk * 8 + c) * n_chunks + chunk].c[tt] = s;      // a ragged last block: its unused columns do not count
  }
}

// the chunks' partial sums of (point, column) added up and scaled: out[i width + k] = scale_i * sum, canonical.  One wave per sum (bary_sum_kernel).
__global__ __launch_bounds__(NT) void eval_sum_kernel(const E4* __restrict__ partial, uint32_t width, uint32_t n_blocks, uint32_t n_points, uint32_t n_chunks, EvalScales sc, E4* __restrict__ out) {
  const uint32_t idx = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;           // idx = i width + k
  if (idx >= n_points * width) return;
  const uint32_t i = idx / width, k = idx % width;
  E4 a = bb::e_zero();
  for (uint32_t q = lane; q < n_chunks; q += 64) a = bb::e_add(a, partial[((uint64_t)i * 8 * n_blocks + k) * n_chunks + q]);
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int t = 0; t < 4; t++) a.c[t] = bb::add(a.c[t], __shfl_down(a.c[t], off, 64));
  if (lane == 0) out[idx] = bb::e_mul_m(a, i ? sc.s_m[1] : sc.s_m[0]);
}

// ---- F(x_j) = sum_i (a_i - A_i(x_j)) / (z_i - x_j), one lane per row ----------------------------------------------------------------------------------------------------------
// lowdeg_combine_kernel's loads (the two 16-byte halves of (block, row), 64-bit offsets, the next block's pair requested before the current one is multiplied in) feeding
// NP x 4 exact 96-bit sums: gpow[(i n_blocks + blk) 8 + u] = R gamma^(i width + 8 blk + u), zero for the columns a ragged last block does not have (uniform reads, scalar
// registers).  Canonical words x Montgomery powers: the reduction leaves the canonical A_i; (a_i - A_i) canonical times the tabled Montgomery inverse is the canonical term.
template <int NP>
__global__ __launch_bounds__(NT, DEEP_WAVES) void eval_quotient_kernel(const uint32_t* __restrict__ mat, uint32_t n_blocks, uint64_t M, const E4* __restrict__ gpow, const E4* __restrict__ dinv,
                                                                     EvalClaims cl, uint32_t* __restrict__ cw) {
  const uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (j >= M) return;
  const uint4* __restrict__ M4 = reinterpret_cast<const uint4*>(mat);
  bb::Acc96 A[NP][4];
#pragma unroll
  for (int i = 0; i < NP; i++)
#pragma unroll
    for (int t = 0; t < 4; t++) A[i][t] = bb::acc96_zero();
  uint4 nlo = M4[j * 2], nhi = M4[j * 2 + 1];
#pragma unroll 1
  for (uint32_t blk = 0; blk < n_blocks; blk++) {
    const uint4 vlo = nlo, vhi = nhi;
    if (blk + 1 < n_blocks) { nlo = M4[((uint64_t)(blk + 1) * M + j) * 2]; nhi = M4[((uint64_t)(blk + 1) * M + j) * 2 + 1]; }
    const uint32_t v[8] = {vlo.x, vlo.y, vlo.z, vlo.w, vhi.x, vhi.y, vhi.z, vhi.w};
#pragma unroll
    for (int u = 0; u < 8; u++)
#pragma unroll
      for (int i = 0; i < NP; i++) {
        const E4 g = gpow[((uint64_t)i * n_blocks + blk) * 8 + u];
#pragma unroll
        for (int t = 0; t < 4; t++) bb::mad96_s(A[i][t], g.c[t], v[u]);
      }
  }
  E4 f = bb::e_zero();
#pragma unroll
  for (int i = 0; i < NP; i++) {
    const E4 Ai{{bb::acc96_div_R(A[i][0]), bb::acc96_div_R(A[i][1]), bb::acc96_div_R(A[i][2]), bb::acc96_div_R(A[i][3])}};
    f = bb::e_add(f, bb::e_mul_m(bb::e_sub(cl.a[i], Ai), dinv[(uint64_t)i * M + j]));
  }
#pragma unroll
  for (int t = 0; t < 4; t++) cw[(uint64_t)t * M + j] = f.c[t];
}

// the matrices as the batch's quotient kernel takes them, by value (kernel arguments: scalar registers)
struct BatchMats { const uint32_t* mat[BATCH_MAX_MATS]; uint32_t n_blocks[BATCH_MAX_MATS]; uint32_t mask[BATCH_MAX_MATS]; uint32_t n_mats; uint32_t total_blocks; };

// ---- F(x_j) = sum_i (a_i - A_i(x_j)) / (z_i - x_j) over ALL the matrices, one lane per row, written once ---------------------------------------------------------------------
// eval_quotient_kernel's loads (the two 16-byte halves of (block, row), 64-bit offsets) streamed over the blocks of every matrix in turn: the next pair is requested before
// the current one is multiplied in, also from a matrix's last block to the next matrix's first.  The loop over the matrices is unrolled (at most four), so the struct is
// indexed by constants only and its fields stay in scalar registers; the loop over a matrix's blocks is not.
// gpow[(i total_blocks + g) 8 + u] = R gamma^e of column 8 blk + u of the matrix whose block blk is the batch's g-th, at point i.  CHOSEN: the table holds zeros for the
// columns a ragged last block does not have (whatever sits there is multiplied by zero, as in eval_quotient_kernel — a per-column test would cost more than the product),
// but a point the matrix is NOT opened at is skipped on the mask: the mask is a kernel argument, the branch is wave-uniform and scalar, and it saves 32 wide products a block
// (a quotient matrix opened at one point of two pays for one).  The table's entries of a skipped (point, block) are never read.
// Registers (the compiler's resource-usage remarks for gfx950, with stark.hip's max-ILP scheduler): 56 VGPRs at NP = 1 (8 waves a SIMD), 88 at NP = 2 (5 waves), no scratch,
// no spill — exactly eval_quotient_kernel's counts, so the matrix loop costs no register.  The live state is NP x 4 sums of three words (24 at NP = 2), two pairs of 16-byte
// loads and the addresses; the rest is what the scheduler spends on interleaving the 64 independent product chains of a block.  The launch bound asks for DEEP_WAVES (4)
// as a floor, as eval_quotient_kernel does, and does not constrain the allocator at these sizes.  A bound of 8 waves (64 VGPRs) at NP = 2 would buy three more waves to
// hide HBM latency at the price of the interleaving; it is not measured here and is left as it is.
template <int NP>
__global__ __launch_bounds__(NT, DEEP_WAVES) void batch_quotient_kernel(BatchMats bm, uint64_t M, const E4* __restrict__ gpow, const E4* __restrict__ dinv, EvalClaims cl, uint32_t* __restrict__ cw) {
  const uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (j >= M) return;
  bb::Acc96 A[NP][4];
#pragma unroll
  for (int i = 0; i < NP; i++)
#pragma unroll
    for (int t = 0; t < 4; t++) A[i][t] = bb::acc96_zero();
  const uint4* __restrict__ first = reinterpret_cast<const uint4*>(bm.mat[0]);
  uint4 nlo = first[j * 2], nhi = first[j * 2 + 1];
  uint32_t g = 0;                                                            // the batch's block count so far
#pragma unroll
  for (int m = 0; m < (int)BATCH_MAX_MATS; m++) {
    if ((uint32_t)m >= bm.n_mats) break;
    const uint4* __restrict__ M4 = reinterpret_cast<const uint4*>(bm.mat[m]);
    const uint32_t n_blocks = bm.n_blocks[m], mask = bm.mask[m];
#pragma unroll 1
    for (uint32_t blk = 0; blk < n_blocks; blk++, g++) {
      const uint4 vlo = nlo, vhi = nhi;
      if (blk + 1 < n_blocks) { nlo = M4[((uint64_t)(blk + 1) * M + j) * 2]; nhi = M4[((uint64_t)(blk + 1) * M + j) * 2 + 1]; }
      else if (m + 1 < (int)BATCH_MAX_MATS && (uint32_t)(m + 1) < bm.n_mats) {
        const uint4* __restrict__ N4 = reinterpret_cast<const uint4*>(bm.mat[m + 1 < (int)BATCH_MAX_MATS ? m + 1 : m]);
        nlo = N4[j * 2]; nhi = N4[j * 2 + 1];
      }
      const uint32_t v[8] = {vlo.x, vlo.y, vlo.z, vlo.w, vhi.x, vhi.y, vhi.z, vhi.w};
#pragma unroll
      for (int i = 0; i < NP; i++) {
        if (!((mask >> i) & 1)) continue;                                    // wave-uniform: the matrix is not opened at point i
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const E4 gp = gpow[((uint64_t)i * bm.total_blocks + g) * 8 + u];
#pragma unroll
          for (int t = 0; t < 4; t++) bb::mad96_s(A[i][t], gp.c[t], v[u]);
        }
      }
    }
  }
  E4 f = bb::e_zero();
#pragma unroll
  for (int i = 0; i < NP; i++) {
    const E4 Ai{{bb::acc96_div_R(A[i][0]), bb::acc96_div_R(A[i][1]), bb::acc96_div_R(A[i][2]), bb::acc96_div_R(A[i][3])}};
    f = bb::e_add(f, bb::e_mul_m(bb::e_sub(cl.a[i], Ai), dinv[(uint64_t)i * M + j]));
  }
#pragma unroll
  for (int t = 0; t < 4; t++) cw[(uint64_t)t * M + j] = f.c[t];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------------------------------------------
// the shape of a batch: widths, masks, and what follows from them
struct BatchPlan {
  uint32_t n_mats, n_points, width[BATCH_MAX_MATS], mask[BATCH_MAX_MATS], n_blocks[BATCH_MAX_MATS], first_block[BATCH_MAX_MATS], total_blocks, sum_width;
  uint32_t first_e[EVAL_MAX_POINTS][BATCH_MAX_MATS];                        // the exponent of column 0 of a selected (point, matrix)
  uint32_t n_evals;
  bool sel(uint32_t i, uint32_t m) const { return (mask[m] >> i) & 1; }
};
// why != nullptr: what is wrong with the shape (n_points is known to be 1 or 2)
const char* batch_plan(uint32_t n_mats, const uint32_t* widths, const uint32_t* masks, uint32_t n_points, BatchPlan* out) {
  if (n_mats < 1 || n_mats > BATCH_MAX_MATS) return "n_mats must be 1 .. 4";
  BatchPlan p{};
  p.n_mats = n_mats; p.n_points = n_points;
  uint32_t used = 0;
  for (uint32_t m = 0; m < n_mats; m++) {
    if (widths[m] < 1 || widths[m] > LOWDEG_MAX_WIDTH) return "a width of widths is outside 1 .. 512";
    if (masks[m] == 0) return "a mask of masks is 0: the matrix is opened at no point";
    if (masks[m] >> n_points) return "a mask of masks has a bit at or above n_points";
    p.width[m] = widths[m]; p.mask[m] = masks[m]; p.n_blocks[m] = (widths[m] + 7) / 8; p.first_block[m] = p.total_blocks;
    p.total_blocks += p.n_blocks[m]; p.sum_width += widths[m]; used |= masks[m];
  }
  if (p.sum_width > BATCH_MAX_TOTAL_WIDTH) return "the widths sum above 512 (terms per 96-bit sum of the combination)";
  if (used != (1u << n_points) - 1) return "a point of points is opened by no matrix (no mask has its bit)";
  for (uint32_t i = 0; i < n_points; i++) for (uint32_t m = 0; m < n_mats; m++) if (p.sel(i, m)) { p.first_e[i][m] = p.n_evals; p.n_evals += p.width[m]; }
  *out = p;
  return nullptr;
}
// R gamma^e at [(i total_blocks + first_block[m] + blk) 8 + u] for the selected (i, m), k = 8 blk + u < width_m; zero everywhere else.  `g`: R gamma^(the first exponent) —
// one for a proof of one height; a group of mixed_eval.inl goes on where the group before it stopped.
std::vector<E4> batch_gamma_table(const E4& gamma, const BatchPlan& p, E4 g = bb::e_one_m()) {
  std::vector<E4> t((size_t)p.n_points * p.total_blocks * 8, bb::e_zero());
  const E4 gamma_m = bb::e_to_mont(gamma);
  for (uint32_t i = 0; i < p.n_points; i++) for (uint32_t m = 0; m < p.n_mats; m++) if (p.sel(i, m))
    for (uint32_t k = 0; k < p.width[m]; k++) { t[((size_t)i * p.total_blocks + p.first_block[m]) * 8 + k] = g; g = bb::e_mul_m(g, gamma_m); }
  return t;
}
// a_i = sum gamma^e y[e] over the selected (m, k) of point i, canonical (y: canonical words, 4 per evaluation, in the exponent order; gp: batch_gamma_table's)
EvalClaims batch_claims(const std::vector<E4>& gp, const uint32_t* y, const BatchPlan& p) {
  EvalClaims cl{};
  for (uint32_t i = 0; i < p.n_points; i++) {
    E4 a = bb::e_zero();                                                     // Montgomery power x canonical value = canonical
    for (uint32_t m = 0; m < p.n_mats; m++) if (p.sel(i, m))
      for (uint32_t k = 0; k < p.width[m]; k++) {
        const uint32_t* v = y + 4 * ((size_t)p.first_e[i][m] + k);
        a = bb::e_add(a, bb::e_mul_m(gp[((size_t)i * p.total_blocks + p.first_block[m]) * 8 + k], E4{{v[0], v[1], v[2], v[3]}}));
      }
    cl.a[i] = a;
  }
  return cl;
}
// the points as the kernels take them; why != nullptr: what is wrong with them
const char* eval_points_check(const uint32_t* points, uint32_t n_points, EvalPoints* pts) {
  if (n_points < 1 || n_points > EVAL_MAX_POINTS) return "n_points must be 1 or 2";
  for (uint32_t i = 0; i < 4 * n_points; i++) if (points[i] >= bb::P) return "a word of points is not canonical (>= p)";
  for (uint32_t i = 0; i < n_points; i++) if (!(points[4 * i + 1] | points[4 * i + 2] | points[4 * i + 3])) return "a point of points lies in the base field (its coordinates 1 .. 3 are zero)";
  if (n_points == 2 && !memcmp(points, points + 4, 16)) return "the two points of points are equal";
  for (uint32_t i = 0; i < n_points; i++) pts->z_m[i] = bb::e_to_mont(E4{{points[4 * i], points[4 * i + 1], points[4 * i + 2], points[4 * i + 3]}});
  for (uint32_t i = n_points; i < EVAL_MAX_POINTS; i++) pts->z_m[i] = bb::e_zero();
  return nullptr;
}
// ((z_i / 31)^N - 1) / N, Montgomery
EvalScales eval_scales(const EvalPoints& pts, uint32_t n_points, uint32_t log_n) {
  EvalScales sc{};
  const uint32_t ginv_m = bb::to_mont(bb::inv(bb::GEN)), ninv_m = bb::to_mont(bb::inv(1u << log_n));
  for (uint32_t i = 0; i < n_points; i++) {
    E4 e = bb::e_mul_fm(pts.z_m[i], ginv_m);
    for (uint32_t k = 0; k < log_n; k++) e = bb::e_mul_m(e, e);
    e.c[0] = bb::sub(e.c[0], bb::R1);
    sc.s_m[i] = bb::e_mul_fm(e, ninv_m);
  }
  return sc;
}
// the two launches of the evaluations: partial sums, then their totals scaled (y: DEVICE, n_points width E4)
void eval_launch_dot(const zkir_stark_ctx* c, const uint32_t* mat, uint32_t width, uint32_t n_points, const E4* wts, E4* partial, const EvalScales& sc, E4* y, hipStream_t s) {
  const uint64_t N = 1ull << c->log_n;
  const uint32_t n_blocks = (width + 7) / 8, n_chunks = eval_chunks(N), log_per = (uint32_t)__builtin_ctzll(N / n_chunks);
  if (n_points == 1) hipLaunchKernelGGL(eval_dot_kernel<1>, dim3(n_chunks, n_blocks), dim3(NT), 0, s, mat, width, N, c->log_blowup, wts, partial, n_chunks, log_per);
  else hipLaunchKernelGGL(eval_dot_kernel<2>, dim3(n_chunks, n_blocks), dim3(NT), 0, s, mat, width, N, c->log_blowup, wts, partial, n_chunks, log_per);
  hipLaunchKernelGGL(eval_sum_kernel, dim3(grid_for((uint64_t)n_points * width, NT / 64)), dim3(NT), 0, s, partial, width, n_blocks, n_points, n_chunks, sc, y);
}
// the codeword pass.  One matrix (its mask is full: batch_plan) takes eval_quotient_kernel, which profiles/r14_batch_eval.txt has 5 - 10 % ahead of the batch kernel on as
// many blocks; the table is the same array for both and the sums are exact, so the choice cannot change a word.
void eval_launch_quotient(const zkir_stark_ctx* c, const BatchPlan& p, const uint32_t* const* mats, const E4* gpow, const E4* dinv, const EvalClaims& cl, uint32_t* cw, hipStream_t s) {
  const uint64_t M = 1ull << (c->log_n + c->log_blowup);
  if (p.n_mats == 1) {
    if (p.n_points == 1) hipLaunchKernelGGL(eval_quotient_kernel<1>, dim3(grid_for(M)), dim3(NT), 0, s, mats[0], p.total_blocks, M, gpow, dinv, cl, cw);
    else hipLaunchKernelGGL(eval_quotient_kernel<2>, dim3(grid_for(M)), dim3(NT), 0, s, mats[0], p.total_blocks, M, gpow, dinv, cl, cw);
    return;
  }
  BatchMats bm{};
  for (uint32_t m = 0; m < p.n_mats; m++) { bm.mat[m] = mats[m]; bm.n_blocks[m] = p.n_blocks[m]; bm.mask[m] = p.mask[m]; }
  bm.n_mats = p.n_mats; bm.total_blocks = p.total_blocks;
  if (p.n_points == 1) hipLaunchKernelGGL(batch_quotient_kernel<1>, dim3(grid_for(M)), dim3(NT), 0, s, bm, M, gpow, dinv, cl, cw);
  else hipLaunchKernelGGL(batch_quotient_kernel<2>, dim3(grid_for(M)), dim3(NT), 0, s, bm, M, gpow, dinv, cl, cw);
}
void eval_launch_weights(const zkir_stark_ctx* c, uint32_t n_points, const EvalPoints& pts, E4* wts, E4* dinv, hipStream_t s) {
  const uint32_t log_M = c->log_n + c->log_blowup;
  hipLaunchKernelGGL(eval_weights_kernel, dim3(grid_for((uint64_t)n_points << log_M)), dim3(NT), 0, s, log_M, c->log_blowup, n_points, c->d_tw_fwd, pts, wts, dinv);
}

// What an entry tells the one prover: its name (in front of every error message), its words function as the cap_words message names it, and which header it writes.
struct EvalEntry { const char* who; const char* words_call; bool zkev; };
constexpr EvalEntry ENTRY_EVAL{"zkir_eval_prove", "zkir_eval_proof_words(log_n, log_blowup, width, n_points, num_queries)", true};
constexpr EvalEntry ENTRY_BATCH{"zkir_batch_eval_prove", "zkir_batch_eval_proof_words(log_n, log_blowup, n_mats, widths, masks, n_points, num_queries)", false};

constexpr EvalEntry ENTRY_RATE{"zkir_prove_rate", "the embedded evaluation proof's words", false};

// What a proof needs beyond its matrices: the checked shape, the proof's length, the schedule and the arena bytes of its working set.  eval_plan makes every refusal
// that does not look at a matrix or tree pointer, in the entries' order, before anything is launched.
struct EvalPlan {
  EvalPoints pts; BatchPlan p; uint64_t total; std::vector<int> ks; uint32_t n_chunks, np_of[BATCH_MAX_MATS]; size_t n_part[BATCH_MAX_MATS], n_gpow, arena_bytes;
};
int eval_plan(const EvalEntry& en, const zkir_stark_ctx* c, uint32_t n_mats, const uint32_t* widths, const uint32_t* masks, const uint32_t* points, uint32_t n_points,
              uint32_t num_queries, uint32_t pow_bits, uint64_t cap_words, EvalPlan* out) {
  auto bad = [&](const std::string& why) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, std::string(en.who) + ": " + why}); return (int)ZKIR_ERR_ARGUMENT; };
  EvalPlan& e = *out;
  const uint32_t log_n = c->log_n, b = c->log_blowup, log_M = log_n + b;
  if (log_n < 3) return bad("the context's log_n must be at least 3: below that there is no layer to commit");
  if (const char* why = eval_points_check(points, n_points, &e.pts)) return bad(why);
  if (const char* why = batch_plan(n_mats, widths, masks, n_points, &e.p)) return bad(why);
  if (num_queries < 1 || num_queries > 128) return bad("num_queries must be 1 .. 128");
  if (pow_bits > 24) return bad("pow_bits must be 0 .. 24");
  const uint64_t batch_total = zkir_batch_eval_proof_words(log_n, b, n_mats, widths, masks, n_points, num_queries);
  if (batch_total == 0) return bad("the context's log_n / log_blowup are outside what a proof can state (log_n 3 .. 26, log_blowup 1 .. 3, their sum at most 27)");
  e.total = batch_total - (en.zkev ? 2 : 0);                               // 'ZKEV' has no (width, mask) pair
  if (cap_words < e.total) return bad(std::string("cap_words is below ") + en.words_call);
  const uint64_t N = 1ull << log_n, M = 1ull << log_M;
  e.ks = zkir::fri_schedule((int)log_n, (int)b);
  e.n_chunks = eval_chunks(N);
  OpenMat opens[BATCH_MAX_MATS];
  size_t want_part = 0;
  for (uint32_t m = 0; m < n_mats; m++) {
    opens[m] = OpenMat{nullptr, widths[m], nullptr};                       // (the record sizes read the widths only)
    e.np_of[m] = (uint32_t)__builtin_popcount(masks[m]);
    e.n_part[m] = (size_t)e.np_of[m] * e.p.n_blocks[m] * 8 * e.n_chunks;
    want_part += arena_al(16 * e.n_part[m]) + arena_al(16 * (size_t)e.np_of[m] * widths[m]);
  }
  e.n_gpow = (size_t)n_points * e.p.total_blocks * 8;
  // the arena: the FRI part with n_mats record buffers, ONE inverse table, ONE weights table, the gamma table, per matrix its partial sums and evaluations
  e.arena_bytes = lowdeg_fri_bytes(log_M, open_rec_words(log_M, opens, n_mats), n_mats, e.ks, num_queries) + arena_al(16 * e.n_gpow) + want_part + arena_al(16 * n_points * N) +
                  arena_al(16 * n_points * M);
  return ZKIR_OK;
}

// The proof itself, in the context's arena FROM ITS CURRENT OFFSET: the caller holds c->mu and has made room for e.arena_bytes above whatever it keeps there (the locked
// entry below: the whole arena, emptied; zkir_prove_rate: above its matrices and trees).  The pinned staging is emptied: a caller keeps nothing there across the call.
// stage_ms (measurements; may be null): weights | evaluations | quotient | FRI commit phase | grinding | query section
int eval_prove_body(const EvalEntry& en, const EvalPlan& e, const zkir_stark_ctx* c, uint32_t n_mats, const uint32_t* const* mats, const uint32_t* widths, const uint32_t* const* trees,
                    const uint32_t* masks, const uint32_t* points, uint32_t n_points, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t* n_words, float* stage_ms,
                    hipStream_t s) {
  const uint32_t log_n = c->log_n, b = c->log_blowup, log_M = log_n + b;
  const uint64_t N = 1ull << log_n, M = 1ull << log_M, total = e.total;
  const std::vector<int>& ks = e.ks;
  const BatchPlan& p = e.p;
  const EvalPoints& pts = e.pts;
  const uint32_t* np_of = e.np_of;
  const size_t* n_part = e.n_part;
  const size_t n_gpow = e.n_gpow;
  OpenMat opens[BATCH_MAX_MATS];
  for (uint32_t m = 0; m < n_mats; m++) opens[m] = OpenMat{mats[m], widths[m], trees[m]};
  if (c->arena_off + e.arena_bytes > c->arena_size) { zkir::set_last_error({ZKIR_ERR_OTHER, std::string(en.who) + ": the workspace has no room for the evaluation proof"}); return ZKIR_ERR_OTHER; }
  ProofRun r(c, s, en.who, stage_ms != nullptr);
  if (stage_ms) HIP_OK(r.se.create());
  E4 *dGpow, *dWts, *dDinv, *dPart[BATCH_MAX_MATS], *dY[BATCH_MAX_MATS]; uint32_t* cw;
  HIP_OK(r.ar.take(&dGpow, n_gpow)); HIP_OK(r.ar.take(&dWts, (size_t)n_points * N)); HIP_OK(r.ar.take(&dDinv, (size_t)n_points * M));
  for (uint32_t m = 0; m < n_mats; m++) { HIP_OK(r.ar.take(&dPart[m], n_part[m])); HIP_OK(r.ar.take(&dY[m], (size_t)np_of[m] * widths[m])); }
  HIP_OK(r.ar.take(&cw, 4 * M));

  // ---- 0. weights (once for the batch) and evaluations (per matrix, at its points only); the transcript up to gamma: header, roots, points, evaluations -------------------------
  std::vector<uint32_t> head = {en.zkev ? EVAL_MAGIC : BATCH_MAGIC, EVAL_VERSION, log_n, b, en.zkev ? widths[0] : n_mats, n_points, num_queries, pow_bits, (uint32_t)ks.size()};
  if (!en.zkev) for (uint32_t m = 0; m < n_mats; m++) { head.push_back(widths[m]); head.push_back(masks[m]); }
  const size_t at_roots = head.size(), at_points = at_roots + 4 * (size_t)n_mats, at_evals = at_points + 4 * (size_t)n_points;
  head.resize(at_evals + 4 * (size_t)p.n_evals);
  memcpy(&head[at_points], points, 16 * (size_t)n_points);
  for (uint32_t m = 0; m < n_mats; m++) HIP_OK(r.d2h(&head[at_roots + 4 * m], trees[m] + 4 * (2 * M - 2), 16));
  r.mark(0);
  eval_launch_weights(c, n_points, pts, dWts, dDinv, s);
  r.mark(1);
  const EvalScales sc = eval_scales(pts, n_points, log_n);
  for (uint32_t m = 0; m < n_mats; m++) {
    // the weight rows and scales of exactly the points the matrix is opened at: mask 1 -> point 0, mask 2 -> point 1 (NP = 1 each), mask 3 -> both
    const uint32_t i0 = masks[m] == 2 ? 1 : 0;
    EvalScales scm{};
    scm.s_m[0] = sc.s_m[i0]; scm.s_m[1] = sc.s_m[1];
    eval_launch_dot(c, mats[m], widths[m], np_of[m], dWts + (size_t)i0 * N, dPart[m], scm, dY[m], s);
    // a matrix's rows of two points that are adjacent in the exponent order (always so for one matrix) come down in one copy
    const uint32_t run = np_of[m] == 2 && p.first_e[1][m] == p.first_e[0][m] + widths[m] ? 2 : 1;
    for (uint32_t li = 0; li < np_of[m]; li += run)
      HIP_OK(r.d2h(&head[at_evals + 4 * (size_t)p.first_e[i0 + li][m]], dY[m] + (size_t)li * widths[m], 16 * (size_t)run * widths[m]));
  }
  r.mark(2);
  HIP_OK(r.sync_d2h());
  if (check_launch(r.who) != ZKIR_OK) return ZKIR_ERR_DEVICE;
  Challenger ch(c->consts);
  ch.observe_n(head.data(), head.size());
  const E4 gamma = ch.sample_ext();

  // ---- 1. the codeword, one pass over all the matrices ----------------------------------------------------------------------------------------------------------------------------
  {
    const std::vector<E4> gp = batch_gamma_table(gamma, p);
    HIP_OK(r.h2d(dGpow, gp.data(), gp.size() * sizeof(E4)));
    eval_launch_quotient(c, p, mats, dGpow, dDinv, batch_claims(gp, &head[at_evals], p), cw, s);
  }
  r.mark(3);

  // ---- 2 - 4: the low-degree proof's, over this codeword, opening every matrix at the one set of query rows ----------------------------------------------------------------------
  if (const int rc = lowdeg_fri_and_queries(r, ch, head, opens, n_mats, num_queries, pow_bits, ks, cw, total, 4, proof_host)) return rc;
  if (stage_ms) r.times(stage_ms, 6);
  *n_words = total;
  return ZKIR_OK;
}

// the locked entry: every argument is checked before anything is launched; one proof at a time per context, in its workspace arena, as in zkir_prove
int eval_prove_impl(const EvalEntry& en, zkir_stark_ctx* c, uint32_t n_mats, const uint32_t* const* mats, const uint32_t* widths, const uint32_t* const* trees, const uint32_t* masks,
                    const uint32_t* points, uint32_t n_points, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words, float* stage_ms,
                    hipStream_t s) {
  auto bad = [&](const std::string& why) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, std::string(en.who) + ": " + why}); return (int)ZKIR_ERR_ARGUMENT; };
  if (n_words) *n_words = 0;
  if (!c || !mats || !widths || !trees || !masks || !points || !proof_host || !n_words) return bad("null context, matrices, widths, trees, masks, points, proof buffer or n_words");
  if (n_mats < 1 || n_mats > BATCH_MAX_MATS) return bad("n_mats must be 1 .. 4");
  for (uint32_t m = 0; m < n_mats; m++) if (!mats[m] || !trees[m]) return bad("null matrix or tree");
  EvalPlan e;
  if (const int rc = eval_plan(en, c, n_mats, widths, masks, points, n_points, num_queries, pow_bits, cap_words, &e)) return rc;
  std::lock_guard<std::mutex> ctx_lock(c->mu);
  if (const int rc = arena_reserve(c, e.arena_bytes)) return rc;
  return eval_prove_body(en, e, c, n_mats, mats, widths, trees, masks, points, n_points, num_queries, pow_bits, proof_host, n_words, stage_ms, s);
}

// zkir_prove_rate's two calls (stark_prove.inl declares them): the 'ZKBE' proof of the prover's three matrices at two points, inside the prover's lock and above its allocations
int rate_eval_plan(const zkir_stark_ctx* c, const uint32_t* widths, const uint32_t* masks, const uint32_t* points, uint32_t num_queries, uint32_t pow_bits, size_t* arena_bytes,
                   uint64_t* total_words) {
  EvalPlan e;
  if (const int rc = eval_plan(ENTRY_RATE, c, 3, widths, masks, points, 2, num_queries, pow_bits, ~0ull, &e)) return rc;
  *arena_bytes = e.arena_bytes; *total_words = e.total;
  return ZKIR_OK;
}
int rate_eval_prove(const zkir_stark_ctx* c, const uint32_t* const* mats, const uint32_t* widths, const uint32_t* const* trees, const uint32_t* masks, const uint32_t* points,
                    uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t* n_words, float* stage_ms, hipStream_t s) {
  EvalPlan e;
  if (const int rc = eval_plan(ENTRY_RATE, c, 3, widths, masks, points, 2, num_queries, pow_bits, ~0ull, &e)) return rc;
  return eval_prove_body(ENTRY_RATE, e, c, 3, mats, widths, trees, masks, points, 2, num_queries, pow_bits, proof_host, n_words, stage_ms, s);
}

// the one-matrix entries' mask: every point (a bad n_points is refused by the points check, before any mask is looked at)
inline uint32_t eval_full_mask(uint32_t n_points) { return n_points <= EVAL_MAX_POINTS ? (1u << n_points) - 1 : 0; }

// the body of the two codeword entries (who: the entry's name, in front of its error messages)
int eval_quotient_impl(const char* who, const zkir_stark_ctx* c, uint32_t n_mats, const uint32_t* const* mats, const uint32_t* widths, const uint32_t* masks, const uint32_t gamma[4],
                       const uint32_t* points, uint32_t n_points, const uint32_t* evals, uint32_t* scratch, uint32_t* cw, hipStream_t s) {
  EvalPoints pts;
  BatchPlan p;
  const char* why = !c || !mats || !widths || !masks || !gamma || !points || !evals || !scratch || !cw ? "null argument" : eval_points_check(points, n_points, &pts);
  if (!why) why = batch_plan(n_mats, widths, masks, n_points, &p);
  if (!why) for (uint32_t m = 0; m < n_mats; m++) if (!mats[m]) why = "null matrix";
  if (!why) for (int t = 0; t < 4; t++) if (gamma[t] >= bb::P) why = "gamma must be canonical";
  if (!why) for (size_t t = 0; t < 4 * (size_t)p.n_evals; t++) if (evals[t] >= bb::P) { why = "evals must be canonical"; break; }
  if (why) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, std::string(who) + ": " + why}); return ZKIR_ERR_ARGUMENT; }
  const std::vector<E4> gp = batch_gamma_table(E4{{gamma[0], gamma[1], gamma[2], gamma[3]}}, p);
  E4* dinv = reinterpret_cast<E4*>(scratch);
  E4* gpow = dinv + ((size_t)n_points << (c->log_n + c->log_blowup));
  HIP_OK(hipMemcpy(gpow, gp.data(), gp.size() * sizeof(E4), hipMemcpyHostToDevice));
  eval_launch_weights(c, n_points, pts, nullptr, dinv, s);
  eval_launch_quotient(c, p, mats, gpow, dinv, batch_claims(gp, evals, p), cw, s);
  return check_launch(who);
}

}  // namespace

extern "C" {

int zkir_batch_eval_prove(zkir_stark_ctx* c, uint32_t n_mats, const uint32_t* const* lde_mats, const uint32_t* widths, const uint32_t* const* trees, const uint32_t* masks,
                          const uint32_t* points, uint32_t n_points, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words, void* stream) {
  return eval_prove_impl(ENTRY_BATCH, c, n_mats, lde_mats, widths, trees, masks, points, n_points, num_queries, pow_bits, proof_host, cap_words, n_words, nullptr, (hipStream_t)stream);
}

// (zkir_amd_experimental.h) the same proof with the device time of its six stages: weights | evaluations | quotient | FRI commit phase | grinding | query section
int zkir_batch_eval_prove_stages(zkir_stark_ctx* c, uint32_t n_mats, const uint32_t* const* lde_mats, const uint32_t* widths, const uint32_t* const* trees, const uint32_t* masks,
                                 const uint32_t* points, uint32_t n_points, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words,
                                 float stage_ms[6], void* stream) {
  return eval_prove_impl(ENTRY_BATCH, c, n_mats, lde_mats, widths, trees, masks, points, n_points, num_queries, pow_bits, proof_host, cap_words, n_words, stage_ms, (hipStream_t)stream);
}

// the batch of one matrix opened at every point, under the 'ZKEV' header
int zkir_eval_prove(zkir_stark_ctx* c, const uint32_t* lde_mat, uint32_t width, const uint32_t* tree, const uint32_t* points, uint32_t n_points, uint32_t num_queries, uint32_t pow_bits,
                    uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words, void* stream) {
  const uint32_t mask = eval_full_mask(n_points);
  return eval_prove_impl(ENTRY_EVAL, c, 1, &lde_mat, &width, &tree, &mask, points, n_points, num_queries, pow_bits, proof_host, cap_words, n_words, nullptr, (hipStream_t)stream);
}

// (zkir_amd_experimental.h) .. with the device time of its six stages
int zkir_eval_prove_stages(zkir_stark_ctx* c, const uint32_t* lde_mat, uint32_t width, const uint32_t* tree, const uint32_t* points, uint32_t n_points, uint32_t num_queries,
                           uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words, float stage_ms[6], void* stream) {
  const uint32_t mask = eval_full_mask(n_points);
  return eval_prove_impl(ENTRY_EVAL, c, 1, &lde_mat, &width, &tree, &mask, points, n_points, num_queries, pow_bits, proof_host, cap_words, n_words, stage_ms, (hipStream_t)stream);
}

uint64_t zkir_eval_at_scratch_words(uint32_t log_n, uint32_t width, uint32_t n_points) {
  return 4 * (uint64_t)n_points * ((1ull << log_n) + 8 * (uint64_t)((width + 7) / 8) * eval_chunks(1ull << log_n));
}

// (zkir_amd_experimental.h) the evaluations alone for GIVEN points: evals = n_points x width canonical E4 (DEVICE), point-major.  Asynchronous on the stream.
int zkir_eval_at_launch(const zkir_stark_ctx* c, const uint32_t* lde_mat, uint32_t width, const uint32_t* points, uint32_t n_points, uint32_t* scratch, uint32_t* evals, void* stream) {
  EvalPoints pts;
  const char* why = !c || !lde_mat || !points || !scratch || !evals ? "null argument" : width < 1 || width > LOWDEG_MAX_WIDTH ? "width outside 1 .. 512" : eval_points_check(points, n_points, &pts);
  if (why) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, std::string("zkir_eval_at_launch: ") + why}); return ZKIR_ERR_ARGUMENT; }
  E4* wts = reinterpret_cast<E4*>(scratch);
  E4* partial = wts + ((size_t)n_points << c->log_n);
  eval_launch_weights(c, n_points, pts, wts, nullptr, (hipStream_t)stream);
  eval_launch_dot(c, lde_mat, width, n_points, wts, partial, eval_scales(pts, n_points, c->log_n), reinterpret_cast<E4*>(evals), (hipStream_t)stream);
  return check_launch("eval_at");
}

uint64_t zkir_batch_eval_quotient_scratch_words(uint32_t log_m, uint32_t n_mats, const uint32_t* widths, uint32_t n_points) {
  uint64_t blocks = 0;
  for (uint32_t m = 0; widths && m < n_mats && m < BATCH_MAX_MATS; m++) blocks += (widths[m] + 7) / 8;
  return 4 * (uint64_t)n_points * ((1ull << log_m) + 8 * blocks);
}
uint64_t zkir_eval_quotient_scratch_words(uint32_t log_m, uint32_t width, uint32_t n_points) { return zkir_batch_eval_quotient_scratch_words(log_m, 1, &width, n_points); }

// (zkir_amd_experimental.h) the codeword alone for GIVEN gamma, points and evaluations (HOST pointers, canonical; evals in the exponent order): cw[t M + j] = coordinate t of
// F(x_j).  The gamma table is uploaded with a synchronous copy: a test and measurement entry, not a stage of a pipeline.
int zkir_batch_eval_quotient_launch(const zkir_stark_ctx* c, uint32_t n_mats, const uint32_t* const* lde_mats, const uint32_t* widths, const uint32_t* masks, const uint32_t gamma[4],
                                    const uint32_t* points, uint32_t n_points, const uint32_t* evals, uint32_t* scratch, uint32_t* cw, void* stream) {
  return eval_quotient_impl("zkir_batch_eval_quotient_launch", c, n_mats, lde_mats, widths, masks, gamma, points, n_points, evals, scratch, cw, (hipStream_t)stream);
}
// .. of one matrix opened at every point (evals point-major)
int zkir_eval_quotient_launch(const zkir_stark_ctx* c, const uint32_t* lde_mat, uint32_t width, const uint32_t gamma[4], const uint32_t* points, uint32_t n_points, const uint32_t* evals,
                              uint32_t* scratch, uint32_t* cw, void* stream) {
  const uint32_t mask = eval_full_mask(n_points);
  return eval_quotient_impl("zkir_eval_quotient_launch", c, 1, &lde_mat, &width, &mask, gamma, points, n_points, evals, scratch, cw, (hipStream_t)stream);
}

}  // extern "C"
