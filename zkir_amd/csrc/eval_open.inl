// eval_open.inl — zkir_eval_prove (include/zkir_amd.h): AN EVALUATION PROOF OF A COMMITMENT at any rate the context serves (log_blowup 1, 2, 3).  Included by stark.hip at file
// scope after lowdeg.inl, whose sections 2 - 4 (FRI commit phase, grinding, queries: lowdeg_fri_and_queries) it runs unchanged over its own codeword.
//
// Statement: the B8 matrix under `tree` (zkir_lde_launch's output: canonical words over 31 <w_M>, M = N << b; zkir_merkle_commit_launch's tree) has every column k close to a
// polynomial p_k of degree < N, and p_k(z_i) = y[i][k] at n_points (1 or 2) caller-chosen points z_i of E4 outside the base field.  The evaluations are the barycentric sums
// over the rows j 2^b (the sub-coset 31 <w_N>), whatever the matrix holds; the codeword is F(x_j) = sum_i (a_i - A_i(x_j)) / (z_i - x_j) over all M rows.  Format, transcript
// and verifier: verify.cpp (zkir_eval_verify) and DESIGN.md; spec of every word: tests/eval_ref.py.
//
// THE INVERSES ARE TABLED, NOT RECOMPUTED: eval_weights_kernel writes 1 / (z_i - x_j) for all M rows once (16 n_points bytes a row), and eval_quotient_kernel reads them back.
// An E4 inversion is ~60 dependent Montgomery products (the base-field power p - 2) — about what the quotient kernel spends on 150 columns of one point — so recomputing it
// per row would put the one HBM-bound pass of the proof at its ALU limit; the table adds 32 n_points bytes of traffic to a row that reads 32 ceil(width / 8) (5 - 10 % at
// 152 columns).  The table is the proof's largest workspace next to the codeword: 16 n_points M bytes.
namespace {

constexpr uint32_t EVAL_MAGIC = 0x56454B5Au, EVAL_VERSION = 1;   // 'ZKEV'
constexpr uint32_t EVAL_MAX_POINTS = 2;
// eval_quotient_kernel: each of its 96-bit sums takes one product gamma^(i width + k)[t] * v per column, as lowdeg_combine_kernel's do
static_assert(bb::P < (1u << 31) && LOWDEG_MAX_WIDTH / 4 <= (1u << 9), "eval_quotient_kernel: a 96-bit sum's top word stays below 2^9");

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

// ---- host side -------------------------------------------------------------------------------------------------------------------------------------------------------------------
// R gamma^(i width + k) at [(i n_blocks + blk) 8 + u], k = 8 blk + u < width, zero for the rest of a ragged last block
std::vector<E4> eval_gamma_table(const E4& gamma, uint32_t width, uint32_t n_points) {
  const uint32_t n_blocks = (width + 7) / 8;
  std::vector<E4> t((size_t)n_points * n_blocks * 8, bb::e_zero());
  const E4 gamma_m = bb::e_to_mont(gamma);
  E4 g = bb::e_one_m();
  for (uint32_t i = 0; i < n_points; i++) for (uint32_t k = 0; k < width; k++) { t[(size_t)i * n_blocks * 8 + k] = g; g = bb::e_mul_m(g, gamma_m); }
  return t;
}
// a_i = sum_k gamma^(i width + k) y[i][k], canonical (y: canonical words [n_points][width][4]; gp: eval_gamma_table's)
EvalClaims eval_claims(const std::vector<E4>& gp, const uint32_t* y, uint32_t width, uint32_t n_points) {
  const uint32_t n_blocks = (width + 7) / 8;
  EvalClaims cl{};
  for (uint32_t i = 0; i < n_points; i++) {
    E4 a = bb::e_zero();                                       // Montgomery power x canonical value = canonical
    for (uint32_t k = 0; k < width; k++) { const uint32_t* v = y + 4 * ((size_t)i * width + k); a = bb::e_add(a, bb::e_mul_m(gp[(size_t)i * n_blocks * 8 + k], E4{{v[0], v[1], v[2], v[3]}})); }
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
void eval_launch_quotient(const zkir_stark_ctx* c, const uint32_t* mat, uint32_t width, uint32_t n_points, const E4* gpow, const E4* dinv, const EvalClaims& cl, uint32_t* cw, hipStream_t s) {
  const uint64_t M = 1ull << (c->log_n + c->log_blowup);
  if (n_points == 1) hipLaunchKernelGGL(eval_quotient_kernel<1>, dim3(grid_for(M)), dim3(NT), 0, s, mat, (width + 7) / 8, M, gpow, dinv, cl, cw);
  else hipLaunchKernelGGL(eval_quotient_kernel<2>, dim3(grid_for(M)), dim3(NT), 0, s, mat, (width + 7) / 8, M, gpow, dinv, cl, cw);
}
void eval_launch_weights(const zkir_stark_ctx* c, uint32_t n_points, const EvalPoints& pts, E4* wts, E4* dinv, hipStream_t s) {
  const uint32_t log_M = c->log_n + c->log_blowup;
  hipLaunchKernelGGL(eval_weights_kernel, dim3(grid_for((uint64_t)n_points << log_M)), dim3(NT), 0, s, log_M, c->log_blowup, n_points, c->d_tw_fwd, pts, wts, dinv);
}

int eval_bad(const std::string& why) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_eval_prove: " + why}); return ZKIR_ERR_ARGUMENT; }

// stage_ms (measurements; may be null): weights | evaluations | quotient | FRI commit phase | grinding | query section
int eval_prove_impl(zkir_stark_ctx* c, const uint32_t* mat, uint32_t width, const uint32_t* tree, const uint32_t* points, uint32_t n_points, uint32_t num_queries, uint32_t pow_bits,
                    uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words, float* stage_ms, hipStream_t s) {
  // every argument is checked before anything is launched
  if (n_words) *n_words = 0;
  if (!c || !mat || !tree || !points || !proof_host || !n_words) return eval_bad("null context, matrix, tree, points, proof buffer or n_words");
  const uint32_t log_n = c->log_n, b = c->log_blowup, log_M = log_n + b;
  if (log_n < 3) return eval_bad("the context's log_n must be at least 3: below that there is no layer to commit");
  if (width < 1 || width > LOWDEG_MAX_WIDTH) return eval_bad("width must be 1 .. 512 (terms per 96-bit sum of the combination)");
  EvalPoints pts;
  if (const char* why = eval_points_check(points, n_points, &pts)) return eval_bad(why);
  if (num_queries < 1 || num_queries > 128) return eval_bad("num_queries must be 1 .. 128");
  if (pow_bits > 24) return eval_bad("pow_bits must be 0 .. 24");
  const uint64_t total = zkir_eval_proof_words(log_n, b, width, n_points, num_queries);
  if (total == 0) return eval_bad("the context's log_n / log_blowup are outside what a proof can state (log_n 3 .. 26, log_blowup 1 .. 3, their sum at most 27)");
  if (cap_words < total) return eval_bad("cap_words is below zkir_eval_proof_words(log_n, log_blowup, width, n_points, num_queries)");

  std::lock_guard<std::mutex> ctx_lock(c->mu);                   // one proof at a time per context: the workspace is its arena, as in zkir_prove
  const uint64_t N = 1ull << log_n, M = 1ull << log_M;
  const std::vector<int> ks = lowdeg_schedule((int)log_n, (int)b);
  const uint32_t n_blocks = (width + 7) / 8, n_chunks = eval_chunks(N);
  const size_t n_gpow = (size_t)n_points * n_blocks * 8, n_part = n_gpow * n_chunks, n_y = (size_t)n_points * width;
  if (const int rc = arena_reserve(c, lowdeg_fri_bytes(log_M, width + 4 * (uint64_t)log_M, 1, ks, num_queries) + arena_al(16 * n_gpow) + arena_al(16 * n_part) + arena_al(16 * n_y) +
                                          arena_al(16 * n_points * N) + arena_al(16 * n_points * M))) return rc;
  ProofRun r(c, s, "zkir_eval_prove", stage_ms != nullptr);
  if (stage_ms) HIP_OK(r.se.create());
  E4 *dGpow, *dPart, *dY, *dWts, *dDinv; uint32_t* cw;
  HIP_OK(r.ar.take(&dGpow, n_gpow)); HIP_OK(r.ar.take(&dPart, n_part)); HIP_OK(r.ar.take(&dY, n_y)); HIP_OK(r.ar.take(&dWts, (size_t)n_points * N));
  HIP_OK(r.ar.take(&dDinv, (size_t)n_points * M)); HIP_OK(r.ar.take(&cw, 4 * M));

  // ---- 0. weights and evaluations; the transcript up to gamma: header, root, points, evaluations ---------------------------------------------------------------------------------
  std::vector<uint32_t> head = {EVAL_MAGIC, EVAL_VERSION, log_n, b, width, n_points, num_queries, pow_bits, (uint32_t)ks.size()};
  head.resize(13 + 4 * (size_t)n_points * (1 + width));
  memcpy(&head[13], points, 16 * (size_t)n_points);
  HIP_OK(r.d2h(&head[9], tree + 4 * (2 * M - 2), 16));
  r.mark(0);
  eval_launch_weights(c, n_points, pts, dWts, dDinv, s);
  r.mark(1);
  eval_launch_dot(c, mat, width, n_points, dWts, dPart, eval_scales(pts, n_points, log_n), dY, s);
  HIP_OK(r.d2h(&head[13 + 4 * (size_t)n_points], dY, 16 * n_y));
  r.mark(2);
  HIP_OK(r.sync_d2h());
  if (check_launch(r.who) != ZKIR_OK) return ZKIR_ERR_DEVICE;
  Challenger ch(c->consts);
  ch.observe_n(head.data(), head.size());
  const E4 gamma = ch.sample_ext();

  // ---- 1. the codeword --------------------------------------------------------------------------------------------------------------------------------------------------------
  {
    const std::vector<E4> gp = eval_gamma_table(gamma, width, n_points);
    HIP_OK(r.h2d(dGpow, gp.data(), gp.size() * sizeof(E4)));
    eval_launch_quotient(c, mat, width, n_points, dGpow, dDinv, eval_claims(gp, &head[13 + 4 * (size_t)n_points], width, n_points), cw, s);
  }
  r.mark(3);

  // ---- 2 - 4: the low-degree proof's, over this codeword --------------------------------------------------------------------------------------------------------------------------
  const OpenMat open{mat, width, tree};
  if (const int rc = lowdeg_fri_and_queries(r, ch, head, &open, 1, num_queries, pow_bits, ks, cw, total, 4, proof_host)) return rc;
  if (stage_ms) r.times(stage_ms, 6);
  *n_words = total;
  return ZKIR_OK;
}

}  // namespace

extern "C" {

int zkir_eval_prove(zkir_stark_ctx* c, const uint32_t* lde_mat, uint32_t width, const uint32_t* tree, const uint32_t* points, uint32_t n_points, uint32_t num_queries, uint32_t pow_bits,
                    uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words, void* stream) {
  return eval_prove_impl(c, lde_mat, width, tree, points, n_points, num_queries, pow_bits, proof_host, cap_words, n_words, nullptr, (hipStream_t)stream);
}

// (zkir_amd_experimental.h) the same proof with the device time of its six stages: weights | evaluations | quotient | FRI commit phase | grinding | query section
int zkir_eval_prove_stages(zkir_stark_ctx* c, const uint32_t* lde_mat, uint32_t width, const uint32_t* tree, const uint32_t* points, uint32_t n_points, uint32_t num_queries,
                           uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words, float stage_ms[6], void* stream) {
  return eval_prove_impl(c, lde_mat, width, tree, points, n_points, num_queries, pow_bits, proof_host, cap_words, n_words, stage_ms, (hipStream_t)stream);
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

uint64_t zkir_eval_quotient_scratch_words(uint32_t log_m, uint32_t width, uint32_t n_points) {
  return 4 * (uint64_t)n_points * ((1ull << log_m) + 8 * (uint64_t)((width + 7) / 8));
}

// (zkir_amd_experimental.h) the codeword alone for GIVEN gamma, points and evaluations (HOST pointers, canonical): cw[t M + j] = coordinate t of F(x_j).  The gamma table
// is uploaded with a synchronous copy: a test and measurement entry, not a stage of a pipeline.
int zkir_eval_quotient_launch(const zkir_stark_ctx* c, const uint32_t* lde_mat, uint32_t width, const uint32_t gamma[4], const uint32_t* points, uint32_t n_points, const uint32_t* evals,
                              uint32_t* scratch, uint32_t* cw, void* stream) {
  EvalPoints pts;
  const char* why = !c || !lde_mat || !gamma || !points || !evals || !scratch || !cw ? "null argument" : width < 1 || width > LOWDEG_MAX_WIDTH ? "width outside 1 .. 512" : eval_points_check(points, n_points, &pts);
  if (!why) for (int t = 0; t < 4; t++) if (gamma[t] >= bb::P) why = "gamma must be canonical";
  if (!why) for (size_t t = 0; t < 4 * (size_t)n_points * width; t++) if (evals[t] >= bb::P) { why = "evals must be canonical"; break; }
  if (why) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, std::string("zkir_eval_quotient_launch: ") + why}); return ZKIR_ERR_ARGUMENT; }
  const std::vector<E4> gp = eval_gamma_table(E4{{gamma[0], gamma[1], gamma[2], gamma[3]}}, width, n_points);
  E4* dinv = reinterpret_cast<E4*>(scratch);
  E4* gpow = dinv + ((size_t)n_points << (c->log_n + c->log_blowup));
  HIP_OK(hipMemcpy(gpow, gp.data(), gp.size() * sizeof(E4), hipMemcpyHostToDevice));
  eval_launch_weights(c, n_points, pts, nullptr, dinv, (hipStream_t)stream);
  eval_launch_quotient(c, lde_mat, width, n_points, gpow, dinv, eval_claims(gp, evals, width, n_points), cw, (hipStream_t)stream);
  return check_launch("eval_quotient");
}

}  // extern "C"
