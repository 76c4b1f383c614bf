// batch_eval.inl — zkir_batch_eval_prove (include/zkir_amd.h): ONE EVALUATION PROOF FOR SEVERAL COMMITMENTS OF ONE HEIGHT, at any rate the context serves.  Included by
// stark.hip at file scope after eval_open.inl, whose weights, dot and sum kernels it launches unchanged, and lowdeg.inl, whose sections 2 - 4 (lowdeg_fri_and_queries) it
// runs over its own codeword with a list of opened matrices.
//
// Statement: n_mats (1 .. 4) B8 matrices of the context's size, each under its own tree, have every column close to a polynomial of degree < N, and matrix m's columns take
// the proof's values at those of the n_points (1 or 2) shared points z_i of E4 that mask_m selects.  The gamma exponent e runs consecutively: for i over the points, for m
// over the matrices with bit i of mask_m set, in order, for k < width_m;  A_i(x) = sum gamma^e col_{m,k}(x), a_i = sum gamma^e y[i][m][k] over the selected (m, k) of point i,
// F(x_j) = sum_i (a_i - A_i(x_j)) / (z_i - x_j) over all M rows.  Format, transcript and verifier: verify.cpp (zkir_batch_eval_verify) and DESIGN.md; spec of every word:
// tests/batch_eval_ref.py.
//
// What the batch shares: ONE inverse table and weights table (eval_weights_kernel, one E4 inversion per (point, row) whatever the number of matrices), ONE pass that writes
// the codeword (batch_quotient_kernel), one FRI commit phase, one grind, one set of query rows.  What stays per matrix: the evaluations (eval_dot_kernel with NP = the
// number of points the matrix is opened at and the weight rows of exactly those points) and the opening records.
namespace {

constexpr uint32_t BATCH_MAGIC = 0x45424B5Au, BATCH_VERSION = 1;   // 'ZKBE'
constexpr uint32_t BATCH_MAX_MATS = OPEN_MAX_MATS, BATCH_MAX_TOTAL_WIDTH = LOWDEG_MAX_WIDTH;
// batch_quotient_kernel: each of its 96-bit sums takes one product gamma^e[t] * v per column of every matrix opened at its point: at most BATCH_MAX_TOTAL_WIDTH terms, the
// bound of eval_quotient_kernel's sums
static_assert(bb::P < (1u << 31) && BATCH_MAX_TOTAL_WIDTH / 4 <= (1u << 9) && BATCH_MAX_TOTAL_WIDTH == LOWDEG_MAX_WIDTH, "batch_quotient_kernel: a 96-bit sum's top word stays below 2^9");

// the matrices as the quotient kernel takes them, by value (kernel arguments: scalar registers)
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
// R gamma^e at [(i total_blocks + first_block[m] + blk) 8 + u] for the selected (i, m), k = 8 blk + u < width_m; zero everywhere else
std::vector<E4> batch_gamma_table(const E4& gamma, const BatchPlan& p) {
  std::vector<E4> t((size_t)p.n_points * p.total_blocks * 8, bb::e_zero());
  const E4 gamma_m = bb::e_to_mont(gamma);
  E4 g = bb::e_one_m();
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
void batch_launch_quotient(const zkir_stark_ctx* c, const BatchPlan& p, const uint32_t* const* mats, const E4* gpow, const E4* dinv, const EvalClaims& cl, uint32_t* cw, hipStream_t s) {
  const uint64_t M = 1ull << (c->log_n + c->log_blowup);
  BatchMats bm{};
  for (uint32_t m = 0; m < p.n_mats; m++) { bm.mat[m] = mats[m]; bm.n_blocks[m] = p.n_blocks[m]; bm.mask[m] = p.mask[m]; }
  bm.n_mats = p.n_mats; bm.total_blocks = p.total_blocks;
  if (p.n_points == 1) hipLaunchKernelGGL(batch_quotient_kernel<1>, dim3(grid_for(M)), dim3(NT), 0, s, bm, M, gpow, dinv, cl, cw);
  else hipLaunchKernelGGL(batch_quotient_kernel<2>, dim3(grid_for(M)), dim3(NT), 0, s, bm, M, gpow, dinv, cl, cw);
}

int batch_bad(const std::string& why) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_batch_eval_prove: " + why}); return ZKIR_ERR_ARGUMENT; }

// stage_ms (measurements; may be null): weights | evaluations | quotient | FRI commit phase | grinding | query section
int batch_prove_impl(zkir_stark_ctx* c, uint32_t n_mats, const uint32_t* const* mats, const uint32_t* widths, const uint32_t* const* trees, const uint32_t* masks, const uint32_t* points,
                     uint32_t n_points, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words, float* stage_ms, hipStream_t s) {
  // every argument is checked before anything is launched
  if (n_words) *n_words = 0;
  if (!c || !mats || !widths || !trees || !masks || !points || !proof_host || !n_words) return batch_bad("null context, matrices, widths, trees, masks, points, proof buffer or n_words");
  if (n_mats < 1 || n_mats > BATCH_MAX_MATS) return batch_bad("n_mats must be 1 .. 4");
  for (uint32_t m = 0; m < n_mats; m++) if (!mats[m] || !trees[m]) return batch_bad("null matrix or tree in lde_mats / trees");
  const uint32_t log_n = c->log_n, b = c->log_blowup, log_M = log_n + b;
  if (log_n < 3) return batch_bad("the context's log_n must be at least 3: below that there is no layer to commit");
  EvalPoints pts;
  if (const char* why = eval_points_check(points, n_points, &pts)) return batch_bad(why);
  BatchPlan p;
  if (const char* why = batch_plan(n_mats, widths, masks, n_points, &p)) return batch_bad(why);
  if (num_queries < 1 || num_queries > 128) return batch_bad("num_queries must be 1 .. 128");
  if (pow_bits > 24) return batch_bad("pow_bits must be 0 .. 24");
  const uint64_t total = zkir_batch_eval_proof_words(log_n, b, n_mats, widths, masks, n_points, num_queries);
  if (total == 0) return batch_bad("the context's log_n / log_blowup are outside what a proof can state (log_n 3 .. 26, log_blowup 1 .. 3, their sum at most 27)");
  if (cap_words < total) return batch_bad("cap_words is below zkir_batch_eval_proof_words(log_n, log_blowup, n_mats, widths, masks, n_points, num_queries)");

  std::lock_guard<std::mutex> ctx_lock(c->mu);                   // one proof at a time per context: the workspace is its arena, as in zkir_prove
  const uint64_t N = 1ull << log_n, M = 1ull << log_M;
  const std::vector<int> ks = lowdeg_schedule((int)log_n, (int)b);
  const uint32_t n_chunks = eval_chunks(N);
  OpenMat opens[BATCH_MAX_MATS];
  uint32_t np_of[BATCH_MAX_MATS];
  size_t n_part[BATCH_MAX_MATS], want_part = 0;
  for (uint32_t m = 0; m < n_mats; m++) {
    opens[m] = OpenMat{mats[m], widths[m], trees[m]};
    np_of[m] = (uint32_t)__builtin_popcount(masks[m]);
    n_part[m] = (size_t)np_of[m] * p.n_blocks[m] * 8 * n_chunks;
    want_part += arena_al(16 * n_part[m]) + arena_al(16 * (size_t)np_of[m] * widths[m]);
  }
  const size_t n_gpow = (size_t)n_points * p.total_blocks * 8;
  // the arena: the FRI part with n_mats record buffers, ONE inverse table, ONE weights table, the gamma table, per matrix its partial sums and evaluations
  if (const int rc = arena_reserve(c, lowdeg_fri_bytes(log_M, open_rec_words(log_M, opens, n_mats), n_mats, ks, num_queries) + arena_al(16 * n_gpow) + want_part +
                                          arena_al(16 * n_points * N) + arena_al(16 * n_points * M))) return rc;
  ProofRun r(c, s, "zkir_batch_eval_prove", stage_ms != nullptr);
  if (stage_ms) HIP_OK(r.se.create());
  E4 *dGpow, *dWts, *dDinv, *dPart[BATCH_MAX_MATS], *dY[BATCH_MAX_MATS]; uint32_t* cw;
  HIP_OK(r.ar.take(&dGpow, n_gpow)); HIP_OK(r.ar.take(&dWts, (size_t)n_points * N)); HIP_OK(r.ar.take(&dDinv, (size_t)n_points * M));
  for (uint32_t m = 0; m < n_mats; m++) { HIP_OK(r.ar.take(&dPart[m], n_part[m])); HIP_OK(r.ar.take(&dY[m], (size_t)np_of[m] * widths[m])); }
  HIP_OK(r.ar.take(&cw, 4 * M));

  // ---- 0. weights (once for the batch) and evaluations (per matrix, at its points only); the transcript up to gamma: header, shape, roots, points, evaluations ------------------
  std::vector<uint32_t> head = {BATCH_MAGIC, BATCH_VERSION, log_n, b, n_mats, n_points, num_queries, pow_bits, (uint32_t)ks.size()};
  for (uint32_t m = 0; m < n_mats; m++) { head.push_back(widths[m]); head.push_back(masks[m]); }
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
    for (uint32_t li = 0; li < np_of[m]; li++) HIP_OK(r.d2h(&head[at_evals + 4 * (size_t)p.first_e[i0 + li][m]], dY[m] + (size_t)li * widths[m], 16 * (size_t)widths[m]));
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
    batch_launch_quotient(c, p, mats, dGpow, dDinv, batch_claims(gp, &head[at_evals], p), cw, s);
  }
  r.mark(3);

  // ---- 2 - 4: the low-degree proof's, over this codeword, opening every matrix at the one set of query rows ----------------------------------------------------------------------
  if (const int rc = lowdeg_fri_and_queries(r, ch, head, opens, n_mats, num_queries, pow_bits, ks, cw, total, 4, proof_host)) return rc;
  if (stage_ms) r.times(stage_ms, 6);
  *n_words = total;
  return ZKIR_OK;
}

}  // namespace

extern "C" {

int zkir_batch_eval_prove(zkir_stark_ctx* c, uint32_t n_mats, const uint32_t* const* lde_mats, const uint32_t* widths, const uint32_t* const* trees, const uint32_t* masks,
                          const uint32_t* points, uint32_t n_points, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words, void* stream) {
  return batch_prove_impl(c, n_mats, lde_mats, widths, trees, masks, points, n_points, num_queries, pow_bits, proof_host, cap_words, n_words, nullptr, (hipStream_t)stream);
}

// (zkir_amd_experimental.h) the same proof with the device time of its six stages: weights | evaluations | quotient | FRI commit phase | grinding | query section
int zkir_batch_eval_prove_stages(zkir_stark_ctx* c, uint32_t n_mats, const uint32_t* const* lde_mats, const uint32_t* widths, const uint32_t* const* trees, const uint32_t* masks,
                                 const uint32_t* points, uint32_t n_points, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words,
                                 float stage_ms[6], void* stream) {
  return batch_prove_impl(c, n_mats, lde_mats, widths, trees, masks, points, n_points, num_queries, pow_bits, proof_host, cap_words, n_words, stage_ms, (hipStream_t)stream);
}

uint64_t zkir_batch_eval_quotient_scratch_words(uint32_t log_m, uint32_t n_mats, const uint32_t* widths, uint32_t n_points) {
  uint64_t blocks = 0;
  for (uint32_t m = 0; widths && m < n_mats && m < BATCH_MAX_MATS; m++) blocks += (widths[m] + 7) / 8;
  return 4 * (uint64_t)n_points * ((1ull << log_m) + 8 * blocks);
}

// (zkir_amd_experimental.h) the codeword alone for GIVEN gamma, points and evaluations (HOST pointers, canonical; evals in the exponent order): cw[t M + j] = coordinate t of
// F(x_j).  The gamma table is uploaded with a synchronous copy: a test and measurement entry, not a stage of a pipeline.
int zkir_batch_eval_quotient_launch(const zkir_stark_ctx* c, uint32_t n_mats, const uint32_t* const* lde_mats, const uint32_t* widths, const uint32_t* masks, const uint32_t gamma[4],
                                    const uint32_t* points, uint32_t n_points, const uint32_t* evals, uint32_t* scratch, uint32_t* cw, void* stream) {
  EvalPoints pts;
  BatchPlan p;
  const char* why = !c || !lde_mats || !widths || !masks || !gamma || !points || !evals || !scratch || !cw ? "null argument" : eval_points_check(points, n_points, &pts);
  if (!why) why = batch_plan(n_mats, widths, masks, n_points, &p);
  if (!why) for (uint32_t m = 0; m < n_mats; m++) if (!lde_mats[m]) why = "null matrix";
  if (!why) for (int t = 0; t < 4; t++) if (gamma[t] >= bb::P) why = "gamma must be canonical";
  if (!why) for (size_t t = 0; t < 4 * (size_t)p.n_evals; t++) if (evals[t] >= bb::P) { why = "evals must be canonical"; break; }
  if (why) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, std::string("zkir_batch_eval_quotient_launch: ") + why}); return ZKIR_ERR_ARGUMENT; }
  const std::vector<E4> gp = batch_gamma_table(E4{{gamma[0], gamma[1], gamma[2], gamma[3]}}, p);
  E4* dinv = reinterpret_cast<E4*>(scratch);
  E4* gpow = dinv + ((size_t)n_points << (c->log_n + c->log_blowup));
  HIP_OK(hipMemcpy(gpow, gp.data(), gp.size() * sizeof(E4), hipMemcpyHostToDevice));
  eval_launch_weights(c, n_points, pts, nullptr, dinv, (hipStream_t)stream);
  batch_launch_quotient(c, p, lde_mats, gpow, dinv, batch_claims(gp, evals, p), cw, (hipStream_t)stream);
  return check_launch("batch_eval_quotient");
}

}  // extern "C"
