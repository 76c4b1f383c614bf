// lowdeg.inl — zkir_lowdeg_prove (include/zkir_amd.h): a LOW-DEGREE PROOF OF A COMMITMENT at any rate the context serves (log_blowup 1, 2, 3).  Included by stark.hip at file
// scope after fri.inl (the FRI prover it shares with zkir_prove: commit phase, grinding, a query's layer jobs) and merkle_open.inl, whose opening kernel it launches unchanged.
//
// Statement: the B8 matrix under `tree` (zkir_lde_launch's output: canonical words over 31 <w_M>, M = N << b; zkir_merkle_commit_launch's tree) has every column close to a
// polynomial of degree < N.  Proof: batched FRI over C(x) = sum_k gamma^k col_k(x), gamma in E4 drawn after the root — no DEEP point, no quotient, no constraint.  Format,
// transcript and verifier: verify.cpp (zkir_lowdeg_verify) and DESIGN.md; spec of every word: tests/lowdeg_ref.py.
//
// The one HBM-bound pass is lowdeg_combine_kernel (4 * 8 * ceil(width / 8) B read and 16 B written per row); everything after it is fri.inl's FRI with log_M = log_n + b.
namespace {

constexpr uint32_t LOWDEG_MAGIC = 0x444C4B5Au, LOWDEG_VERSION = 1;   // 'ZKLD'
// Each of the four 96-bit sums of a row takes one product gamma^k[t] * v per column, both below p < 2^31: `width` terms stay below width * 2^62, so the sum's top word
// stays below width / 4.  bb::acc96_div_R asks for a top word below 2^9: 2^9 terms (deep_kernel's static_assert) are a quarter of what the bound admits.
constexpr uint32_t LOWDEG_MAX_WIDTH = 512;
static_assert(bb::P < (1u << 31) && LOWDEG_MAX_WIDTH / 4 <= (1u << 9), "lowdeg_combine_kernel: a 96-bit sum's top word stays below 2^9");

// ---- C(x_j) = sum_k gamma^k col_k(x_j), one lane per row ------------------------------------------------------------------------------------------------------------------
// The loads are deep_kernel's: the two 16-byte halves of (block, row), M4[(blk M + j) 2 + {0, 1}] — 64-bit offsets throughout (block 18 of 2^27 rows starts past 2^32 words);
// the next block's pair is requested before the current one is multiplied in.  The words are CANONICAL (zkir_lde_launch), the gamma powers Montgomery (gpow: R gamma^k,
// 8 * n_blocks entries, the columns a ragged last block does not have carry coefficient zero; uniform reads, scalar registers): each coordinate is an exact 96-bit sum
// (bb::mad96_s) reduced once, and the reduction's division by R leaves the canonical coordinate.  Written column-wise, cw[t M + j]: what the fold and leaf-hash kernels read.
__global__ __launch_bounds__(NT, DEEP_WAVES) void lowdeg_combine_kernel(const uint32_t* __restrict__ mat, uint32_t n_blocks, uint64_t M, const E4* __restrict__ gpow, uint32_t* __restrict__ cw) {
  const uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (j >= M) return;
  const uint4* __restrict__ M4 = reinterpret_cast<const uint4*>(mat);
  bb::Acc96 A[4];
#pragma unroll
  for (int t = 0; t < 4; t++) A[t] = bb::acc96_zero();
  uint4 nlo = M4[j * 2], nhi = M4[j * 2 + 1];
#pragma unroll 1
  for (uint32_t blk = 0; blk < n_blocks; blk++) {
    const uint4 vlo = nlo, vhi = nhi;
    if (blk + 1 < n_blocks) { nlo = M4[((uint64_t)(blk + 1) * M + j) * 2]; nhi = M4[((uint64_t)(blk + 1) * M + j) * 2 + 1]; }
    const uint32_t v[8] = {vlo.x, vlo.y, vlo.z, vlo.w, vhi.x, vhi.y, vhi.z, vhi.w};
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const E4 g = gpow[8 * blk + u];
#pragma unroll
      for (int t = 0; t < 4; t++) bb::mad96_s(A[t], g.c[t], v[u]);
    }
  }
#pragma unroll
  for (int t = 0; t < 4; t++) cw[(uint64_t)t * M + j] = bb::acc96_div_R(A[t]);
}

// R gamma^k for k < width, zero up to the next multiple of eight
std::vector<E4> lowdeg_gamma_table(const E4& gamma, uint32_t width) {
  std::vector<E4> t(8 * (size_t)((width + 7) / 8), bb::e_zero());
  const E4 gamma_m = bb::e_to_mont(gamma);
  E4 g = bb::e_one_m();
  for (uint32_t k = 0; k < width; k++) { t[k] = g; g = bb::e_mul_m(g, gamma_m); }
  return t;
}

// A matrix a proof's queries open: the B8 matrix, its real columns, its tree (DEVICE pointers).  A proof opens one (zkir_lowdeg_prove, zkir_eval_prove) or several of the
// same height (zkir_batch_eval_prove); a query carries record_m(q), record_m(q + M/2) matrix by matrix.
struct OpenMat { const uint32_t* mat; uint32_t width; const uint32_t* tree; };
constexpr uint32_t OPEN_MAX_MATS = 4;
// words of the records of ONE row across the matrices: sum of width_m + 4 log_M
uint64_t open_rec_words(uint32_t log_M, const OpenMat* mats, uint32_t n_mats) {
  uint64_t rec = 0;
  for (uint32_t m = 0; m < n_mats; m++) rec += (uint64_t)mats[m].width + 4 * (uint64_t)log_M;
  return rec;
}

// words of one query: q, two records per matrix (rec_words: open_rec_words), its FRI layers
uint64_t lowdeg_query_words(uint32_t log_M, uint64_t rec_words, const std::vector<int>& ks) { return 1 + 2 * rec_words + zkir::fri_query_words(log_M, ks); }

// workspace of everything from the codeword on: the codeword (16 M bytes), the layers and their trees (at most 48 M bytes together at the schedules of log_n >= 5), the
// query section and its inputs (one record buffer per opened matrix)
size_t lowdeg_fri_bytes(uint32_t log_M, uint64_t rec_words, uint32_t n_mats, const std::vector<int>& ks, uint32_t num_queries) {
  const uint64_t M = 1ull << log_M;
  size_t want = arena_al(16 * M) + 8 * 256 + arena_al(16 * (ks.size() + 1) * 4);
  { int lm = (int)log_M; for (int k : ks) { const uint64_t g = (1ull << lm) >> k; want += arena_al(16 * (2 * g - 1)) + arena_al(16 * g); lm -= k; } }
  size_t n_jobs = 0;
  for (int k : ks) n_jobs += ((size_t)1 << k) + 1;
  n_jobs = (n_jobs + n_mats) * num_queries;
  return want + arena_al(2 * (size_t)num_queries * 8) + arena_al(2 * (size_t)num_queries * rec_words * 4) + 256 * (size_t)n_mats + arena_al(n_jobs * sizeof(GatherJob)) +
         arena_al((size_t)num_queries * lowdeg_query_words(log_M, rec_words, ks) * 4);
}

// Matrices of ONE height 2^log_M that a proof's queries open, and at how many rows a query: per = 2 — rows q and q + 2^log_M / 2 (the codeword's own matrices) — or
// per = 1 — the row q mod 2^log_M (a lower group of mixed_eval.inl: the index the walk stands at when it reaches the layer of that size).
struct OpenGroup { uint32_t log_M; const OpenMat* mats; uint32_t n_mats; uint32_t per; };

// The query section of every proof here, for the sampled `queries` (each below 2^(log_M - 1), log_M: the codeword's): the matrix records by merkle_open_kernel from one device
// index array per group, copied next to the FRI leaves and paths by gather_kernel; one download.  A query: q, the groups' records in order (matrix by matrix, `per` records
// each), the layers.  `head` is the whole proof before the queries, qsize the words of a query; stage mark `mark` is recorded; the whole proof is written to proof_host.
int open_query_section(ProofRun& r, const std::vector<uint32_t>& queries, const OpenGroup* groups, uint32_t n_groups, uint32_t log_M, const std::vector<int>& ks,
                       const std::vector<uint32_t*>& fri_layers, const std::vector<uint32_t*>& fri_trees, uint64_t qsize, const std::vector<uint32_t>& head, int mark, uint32_t* proof_host) {
  hipStream_t s = r.s;
  Arena& ar = r.ar;
  const size_t nq = queries.size();
  std::vector<std::vector<uint32_t*>> dRec(n_groups);
  for (uint32_t h = 0; h < n_groups; h++) {
    const OpenGroup& g = groups[h];
    const uint64_t Mh = 1ull << g.log_M;
    std::vector<uint64_t> idx;
    for (uint32_t q : queries) {
      if (g.per == 2) { idx.push_back(q); idx.push_back((uint64_t)q + Mh / 2); }
      else idx.push_back(q & (Mh - 1));
    }
    uint64_t* dIdx;
    HIP_OK(ar.take(&dIdx, idx.size()));
    HIP_OK(r.h2d(dIdx, idx.data(), idx.size() * 8));
    dRec[h].resize(g.n_mats);
    for (uint32_t m = 0; m < g.n_mats; m++) {
      HIP_OK(ar.take(&dRec[h][m], idx.size() * (g.mats[m].width + 4 * (size_t)g.log_M)));
      hipLaunchKernelGGL(merkle_open_kernel, dim3(grid_for(idx.size() * OPEN_LANES)), dim3(NT), 0, s, g.mats[m].mat, g.mats[m].width, Mh, g.log_M, g.mats[m].tree, dIdx, (uint64_t)idx.size(), dRec[h][m]);
    }
  }
  std::vector<GatherJob> jobs;
  uint32_t off = 0;
  for (size_t t = 0; t < nq; t++) {
    off += 1;                                                                // the index word: written by the host below
    for (uint32_t h = 0; h < n_groups; h++)
      for (uint32_t m = 0; m < groups[h].n_mats; m++) {
        const uint32_t rec = groups[h].mats[m].width + 4 * groups[h].log_M, per = groups[h].per;
        jobs.push_back({dRec[h][m] + per * t * rec, 1, per * rec, off, 0u, 0u}); off += per * rec;
      }
    fri_query_jobs(jobs, off, queries[t], log_M, ks, fri_layers, fri_trees);
  }
  if ((uint64_t)off != qsize * nq) return r.fail(ZKIR_ERR_OTHER, "query section length");
  GatherJob* dJobs; uint32_t* dOut;
  HIP_OK(ar.take(&dJobs, jobs.size())); HIP_OK(ar.take(&dOut, (size_t)off));
  HIP_OK(r.h2d(dJobs, jobs.data(), jobs.size() * sizeof(GatherJob)));
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)jobs.size()), dim3(64), 0, s, dJobs, (uint32_t)jobs.size(), dOut);
  uint32_t* h_out = r.pin.take_n<uint32_t>((size_t)off);
  if (!h_out) return r.fail(ZKIR_ERR_DEVICE, "no pinned host memory for the query section");
  HIP_OK(hipMemcpyAsync(h_out, dOut, (size_t)off * 4, hipMemcpyDeviceToHost, s));
  r.mark(mark);
  HIP_OK(hipStreamSynchronize(s));
  if (check_launch(r.who) != ZKIR_OK) return ZKIR_ERR_DEVICE;
  for (size_t t = 0; t < nq; t++) h_out[t * qsize] = queries[t];
  memcpy(proof_host, head.data(), head.size() * 4);
  memcpy(proof_host + head.size(), h_out, (size_t)off * 4);
  return ZKIR_OK;
}

// Sections 2 - 4 of a proof over a codeword of M = 2^log_M values (cw[t M + j], canonical) under the n_mats (1 .. OPEN_MAX_MATS) matrices `mats`: the FRI commit phase,
// grinding, the queries (one merkle_open_kernel launch per matrix from the one index array; a query's gather jobs: the records matrix by matrix, then the layers).
// `ch` is the transcript as it stands once the codeword's challenge is drawn, `head` the proof words so far (the layer roots, the final layer and the nonce are appended),
// `total` the proof's length.  Stage marks first_mark .. first_mark + 2 are recorded after the three sections.  Writes the whole proof to proof_host.
int lowdeg_fri_and_queries(ProofRun& r, Challenger& ch, std::vector<uint32_t>& head, const OpenMat* mats, uint32_t n_mats, uint32_t num_queries, uint32_t pow_bits,
                           const std::vector<int>& ks, uint32_t* codeword, uint64_t total, int first_mark, uint32_t* proof_host) {
  const zkir_stark_ctx* c = r.c;
  const uint32_t log_M = c->log_n + c->log_blowup;
  if (n_mats < 1 || n_mats > OPEN_MAX_MATS) return r.fail(ZKIR_ERR_OTHER, "number of opened matrices");
  const uint64_t qsize = lowdeg_query_words(log_M, open_rec_words(log_M, mats, n_mats), ks), head_words = total - qsize * num_queries;

  // ---- 2. FRI commit phase, 3. grinding (fri.inl) ----------------------------------------------------------------------------------------------------------------------------
  std::vector<uint32_t*> fri_trees, fri_layers;
  if (const int rc = fri_commit(r, ch, ks, log_M, zkir::fri_final_size((int)c->log_blowup), codeword, fri_layers, fri_trees, head)) return rc;
  r.mark(first_mark);
  uint32_t pow_nonce;
  if (const int rc = fri_grind(r, ch, pow_bits, &pow_nonce)) return rc;
  head.push_back(pow_nonce);
  r.mark(first_mark + 1);
  if (head.size() != head_words) return r.fail(ZKIR_ERR_OTHER, "header length");

  // ---- 4. queries ----------------------------------------------------------------------------------------------------------------------------------------------------------------
  std::vector<uint32_t> queries(num_queries);
  for (auto& q : queries) q = ch.sample_bits((int)log_M - 1);
  const OpenGroup group{log_M, mats, n_mats, 2};
  return open_query_section(r, queries, &group, 1, log_M, ks, fri_layers, fri_trees, qsize, head, first_mark + 2, proof_host);
}

int lowdeg_bad(const std::string& why) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_lowdeg_prove: " + why}); return ZKIR_ERR_ARGUMENT; }

// stage_ms (measurements; may be null): combine | FRI commit phase | grinding | query section
int lowdeg_prove_impl(zkir_stark_ctx* c, const uint32_t* mat, uint32_t width, const uint32_t* tree, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words,
                      uint64_t* n_words, float* stage_ms, hipStream_t s) {
  // every argument is checked before anything is launched
  if (n_words) *n_words = 0;
  if (!c || !mat || !tree || !proof_host || !n_words) return lowdeg_bad("null context, matrix, tree, proof buffer or n_words");
  const uint32_t log_n = c->log_n, b = c->log_blowup, log_M = log_n + b;
  if (log_n < 3) return lowdeg_bad("the context's log_n must be at least 3: below that there is no layer to commit");
  if (width < 1 || width > LOWDEG_MAX_WIDTH) return lowdeg_bad("width must be 1 .. 512 (terms per 96-bit sum of the combination)");
  if (num_queries < 1 || num_queries > 128) return lowdeg_bad("num_queries must be 1 .. 128");
  if (pow_bits > 24) return lowdeg_bad("pow_bits must be 0 .. 24");
  const uint64_t total = zkir_lowdeg_proof_words(log_n, b, width, num_queries);
  if (total == 0) return lowdeg_bad("the context's log_n / log_blowup are outside what a proof can state (log_n 3 .. 26, log_blowup 1 .. 3, their sum at most 27)");
  if (cap_words < total) return lowdeg_bad("cap_words is below zkir_lowdeg_proof_words(log_n, log_blowup, width, num_queries)");

  std::lock_guard<std::mutex> ctx_lock(c->mu);                   // one proof at a time per context: the workspace is its arena, as in zkir_prove
  const uint64_t M = 1ull << log_M;
  const std::vector<int> ks = zkir::fri_schedule((int)log_n, (int)b);
  const uint32_t n_blocks = (width + 7) / 8;
  if (const int rc = arena_reserve(c, lowdeg_fri_bytes(log_M, width + 4 * (uint64_t)log_M, 1, ks, num_queries) + arena_al(n_blocks * 8 * sizeof(E4)))) return rc;
  ProofRun r(c, s, "zkir_lowdeg_prove", stage_ms != nullptr);
  if (stage_ms) HIP_OK(r.se.create());

  // ---- transcript up to gamma: header, root ------------------------------------------------------------------------------------------------------------------------------
  std::vector<uint32_t> head = {LOWDEG_MAGIC, LOWDEG_VERSION, log_n, b, width, num_queries, pow_bits, (uint32_t)ks.size()};
  uint32_t root[4];
  HIP_OK(r.d2h(root, tree + 4 * (2 * M - 2), 16));
  HIP_OK(r.sync_d2h());
  Challenger ch(c->consts);
  ch.observe_n(head.data(), 8);
  ch.observe_n(root, 4);
  const E4 gamma = ch.sample_ext();
  head.insert(head.end(), root, root + 4);

  // ---- 1. the codeword --------------------------------------------------------------------------------------------------------------------------------------------------------
  E4* dGpow; uint32_t* cw;
  HIP_OK(r.ar.take(&dGpow, (size_t)n_blocks * 8)); HIP_OK(r.ar.take(&cw, 4 * M));
  {
    const std::vector<E4> gp = lowdeg_gamma_table(gamma, width);
    HIP_OK(r.h2d(dGpow, gp.data(), gp.size() * sizeof(E4)));
  }
  r.mark(0);
  hipLaunchKernelGGL(lowdeg_combine_kernel, dim3(grid_for(M)), dim3(NT), 0, s, mat, n_blocks, M, dGpow, cw);
  r.mark(1);

  // ---- 2 - 4 ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
  const OpenMat open{mat, width, tree};
  if (const int rc = lowdeg_fri_and_queries(r, ch, head, &open, 1, num_queries, pow_bits, ks, cw, total, 2, proof_host)) return rc;
  if (stage_ms) r.times(stage_ms, 4);
  *n_words = total;
  return ZKIR_OK;
}

}  // namespace

extern "C" {

int zkir_lowdeg_prove(zkir_stark_ctx* c, const uint32_t* lde_mat, uint32_t width, const uint32_t* tree, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words,
                      uint64_t* n_words, void* stream) {
  return lowdeg_prove_impl(c, lde_mat, width, tree, num_queries, pow_bits, proof_host, cap_words, n_words, nullptr, (hipStream_t)stream);
}

// (zkir_amd_experimental.h) the same proof with the device time of its four stages: combine | FRI commit phase | grinding | query section
int zkir_lowdeg_prove_stages(zkir_stark_ctx* c, const uint32_t* lde_mat, uint32_t width, const uint32_t* tree, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words,
                             uint64_t* n_words, float stage_ms[4], void* stream) {
  return lowdeg_prove_impl(c, lde_mat, width, tree, num_queries, pow_bits, proof_host, cap_words, n_words, stage_ms, (hipStream_t)stream);
}

// (zkir_amd_experimental.h) lowdeg_combine_kernel alone for a GIVEN gamma (canonical E4): cw[t M + j] = coordinate t of sum_k gamma^k col_k(x_j), M = N << log_blowup rows.
// The gamma table is uploaded with a synchronous copy: a test and measurement entry, not a stage of a pipeline.
int zkir_lowdeg_combine_launch(const zkir_stark_ctx* c, const uint32_t* lde_mat, uint32_t width, const uint32_t gamma[4], uint32_t* gpow_scratch, uint32_t* cw, void* stream) {
  if (!c || !lde_mat || !gamma || !gpow_scratch || !cw || width < 1 || width > LOWDEG_MAX_WIDTH) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_lowdeg_combine_launch: null argument, or width outside 1 .. 512"}); return ZKIR_ERR_ARGUMENT; }
  for (int t = 0; t < 4; t++) if (gamma[t] >= bb::P) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_lowdeg_combine_launch: gamma must be canonical"}); return ZKIR_ERR_ARGUMENT; }
  const std::vector<E4> gp = lowdeg_gamma_table(E4{{gamma[0], gamma[1], gamma[2], gamma[3]}}, width);
  HIP_OK(hipMemcpy(gpow_scratch, gp.data(), gp.size() * sizeof(E4), hipMemcpyHostToDevice));
  const uint64_t M = 1ull << (c->log_n + c->log_blowup);
  hipLaunchKernelGGL(lowdeg_combine_kernel, dim3(grid_for(M)), dim3(NT), 0, (hipStream_t)stream, lde_mat, (width + 7) / 8, M, reinterpret_cast<const E4*>(gpow_scratch), cw);
  return check_launch("lowdeg_combine");
}

}  // extern "C"
