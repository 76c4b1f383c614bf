// mixed_eval.inl — zkir_mixed_eval_prove (include/zkir_amd.h): ONE EVALUATION PROOF OF COMMITMENTS OF DIFFERENT HEIGHTS at one rate (log_blowup 1, 2, 3).  Included by
// stark.hip at file scope after eval_open.inl, whose weights, evaluation and quotient launches it runs group by group, each with its group's own context, and after fri.inl,
// whose commit phase takes the lower groups' codewords as addends.
//
// Statement: n_groups (2 or 3) groups of strictly decreasing heights N_0 > N_1 > ..; group h is exactly what a 'ZKBE' proof states at its own height — 1 .. 4 B8 matrices of
// M_h = N_h << b rows, each under its own tree, widths summing to at most 512, its own 1 or 2 points of E4, a mask per matrix.  The evaluations are 'ZKBE''s barycentric sums.
// ONE gamma is drawn after the header and all roots, points and evaluations; its exponent runs consecutively through the groups in order and inside a group in 'ZKBE''s order.
// F_h is 'ZKBE''s quotient of group h over 31 <w_{M_h}> with those exponents.  Layer 0 of the one FRI is F_0; the schedule (fri_mixed_schedule) makes every M_h a committed
// layer's size, and when a fold leaves the layer of size M_h, F_h is added to it by index before it is hashed (fri_fold_k_kernel's ADD form).  As a function of that layer's
// own point F_h is still a polynomial of degree < N_h, whatever the squared shift, so the final layer has degree < 4 exactly as in a proof of one height.
//
// A query opens group 0 at rows q and q + M_0/2 and every lower group at the ONE row q mod M_h — the index the walk stands at when it reaches the layer of that size.
// Format ('ZKMH'), transcript, verifier: verify.cpp (zkir_mixed_eval_verify) and DESIGN.md; spec of every word: tests/mixed_eval_ref.py.
//
// The arena and the mutex are the FIRST group's context's; the other contexts are only read (log_n, log_blowup, d_tw_fwd).
namespace {

constexpr uint32_t MIXED_MAGIC = 0x484D4B5Au, MIXED_VERSION = 1, MIXED_MAX_GROUPS = 3;   // 'ZKMH'

// one group as the prover sees it: where its entries stand in the flat argument arrays, its shape, its device buffers
struct MixedGroup {
  const zkir_stark_ctx* c; uint32_t log_M, first_mat, first_point, n_points, first_e;
  EvalPoints pts; BatchPlan p;
  OpenMat opens[BATCH_MAX_MATS]; uint32_t np_of[BATCH_MAX_MATS]; size_t n_part[BATCH_MAX_MATS], n_gpow;
  E4 *dGpow, *dWts, *dDinv, *dPart[BATCH_MAX_MATS], *dY[BATCH_MAX_MATS]; uint32_t* cw;
};

// stage_ms (measurements; may be null): weights | evaluations | quotients | FRI commit phase | grinding | query section
int mixed_prove_impl(zkir_stark_ctx* const* ctxs, uint32_t n_groups, const uint32_t* n_mats, const uint32_t* const* mats, const uint32_t* widths, const uint32_t* const* trees,
                     const uint32_t* masks, const uint32_t* points, const uint32_t* n_points, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words,
                     uint64_t* n_words, float* stage_ms, hipStream_t s) {
  const char* who = "zkir_mixed_eval_prove";
  auto bad = [&](const std::string& why) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, std::string(who) + ": " + why}); return (int)ZKIR_ERR_ARGUMENT; };
  // every argument is checked before anything is launched
  if (n_words) *n_words = 0;
  if (!ctxs || !n_mats || !mats || !widths || !trees || !masks || !points || !n_points || !proof_host || !n_words)
    return bad("null contexts, n_mats, matrices, widths, trees, masks, points, n_points, proof buffer or n_words");
  if (n_groups < 2 || n_groups > MIXED_MAX_GROUPS) return bad("n_groups must be 2 or 3 (one group is zkir_batch_eval_prove's)");
  for (uint32_t h = 0; h < n_groups; h++) if (!ctxs[h]) return bad("null context");
  const uint32_t b = ctxs[0]->log_blowup;
  MixedGroup G[MIXED_MAX_GROUPS];
  uint32_t log_ns[MIXED_MAX_GROUPS], at_mat = 0, at_point = 0, n_evals = 0;
  for (uint32_t h = 0; h < n_groups; h++) {
    MixedGroup& g = G[h];
    g.c = ctxs[h];
    if (g.c->log_blowup != b) return bad("a context's log_blowup is not the first context's: one proof has one rate");
    if (g.c->log_n < 3) return bad("a context's log_n must be at least 3: below that there is no layer to commit");
    if (h && g.c->log_n >= ctxs[h - 1]->log_n) return bad("the contexts' heights must strictly decrease (equal heights belong in one group)");
    log_ns[h] = g.c->log_n; g.log_M = g.c->log_n + b;
    if (n_mats[h] < 1 || n_mats[h] > BATCH_MAX_MATS) return bad("a group's n_mats must be 1 .. 4");
    g.first_mat = at_mat; g.first_point = at_point; g.n_points = n_points[h]; g.first_e = n_evals;
    if (const char* why = eval_points_check(points + 4 * (size_t)at_point, g.n_points, &g.pts)) return bad(why);
    if (const char* why = batch_plan(n_mats[h], widths + at_mat, masks + at_mat, g.n_points, &g.p)) return bad(why);
    for (uint32_t m = 0; m < n_mats[h]; m++) {
      if (!mats[at_mat + m] || !trees[at_mat + m]) return bad("null matrix or tree");
      g.opens[m] = OpenMat{mats[at_mat + m], widths[at_mat + m], trees[at_mat + m]};
    }
    at_mat += n_mats[h]; at_point += g.n_points; n_evals += g.p.n_evals;
  }
  if (num_queries < 1 || num_queries > 128) return bad("num_queries must be 1 .. 128");
  if (pow_bits > 24) return bad("pow_bits must be 0 .. 24");
  const uint64_t total = zkir_mixed_eval_proof_words(b, n_groups, log_ns, n_mats, n_points, widths, masks, num_queries);
  if (total == 0) return bad("the contexts' log_n / log_blowup are outside what a proof can state (log_n 3 .. 26, log_blowup 1 .. 3, their sum at most 27)");
  if (cap_words < total) return bad("cap_words is below zkir_mixed_eval_proof_words(log_blowup, n_groups, log_ns, n_mats, n_points, widths, masks, num_queries)");

  const zkir_stark_ctx* c = ctxs[0];
  std::lock_guard<std::mutex> ctx_lock(c->mu);                   // one proof at a time on the first context: the workspace is its arena
  const uint32_t log_M = G[0].log_M;
  const std::vector<int> ks = zkir::fri_mixed_schedule(log_ns, n_groups, (int)b);
  // words of one query: q, two records per matrix of group 0, one per matrix of a lower group, the layers
  uint64_t rec_low = 0;
  for (uint32_t h = 1; h < n_groups; h++) rec_low += open_rec_words(G[h].log_M, G[h].opens, G[h].p.n_mats);
  const uint64_t rec0 = open_rec_words(log_M, G[0].opens, G[0].p.n_mats), qsize = 1 + 2 * rec0 + rec_low + zkir::fri_query_words(log_M, ks);
  // the arena: group 0's FRI part (lowdeg_fri_bytes, with the lower groups' records counted as record words and their matrices as record buffers), per lower group its
  // index array, per group what a 'ZKBE' proof of it takes (gamma table, weights, inverse table, partial sums, evaluations) and its codeword (group 0's is the FRI part's)
  size_t want = lowdeg_fri_bytes(log_M, rec0 + rec_low, at_mat, ks, num_queries) + (size_t)n_groups * (arena_al((size_t)num_queries * 8) + 256);
  for (uint32_t h = 0; h < n_groups; h++) {
    MixedGroup& g = G[h];
    const uint64_t Nh = 1ull << g.c->log_n, Mh = 1ull << g.log_M;
    const uint32_t n_chunks = eval_chunks(Nh);
    g.n_gpow = (size_t)g.n_points * g.p.total_blocks * 8;
    want += arena_al(16 * g.n_gpow) + arena_al(16 * g.n_points * Nh) + arena_al(16 * g.n_points * Mh) + (h ? arena_al(16 * Mh) : 0);
    for (uint32_t m = 0; m < g.p.n_mats; m++) {
      g.np_of[m] = (uint32_t)__builtin_popcount(g.p.mask[m]);
      g.n_part[m] = (size_t)g.np_of[m] * g.p.n_blocks[m] * 8 * n_chunks;
      want += arena_al(16 * g.n_part[m]) + arena_al(16 * (size_t)g.np_of[m] * g.p.width[m]);
    }
  }
  if (const int rc = arena_reserve(c, want)) return rc;
  ProofRun r(c, s, who, stage_ms != nullptr);
  if (stage_ms) HIP_OK(r.se.create());
  for (uint32_t h = 0; h < n_groups; h++) {
    MixedGroup& g = G[h];
    HIP_OK(r.ar.take(&g.dGpow, g.n_gpow)); HIP_OK(r.ar.take(&g.dWts, (size_t)g.n_points << g.c->log_n)); HIP_OK(r.ar.take(&g.dDinv, (size_t)g.n_points << g.log_M));
    for (uint32_t m = 0; m < g.p.n_mats; m++) { HIP_OK(r.ar.take(&g.dPart[m], g.n_part[m])); HIP_OK(r.ar.take(&g.dY[m], (size_t)g.np_of[m] * g.p.width[m])); }
    HIP_OK(r.ar.take(&g.cw, (size_t)4 << g.log_M));
  }

  // ---- 0. weights and evaluations, group by group as a 'ZKBE' proof's; the transcript up to gamma: header, group shapes, roots, points, evaluations ----------------------------
  std::vector<uint32_t> head = {MIXED_MAGIC, MIXED_VERSION, b, n_groups, num_queries, pow_bits, (uint32_t)ks.size()};
  for (uint32_t h = 0; h < n_groups; h++) {
    head.push_back(log_ns[h]); head.push_back(G[h].p.n_mats); head.push_back(G[h].n_points);
    for (uint32_t m = 0; m < G[h].p.n_mats; m++) { head.push_back(G[h].p.width[m]); head.push_back(G[h].p.mask[m]); }
  }
  const size_t at_roots = head.size(), at_points = at_roots + 4 * (size_t)at_mat, at_evals = at_points + 4 * (size_t)at_point;
  head.resize(at_evals + 4 * (size_t)n_evals);
  memcpy(&head[at_points], points, 16 * (size_t)at_point);
  for (uint32_t h = 0; h < n_groups; h++)
    for (uint32_t m = 0; m < G[h].p.n_mats; m++) HIP_OK(r.d2h(&head[at_roots + 4 * (size_t)(G[h].first_mat + m)], G[h].opens[m].tree + 4 * ((2ull << G[h].log_M) - 2), 16));
  r.mark(0);
  for (uint32_t h = 0; h < n_groups; h++) eval_launch_weights(G[h].c, G[h].n_points, G[h].pts, G[h].dWts, G[h].dDinv, s);
  r.mark(1);
  for (uint32_t h = 0; h < n_groups; h++) {
    MixedGroup& g = G[h];
    const uint64_t Nh = 1ull << g.c->log_n;
    const EvalScales sc = eval_scales(g.pts, g.n_points, g.c->log_n);
    for (uint32_t m = 0; m < g.p.n_mats; m++) {                              // (eval_prove_impl's loop: the weight rows and scales of exactly the points the matrix is opened at)
      const uint32_t i0 = g.p.mask[m] == 2 ? 1 : 0;
      EvalScales scm{};
      scm.s_m[0] = sc.s_m[i0]; scm.s_m[1] = sc.s_m[1];
      eval_launch_dot(g.c, g.opens[m].mat, g.p.width[m], g.np_of[m], g.dWts + (size_t)i0 * Nh, g.dPart[m], scm, g.dY[m], s);
      for (uint32_t li = 0; li < g.np_of[m]; li++)
        HIP_OK(r.d2h(&head[at_evals + 4 * ((size_t)g.first_e + g.p.first_e[i0 + li][m])], g.dY[m] + (size_t)li * g.p.width[m], 16 * (size_t)g.p.width[m]));
    }
  }
  r.mark(2);
  HIP_OK(r.sync_d2h());
  if (check_launch(who) != ZKIR_OK) return ZKIR_ERR_DEVICE;
  Challenger ch(c->consts);
  ch.observe_n(head.data(), head.size());
  const E4 gamma = ch.sample_ext();

  // ---- 1. the codewords: F_h over its own domain, the gamma table of group h starting at the group's first exponent -----------------------------------------------------------
  {
    const E4 gamma_m = bb::e_to_mont(gamma);
    E4 first = bb::e_one_m();
    for (uint32_t h = 0; h < n_groups; h++) {
      MixedGroup& g = G[h];
      const std::vector<E4> gp = batch_gamma_table(gamma, g.p, first);
      HIP_OK(r.h2d(g.dGpow, gp.data(), gp.size() * sizeof(E4)));
      const uint32_t* gm[BATCH_MAX_MATS];
      for (uint32_t m = 0; m < g.p.n_mats; m++) gm[m] = g.opens[m].mat;
      eval_launch_quotient(g.c, g.p, gm, g.dGpow, g.dDinv, batch_claims(gp, &head[at_evals + 4 * (size_t)g.first_e], g.p), g.cw, s);
      for (uint32_t e = 0; e < g.p.n_evals; e++) first = bb::e_mul_m(first, gamma_m);
    }
  }
  r.mark(3);

  // ---- 2. FRI commit phase with F_h added to the layer of its size, 3. grinding (fri.inl) ---------------------------------------------------------------------------------------
  std::vector<const uint32_t*> addends(ks.size(), nullptr);
  {
    int log_m = (int)log_M;
    for (size_t j = 0; j < ks.size(); j++) {
      log_m -= ks[j];
      for (uint32_t h = 1; h < n_groups; h++) if ((int)G[h].log_M == log_m) addends[j] = G[h].cw;
    }
    for (uint32_t h = 1; h < n_groups; h++) {
      bool placed = false;
      for (const uint32_t* a : addends) placed |= a == G[h].cw;
      if (!placed) return r.fail(ZKIR_ERR_OTHER, "a lower group's size is no committed layer's");
    }
  }
  std::vector<uint32_t*> fri_trees, fri_layers;
  if (const int rc = fri_commit(r, ch, ks, log_M, zkir::fri_final_size((int)b), G[0].cw, fri_layers, fri_trees, head, &addends)) return rc;
  r.mark(4);
  uint32_t pow_nonce;
  if (const int rc = fri_grind(r, ch, pow_bits, &pow_nonce)) return rc;
  head.push_back(pow_nonce);
  r.mark(5);
  const uint64_t head_words = total - qsize * num_queries;
  if (head.size() != head_words) return r.fail(ZKIR_ERR_OTHER, "header length");

  // ---- 4. queries (lowdeg.inl: open_query_section): group 0's records at q and q + M_0/2, a lower group's at q mod M_h ------------------------------------------------------------
  std::vector<uint32_t> queries(num_queries);
  for (auto& q : queries) q = ch.sample_bits((int)log_M - 1);
  OpenGroup og[MIXED_MAX_GROUPS];
  for (uint32_t h = 0; h < n_groups; h++) og[h] = OpenGroup{G[h].log_M, G[h].opens, G[h].p.n_mats, h ? 1u : 2u};
  if (const int rc = open_query_section(r, queries, og, n_groups, log_M, ks, fri_layers, fri_trees, qsize, head, 6, proof_host)) return rc;
  if (stage_ms) r.times(stage_ms, 6);
  *n_words = total;
  return ZKIR_OK;
}

}  // namespace

extern "C" {

int zkir_mixed_eval_prove(zkir_stark_ctx* const* ctxs, uint32_t n_groups, const uint32_t* n_mats, const uint32_t* const* lde_mats, const uint32_t* widths, const uint32_t* const* trees,
                          const uint32_t* masks, const uint32_t* points, const uint32_t* n_points, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words,
                          uint64_t* n_words, void* stream) {
  return mixed_prove_impl(ctxs, n_groups, n_mats, lde_mats, widths, trees, masks, points, n_points, num_queries, pow_bits, proof_host, cap_words, n_words, nullptr, (hipStream_t)stream);
}

// (zkir_amd_experimental.h) the same proof with the device time of its six stages: weights | evaluations | quotients | FRI commit phase | grinding | query section
int zkir_mixed_eval_prove_stages(zkir_stark_ctx* const* ctxs, uint32_t n_groups, const uint32_t* n_mats, const uint32_t* const* lde_mats, const uint32_t* widths,
                                 const uint32_t* const* trees, const uint32_t* masks, const uint32_t* points, const uint32_t* n_points, uint32_t num_queries, uint32_t pow_bits,
                                 uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words, float stage_ms[6], void* stream) {
  return mixed_prove_impl(ctxs, n_groups, n_mats, lde_mats, widths, trees, masks, points, n_points, num_queries, pow_bits, proof_host, cap_words, n_words, stage_ms, (hipStream_t)stream);
}

// (zkir_amd_experimental.h) fri_fold_k_kernel alone: the layer of 2^log_m values of the context's FRI (layer[t m + j], canonical, DEVICE; log_m at most log_n + log_blowup: the
// shift is 31^(2^(log_n + log_blowup - log_m))) folded k (1 .. 3) times with beta (HOST, canonical E4), beta^2, beta^4 into out[t g + i], g = m >> k; addend (DEVICE, 4 g
// words, or NULL) is added by index.  The challenges are uploaded with a synchronous copy into a block allocated and freed here: a test and measurement entry.
int zkir_fri_fold_launch(const zkir_stark_ctx* c, const uint32_t* layer, uint32_t log_m, uint32_t k, const uint32_t beta[4], const uint32_t* addend, uint32_t* out, void* stream) {
  const char* why = !c || !layer || !beta || !out ? "null argument" : k < 1 || k > 3 ? "k must be 1 .. 3" : log_m < k || log_m > c->log_n + c->log_blowup ? "log_m must be k .. log_n + log_blowup" : nullptr;
  if (!why) for (int t = 0; t < 4; t++) if (beta[t] >= bb::P) why = "beta must be canonical";
  if (why) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, std::string("zkir_fri_fold_launch: ") + why}); return ZKIR_ERR_ARGUMENT; }
  const uint32_t log_2n = c->log_n + c->log_blowup;
  uint32_t shift = bb::GEN;
  for (uint32_t f = log_m; f < log_2n; f++) shift = bb::mul(shift, shift);
  FoldParams fp{};
  E4 bm[3], cur = bb::e_to_mont(E4{{beta[0], beta[1], beta[2], beta[3]}});
  for (uint32_t f = 0; f < 3; f++) {
    if (f < k) { fp.half_shift_inv_m[f] = bb::to_mont(bb::inv(bb::mul(2, shift))); shift = bb::mul(shift, shift); }
    bm[f] = cur; cur = bb::e_mul_m(cur, cur);
  }
  E4* dBeta = nullptr;
  HIP_OK(hipMalloc((void**)&dBeta, sizeof(bm)));
  const hipError_t up = hipMemcpy(dBeta, bm, sizeof(bm), hipMemcpyHostToDevice);
  if (up == hipSuccess) {
    fri_launch_fold((int)k, layer, log_m, log_2n, c->d_tw_fwd, fp, dBeta, out, addend, (hipStream_t)stream);
    (void)hipStreamSynchronize((hipStream_t)stream);                         // the challenges are freed below
  }
  (void)hipFree(dBeta);
  if (up != hipSuccess) { zkir::set_last_error({ZKIR_ERR_DEVICE, std::string("zkir_fri_fold_launch: ") + hipGetErrorString(up)}); return ZKIR_ERR_DEVICE; }
  return check_launch("fri_fold");
}

}  // extern "C"
