// mixed_verify.inl — zkir_mixed_eval_verify_device (include/zkir_amd.h): the verifier of a mixed-height evaluation proof ('ZKMH') with its QUERY STAGE (verify_stages.h:
// MixedQueries, checks 6 .. 11 of all queries) on the device.  Included by stark.hip at file scope, after query_stage.inl, whose __device__ pieces and layout builder it
// uses and whose untrusted-input contract it keeps (the stage runs after checks 1 and 3, so the proof's length is EXACTLY its header's and every word is below p), and
// after pcs_verify.inl, whose per-thread job counts and stage clocks it shares.  Its kernels and its block are its own — a query's rule differs by group and a fold may
// add another launch's value — under the same contract: verify_device(dev)'s block, pinned staging and mutex; one staged upload, one download, one synchronisation on the
// caller's stream; nothing launched when the verdict is 1 .. 5, 12 or 13 (verify.cpp's host code runs first and unchanged); a negative return is "no verdict".
//
// THREE launches on the one stream:
//   mixed_hash_jobs_kernel   num_queries (2 n_mats_0 + sum_{h>=1} n_mats_h + n_layers) jobs, a row of 16 lanes each.  A query's slots in the order its records stand:
//                            group 0's matrices at q and q + M_0/2 (depth log M_0), each lower group's matrices once at depth log M_h with idx_add = 0 (the kernel's
//                            mask gives q mod M_h), the FRI layers
//   mixed_value_kernel       a wave per (query, half) — group 0's rule at q / q + M_0/2 against layer 0's values (check 8) — and a wave per (query, lower group h):
//                            F_h(q mod M_h) by group h's rule at x = 31 w_{M_h}^(q mod M_h), four Montgomery words to the F buffer, no comparison
//   mixed_fold_kernel        a lane per (query, layer j): layer j's own values folded and compared with the next layer's v[slot] — PLUS the stored F_h when the next
//                            layer has size M_h — or, for the last layer, with the final layer (no M_h is the final layer's size)
// WHY THREE.  A fold lane whose next layer has size M_h needs F_h of its query, which another workgroup forms; a lane cannot wait for a workgroup of its own launch (it
// may not be resident yet), so the folds are a launch of their own behind the values' launch and the stream's order is the only synchronisation: no flag in device memory
// is ever waited for.  (Forming F_h inside the fold lane would keep two launches but puts a width-long column sum on one lane; 152 columns a wave is the measured case.)
namespace {

// The hash jobs' shape, BY VALUE: query_stage.inl's slots (leaf_off from the query's first word, the Merkle index (q + idx_add) mod 2^depth) for one proof whose query
// has up to MIXED_MAX_SLOTS of them, in this file's own order.
struct MixedHashShape {
  uint64_t at_queries, qsize;
  uint32_t n_slots, n_jobs;
  uint32_t leaf_off[zkir::MIXED_MAX_SLOTS], leaf_words[zkir::MIXED_MAX_SLOTS], depth[zkir::MIXED_MAX_SLOTS], root_at[zkir::MIXED_MAX_SLOTS], idx_add[zkir::MIXED_MAX_SLOTS];
};

// One leaf-and-path job a row of 16 lanes: flags[job] = 0 / 1, one plain store.
__global__ __launch_bounds__(NT_MV) void mixed_hash_jobs_kernel(const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ w, const uint32_t* __restrict__ qs, MixedHashShape sh, uint32_t* __restrict__ flags) {
  const uint32_t job = (blockIdx.x * NT_MV + threadIdx.x) / 16;
  const uint32_t l = threadIdx.x & 15;
  if (job >= sh.n_jobs) return;                                  // (whole rows)
  const uint32_t t = job / sh.n_slots, slot = job - t * sh.n_slots;
  const uint32_t depth = sh.depth[slot], width = sh.leaf_words[slot];
  const uint32_t j = (qs[t] + sh.idx_add[slot]) & ((1u << depth) - 1u);
  const uint32_t* r = w + sh.at_queries + (uint64_t)t * sh.qsize + sh.leaf_off[slot];
  const uint32_t eq = pcs_row16_hashes_to(cp, r, width, depth, j, w + sh.root_at[slot], l);
  if (l == 0) flags[job] = eq ? 0u : 1u;
}

// A group's layer-0 rule (PcsQueries' rule fields) as the value kernel reads it: DEVICE MEMORY, one per group — a wave picks its group at run time.  rec_off[m]: matrix
// m's record from the query's first word (group 0: the record at q; the one at q + M_0/2 follows it, widths[m] + 4 log_M words on).
struct MixedRule {
  uint32_t log_M, n_points, n_sel, wM_m;
  uint32_t widths[zkir::PCS_MAX_MATS], rec_off[zkir::PCS_MAX_MATS];
  uint32_t sel_point[zkir::PCS_MAX_SEL], sel_mat[zkir::PCS_MAX_SEL], sel_e0[zkir::PCS_MAX_SEL];
  uint32_t z_m[2][4], a_m[2][4];
};
constexpr uint32_t MIXED_L_ADD = 10;                             // layer table word (query_stage.inl's layout, its spare word): h >= 1 when the NEXT layer has size M_h, else 0
struct MixedValueShape {
  uint64_t at_queries, qsize, at_fin;
  uint32_t n_layers, num_queries, n_groups, fin_mask;
  uint32_t lay0_off;                                             // layer 0's values in a query
};

// query_value_kernel's layer-0 wave on rule r: sum_i (a_i - A_i) / (z_i - x), x = 31 w_M^pos, A_i from the rows at qb + rec_off (+ the second record's stride when s2);
// every lane returns the value (Montgomery)
__device__ __forceinline__ E4 mixed_rule_value(const uint32_t* __restrict__ qb, const uint32_t* __restrict__ gamma_m, const MixedRule& r, uint32_t pos, uint32_t s2, uint32_t lane) {
  E4 A0 = bb::e_zero(), A1 = bb::e_zero();
  for (uint32_t si = 0; si < r.n_sel; si++) {
    const uint32_t m = r.sel_mat[si], width = r.widths[m];
    const E4 acc = pcs_row_dot(gamma_m + 4 * (uint64_t)r.sel_e0[si], qb + r.rec_off[m] + s2 * (width + 4 * r.log_M), width, lane);
    if (r.sel_point[si] == 0) A0 = bb::e_add(A0, acc); else A1 = bb::e_add(A1, acc);
  }
  pcs_wave_sum(A0, A1);
  return pcs_point_sum(r.n_points, r.z_m, r.a_m, A0, A1, r.wM_m, pos);
}

// Workgroups [0, 2 num_queries): (query t, half s2) — check 8: flags8[2 t + s2].  The workgroups behind them: (query t, lower group h) — F_h(q mod M_h) to
// fbuf[4 (t (n_groups - 1) + h - 1) ..].
__global__ __launch_bounds__(64) void mixed_value_kernel(const uint32_t* __restrict__ w, const uint32_t* __restrict__ qs, const uint32_t* __restrict__ gamma_m,
                                                         const MixedRule* __restrict__ rules, MixedValueShape sh, uint32_t* __restrict__ flags8, uint32_t* __restrict__ fbuf) {
  const uint32_t lane = threadIdx.x;
  if (blockIdx.x < 2 * sh.num_queries) {
    const uint32_t t = blockIdx.x >> 1, s2 = blockIdx.x & 1u;
    const MixedRule& r = rules[0];
    const uint32_t* qb = w + sh.at_queries + (uint64_t)t * sh.qsize;
    const E4 want = mixed_rule_value(qb, gamma_m, r, qs[t] + (s2 ? 1u << (r.log_M - 1) : 0u), s2, lane);
    const E4 v = pcs_load_m(qb + sh.lay0_off + 4 * s2);
    if (lane == 0) flags8[blockIdx.x] = pcs_differ(v, want) ? 1u : 0u;
    return;
  }
  const uint32_t id = blockIdx.x - 2 * sh.num_queries;
  if (id >= sh.num_queries * (sh.n_groups - 1)) return;          // (the grid is exact)
  const uint32_t t = id / (sh.n_groups - 1), h = 1 + (id - t * (sh.n_groups - 1));
  const MixedRule& r = rules[h];
  const E4 F = mixed_rule_value(w + sh.at_queries + (uint64_t)t * sh.qsize, gamma_m, r, qs[t] & ((1u << r.log_M) - 1u), 0, lane);
  if (lane < 4) fbuf[4 * (size_t)id + lane] = lane == 0 ? F.c[0] : lane == 1 ? F.c[1] : lane == 2 ? F.c[2] : F.c[3];
}

// query_value_kernel's fold lanes with the one new rule: L[MIXED_L_ADD] = h >= 1 — the next layer has size M_h — and the lane compares that layer's v[slot] with its fold
// plus the query's F_h.  The layer table and the F buffer are device memory.
__global__ __launch_bounds__(64) void mixed_fold_kernel(const uint32_t* __restrict__ w, const uint32_t* __restrict__ qs, const uint32_t* __restrict__ betas_m,
                                                        const uint32_t* __restrict__ ltab, const uint32_t* __restrict__ fbuf, MixedValueShape sh, uint32_t* __restrict__ flags_fold) {
  const uint32_t id = blockIdx.x * 64 + threadIdx.x;
  if (id >= sh.num_queries * sh.n_layers) return;
  const uint32_t t = id / sh.n_layers, j = id - t * sh.n_layers;
  const uint32_t* qb = w + sh.at_queries + (uint64_t)t * sh.qsize;
  const uint32_t* L = ltab + PCS_LAYER_WORDS * j;
  const uint32_t add = L[MIXED_L_ADD];
  const uint32_t idx = qs[t] & ((1u << L[PCS_L_DEPTH]) - 1u);
  E4 got = pcs_fold_lane(qb + L[PCS_L_OFF], L, betas_m + 4 * j, idx);
  if (add) {
    const uint32_t* f = fbuf + 4 * ((size_t)t * (sh.n_groups - 1) + add - 1);
    got = bb::e_add(got, E4{{f[0], f[1], f[2], f[3]}});
  }
  const uint32_t* nxt = j + 1 < sh.n_layers ? qb + L[PCS_LAYER_WORDS + PCS_L_OFF] + 4 * (idx >> L[PCS_LAYER_WORDS + PCS_L_DEPTH]) : w + sh.at_fin + 4 * (idx & sh.fin_mask);
  flags_fold[id] = pcs_differ(pcs_load_m(nxt), got) ? 1u : 0u;
}

// The verdict from the flags in the host loop's order: for t rising — 6; 7 for the records in the order they stand in the query; 8; per layer j: 9 (j), then 10 (j) for
// j > 0; 11.
int mixed_resolve(const zkir::MixedQueries& Q, uint32_t n_rec, const uint32_t* fh, const uint32_t* f8, const uint32_t* ff) {
  const uint32_t n_slots = n_rec + Q.n_layers;
  for (uint32_t t = 0; t < Q.num_queries; t++) {
    if (Q.w[Q.at_queries + (uint64_t)t * Q.qsize] != Q.qs[t]) return 6;
    const uint32_t* h = fh + (size_t)t * n_slots;
    for (uint32_t sl = 0; sl < n_rec; sl++) if (h[sl]) return 7;
    if (f8[2 * t] | f8[2 * t + 1]) return 8;
    for (uint32_t j = 0; j < Q.n_layers; j++) {
      if (h[n_rec + j]) return 9;
      if (j > 0 && ff[(size_t)t * Q.n_layers + j - 1]) return 10;
    }
    if (ff[(size_t)t * Q.n_layers + Q.n_layers - 1]) return 11;
  }
  return 0;
}

// The device form of the mixed query stage.  Block: [proof][samples][gamma table][betas][layer table][rules][flags: hash jobs | layer-0 | folds][F buffer]; the part before
// the flags is the one upload, the flags the one download; the F buffer never leaves the device.
struct MixedDeviceStage {
  hipStream_t s;
  int run(const zkir::MixedQueries& Q) {
    const char* const bad_shape = "zkir_mixed_eval_verify_device: the query section is not the header's";
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_mixed_eval_verify_device: no current HIP device"}); return -ZKIR_ERR_DEVICE; }
    // ---- the bounds of this path (verify.cpp has checked them; nothing below indexes past them) ----
    if (Q.n_groups < 2 || Q.n_groups > zkir::MIXED_MAX_GROUPS || Q.n_layers < 1 || Q.n_layers > zkir::MIXED_MAX_LAYERS || Q.num_queries < 1) { zkir::set_last_error({ZKIR_ERR_OTHER, bad_shape}); return -ZKIR_ERR_OTHER; }
    uint32_t n_rec = 0;
    for (uint32_t h = 0; h < Q.n_groups; h++) {
      const zkir::PcsQueries& g = Q.g[h];
      if (g.n_mats < 1 || g.n_mats > zkir::PCS_MAX_MATS || g.n_sel > zkir::PCS_MAX_SEL || g.n_points < 1 || g.n_points > 2 || g.log_M < 1 || g.log_M > 27 || (h && g.log_M >= Q.g[h - 1].log_M)) {
        zkir::set_last_error({ZKIR_ERR_OTHER, bad_shape}); return -ZKIR_ERR_OTHER;
      }
      n_rec += (h ? 1 : 2) * g.n_mats;
    }
    const uint32_t nq = Q.num_queries, n_lower = Q.n_groups - 1, n_slots = n_rec + Q.n_layers, n_gamma = Q.g[0].n_gamma;
    if (n_slots > zkir::MIXED_MAX_SLOTS) { zkir::set_last_error({ZKIR_ERR_OTHER, bad_shape}); return -ZKIR_ERR_OTHER; }
    VerifyDevice& V = verify_device(dev);
    std::lock_guard<std::mutex> lock(V.mu);
    V.pin.reset();
    const uint64_t hash_jobs = (uint64_t)nq * n_slots, value_jobs = (uint64_t)nq * (2 + n_lower + Q.n_layers);
    const size_t n_flags = (size_t)hash_jobs + (size_t)nq * (2 + Q.n_layers);
    const size_t o_qs = al256(Q.len * 4), o_gamma = o_qs + al256((size_t)nq * 4), o_betas = o_gamma + al256((size_t)n_gamma * 16), o_ltab = o_betas + al256((size_t)Q.n_layers * 16),
                 o_rules = o_ltab + al256((size_t)Q.n_layers * PCS_LAYER_WORDS * 4), o_flags = o_rules + al256(Q.n_groups * sizeof(MixedRule)), o_fbuf = o_flags + al256(n_flags * 4),
                 total = o_fbuf + al256((size_t)nq * n_lower * 16);
    // ---- the shapes: every offset from the checked header ----
    MixedHashShape hs{};
    MixedValueShape vs{};
    MixedRule rules[zkir::MIXED_MAX_GROUPS] = {};
    hs.at_queries = vs.at_queries = Q.at_queries; hs.qsize = vs.qsize = Q.qsize; vs.at_fin = Q.at_fin;
    hs.n_slots = n_slots; hs.n_jobs = (uint32_t)hash_jobs;
    vs.n_layers = Q.n_layers; vs.num_queries = nq; vs.n_groups = Q.n_groups; vs.fin_mask = (4u << Q.b) - 1u;
    QueryMat mats[zkir::MIXED_MAX_GROUPS * zkir::PCS_MAX_MATS];   // the records in the order they stand: group 0's twice, a lower group's once (the kernel's mask gives q mod M_h)
    uint32_t n_mats = 0;
    for (uint32_t h = 0; h < Q.n_groups; h++)
      for (uint32_t m = 0; m < Q.g[h].n_mats; m++) mats[n_mats++] = QueryMat{Q.g[h].widths[m], Q.g[h].log_M, (uint32_t)Q.at_roots + 4 * (Q.first_mat[h] + m), h ? 1u : 2u, 0};
    uint32_t ltab[zkir::MIXED_MAX_LAYERS * PCS_LAYER_WORDS];
    if (query_layout(Q.g[0].log_M, Q.b, Q.ks, Q.n_layers, (uint32_t)Q.at_lroots, mats, n_mats, Q.qsize, QuerySlots{hs.leaf_off, hs.leaf_words, hs.depth, hs.root_at, hs.idx_add}, ltab, &vs.lay0_off) ||
        Q.at_queries + (uint64_t)nq * Q.qsize != Q.len) { zkir::set_last_error({ZKIR_ERR_OTHER, bad_shape}); return -ZKIR_ERR_OTHER; }
    for (uint32_t j = 0; j + 1 < Q.n_layers; j++)                // the layer whose NEXT layer has the size of a lower group adds that group's F_h
      for (uint32_t h = 1; h < Q.n_groups; h++) if (Q.g[h].log_M == ltab[PCS_LAYER_WORDS * (j + 1) + PCS_L_LOG_M]) ltab[PCS_LAYER_WORDS * j + MIXED_L_ADD] = h;
    for (uint32_t h = 0, at = 0; h < Q.n_groups; h++) {
      const zkir::PcsQueries& g = Q.g[h];
      MixedRule& r = rules[h];
      r.log_M = g.log_M; r.n_points = g.n_points; r.n_sel = g.n_sel; r.wM_m = bb::to_mont(bb::root_of_unity((int)g.log_M));
      for (uint32_t i = 0; i < g.n_sel; i++) {
        if (g.sel[i].mat >= g.n_mats || g.sel[i].point >= g.n_points || (uint64_t)g.sel[i].e0 + g.widths[g.sel[i].mat] > n_gamma) { zkir::set_last_error({ZKIR_ERR_OTHER, bad_shape}); return -ZKIR_ERR_OTHER; }
        r.sel_point[i] = g.sel[i].point; r.sel_mat[i] = g.sel[i].mat; r.sel_e0[i] = g.sel[i].e0;
      }
      memcpy(r.z_m, g.z_m, sizeof r.z_m); memcpy(r.a_m, g.a_m, sizeof r.a_m);
      for (uint32_t m = 0; m < g.n_mats; m++, at++) { r.widths[m] = g.widths[m]; r.rec_off[m] = mats[at].rec_off; }
    }
    // ---- one staged upload ----
    const bool timed = getenv("ZKIR_PCS_VERIFY_TIMES") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t0 = now();
    const int erc = V.ensure(total);
    if (erc) return -erc;
    unsigned char* h = (unsigned char*)V.pin.take(o_flags);
    uint32_t* h_flags = V.pin.take_n<uint32_t>(n_flags);
    if (!h || !h_flags) { zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_mixed_eval_verify_device: no pinned host memory"}); return -ZKIR_ERR_DEVICE; }
    memcpy(h, Q.w, Q.len * 4); memcpy(h + o_qs, Q.qs, (size_t)nq * 4); memcpy(h + o_gamma, Q.g[0].gamma_m, (size_t)n_gamma * 16);
    memcpy(h + o_betas, Q.betas_m, (size_t)Q.n_layers * 16); memcpy(h + o_ltab, ltab, (size_t)Q.n_layers * PCS_LAYER_WORDS * 4); memcpy(h + o_rules, rules, Q.n_groups * sizeof(MixedRule));
    if (hipMemcpyAsync(V.d, h, o_flags, hipMemcpyHostToDevice, s) != hipSuccess) { (void)check_launch("zkir_mixed_eval_verify_device: upload"); return -ZKIR_ERR_DEVICE; }
    if (timed && hipStreamSynchronize(s) != hipSuccess) return -ZKIR_ERR_DEVICE;
    const auto t1 = now();
    // ---- three launches: the stream orders the folds behind the values they add ----
    const uint32_t* d_w = (const uint32_t*)V.d; const uint32_t* d_qs = (const uint32_t*)(V.d + o_qs); const uint32_t* d_gamma = (const uint32_t*)(V.d + o_gamma);
    const uint32_t* d_betas = (const uint32_t*)(V.d + o_betas); const uint32_t* d_ltab = (const uint32_t*)(V.d + o_ltab); const MixedRule* d_rules = (const MixedRule*)(V.d + o_rules);
    uint32_t* d_flags = (uint32_t*)(V.d + o_flags); uint32_t* d_fbuf = (uint32_t*)(V.d + o_fbuf);
    uint32_t *d_f8 = d_flags + hash_jobs, *d_ff = d_f8 + 2 * (size_t)nq;
    hipLaunchKernelGGL(mixed_hash_jobs_kernel, dim3(grid_for(hash_jobs * 16, NT_MV)), dim3(NT_MV), 0, s, V.d_p2, d_w, d_qs, hs, d_flags);
    hipLaunchKernelGGL(mixed_value_kernel, dim3(2 * nq + nq * n_lower), dim3(64), 0, s, d_w, d_qs, d_gamma, d_rules, vs, d_f8, d_fbuf);
    hipLaunchKernelGGL(mixed_fold_kernel, dim3(grid_for((uint64_t)nq * Q.n_layers, 64)), dim3(64), 0, s, d_w, d_qs, d_betas, d_ltab, (const uint32_t*)d_fbuf, vs, d_ff);
    pcs_last_jobs[0] = hash_jobs; pcs_last_jobs[1] = value_jobs;
    if (timed && hipStreamSynchronize(s) != hipSuccess) { (void)check_launch("zkir_mixed_eval_verify_device: kernels"); return -ZKIR_ERR_DEVICE; }
    const auto t2 = now();
    // ---- one download, one synchronisation ----
    if (hipMemcpyAsync(h_flags, d_flags, n_flags * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess || check_launch("zkir_mixed_eval_verify_device: query stage") != ZKIR_OK) {
      (void)check_launch("zkir_mixed_eval_verify_device: query stage"); return -ZKIR_ERR_DEVICE;
    }
    const auto t3 = now();
    if (timed) { pcs_last_ms[0] = ms(t0, t1); pcs_last_ms[1] = ms(t1, t2); pcs_last_ms[2] = ms(t2, t3); }
    return mixed_resolve(Q, n_rec, h_flags, h_flags + hash_jobs, h_flags + hash_jobs + 2 * (size_t)nq);
  }
};
int mixed_device_run(void* p, const zkir::MixedQueries& Q) { return guarded([&] { return static_cast<MixedDeviceStage*>(p)->run(Q); }); }

}  // namespace

extern "C" int zkir_mixed_eval_verify_device(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals, void* stream) {
  pcs_last_jobs[0] = pcs_last_jobs[1] = 0;
  pcs_last_ms[0] = pcs_last_ms[1] = pcs_last_ms[2] = 0;
  MixedDeviceStage st{(hipStream_t)stream};
  return guarded([&] { return zkir::mixed_eval_verify_with_stage(proof, n_words, expect_roots, expect_points, expect_evals, zkir::MixedQueryStage{&st, mixed_device_run}); });
}
