// stark_verify.inl — zkir_verify_on_device, zkir_verify_many_on_device, zkir_verify_chain_on_device (include/zkir_amd.h) and zkir_stark_query_stage_probe
// (zkir_amd_experimental.h): the product's own verifier with its QUERY STAGE (verify_stages.h: StarkQueries, checks 20 .. 27 of all queries) on the device, for ONE proof,
// for MANY independent proofs, or for the segments of a CHAIN — always one batch.  Included by stark.hip at file scope, after pcs_verify.inl, whose __device__ pieces
// (the row-of-16 sponge-and-path chain, the wave-wide layer-0 sum, sum (a_i - A_i) / (z_i - x), the fold step and the layer table) the two kernels here call.
//
// Everything before the stage — header, program, cells, tapes (a mode-4 proof's through verify_device.inl's tape stages), the whole transcript, the constraints at zeta,
// the final layer's degree, grinding, the sampling — is verify.cpp's host code, run first, proof after proof.  One stage run then serves n proofs whose SHAPES DIFFER
// (mode, so the widths; log_n, so depths and schedule; the number of queries): the shape is a per-proof record in device memory (StarkShape) and a job finds its proof by
// a binary search in a prefix table the host writes.  ONE staged upload, TWO launches, one download of the flags, one synchronisation on the caller's stream:
//   stark_hash_jobs_kernel   sum_i n_full_i (6 + n_layers_i) jobs, a row of 16 lanes each: a matrix record's row or a FRI layer's values hashed and walked up to its root
//   stark_value_kernel       a wave per (proof, query, half): the layer-0 value by PcsQueries' rule (n_points = 2, z = (zeta, zeta w), a = (a0, b0), five selections);
//                            a lane per (proof, query, layer): the layer's own values folded and compared with the next layer's word or the final layer
// and the host picks each proof's verdict in the order the host loop returns it (stark_resolve).
//
// THE BLOCK.  [shapes: n StarkShape][prefix tables: hash jobs, queries, fold lanes, n + 1 words each][per proof: samples, gamma table, betas, layer table][per proof: its
// words from the trace root to the end of its last whole query][flags: hash jobs | layer-0 waves | fold lanes].  Everything before the flags is the one upload.
//
// UNTRUSTED INPUT.  The stage runs after verify_impl's word-range scan (every word from word 2 on is below p) and after the header checks (the mode fixes WM / WA,
// log_n <= 26, at most 128 queries), so every extent below is a function of checked words.  The proof's LENGTH is not checked before the queries: the device takes only the
// n_full = min(num_queries, (len - at_queries) / qsize) queries that lie wholly inside the proof, the host loop the rest (the cut one decides), merged in query order.  The
// row a job opens is the transcript's sample, never the proof's index word (which only the host compares: check 20).  Only the words from the trace root to the end of the
// last whole query are uploaded — never the program, the cells or the tapes in front of them — and no kernel reads outside them.
namespace {

constexpr uint32_t STARK_MAX_SLOTS = 6 + zkir::PCS_MAX_LAYERS;   // the hash jobs of one query: three matrices at two rows, the layers

// One proof's shape, DEVICE MEMORY.  Offsets of the proof's words are counted from its trace root (the first uploaded word), which stands at word `base` of the block.
struct StarkShape {
  uint64_t base;
  uint32_t o_qs, o_gamma, o_betas, o_ltab;                       // the proof's tables, words of the block
  uint32_t at_queries, qsize, at_fin;
  uint32_t n_layers, n_slots, log_M, fin_mask, wM_m, lay0_off;
  uint32_t leaf_off[STARK_MAX_SLOTS], leaf_words[STARK_MAX_SLOTS], depth[STARK_MAX_SLOTS], root_at[STARK_MAX_SLOTS], idx_add[STARK_MAX_SLOTS];
  uint32_t widths[3], rec_off[3];                                // main, aux, quotient: the record at q (the one at q + N follows it, widths[m] + 4 log_M words on)
  uint32_t sel_point[5], sel_mat[5], sel_e0[5];
  uint32_t z_m[2][4], a_m[2][4];
};

// the proof a job belongs to: the largest i < n with prefix[i] <= id (prefix[0] = 0, prefix rising; a proof without jobs has an empty range and is never found)
__device__ __forceinline__ uint32_t stark_proof_of(const uint32_t* __restrict__ prefix, uint32_t n, uint32_t id) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (prefix[mid] <= id) lo = mid; else hi = mid; }
  return lo;
}

// A row of 16 lanes per leaf-and-path job; job -> (proof i, query t, slot).  flags[job] = 0 / 1.
__global__ __launch_bounds__(NT_MV) void stark_hash_jobs_kernel(const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ blk, const StarkShape* __restrict__ shapes,
                                                                const uint32_t* __restrict__ hj, uint32_t n, uint32_t n_jobs, uint32_t* __restrict__ flags) {
  const uint32_t job = (blockIdx.x * NT_MV + threadIdx.x) / 16;
  const uint32_t l = threadIdx.x & 15;
  if (job >= n_jobs) return;                                     // (whole rows)
  const uint32_t i = stark_proof_of(hj, n, job);
  const StarkShape& sh = shapes[i];
  const uint32_t local = job - hj[i], t = local / sh.n_slots, slot = local - t * sh.n_slots;
  const uint32_t* w = blk + sh.base;
  const uint32_t depth = sh.depth[slot], width = sh.leaf_words[slot];
  const uint32_t j = (blk[sh.o_qs + t] + sh.idx_add[slot]) & ((1u << depth) - 1u);
  const uint32_t* r = w + sh.at_queries + (uint64_t)t * sh.qsize + sh.leaf_off[slot];
  const uint32_t eq = pcs_row16_hashes_to(cp, r, width, depth, j, w + sh.root_at[slot], l);
  if (l == 0) flags[job] = eq ? 0u : 1u;
}

// Workgroups [0, n_waves): a WAVE per (proof, query t, half s2), wave id = 2 (cq[i] + t) + s2 — the layer-0 value at row q + s2 N against layer 0's value s2 (check 24):
// flags24[wave].  The workgroups behind them: a LANE per (proof, query t, layer j), lane id = fj[i] + t n_layers + j — layer j's own values folded and compared with the
// next layer's v[slot] (check 25 of layer j + 1) or the final layer's value (check 26): flags_fold[lane id].
__global__ __launch_bounds__(64) void stark_value_kernel(const uint32_t* __restrict__ blk, const StarkShape* __restrict__ shapes, const uint32_t* __restrict__ cq,
                                                         const uint32_t* __restrict__ fj, uint32_t n, uint32_t n_waves, uint32_t n_folds, uint32_t* __restrict__ flags24,
                                                         uint32_t* __restrict__ flags_fold) {
  const uint32_t lane = threadIdx.x;
  if (blockIdx.x < n_waves) {
    const uint32_t qid = blockIdx.x >> 1, s2 = blockIdx.x & 1u;
    const uint32_t i = stark_proof_of(cq, n, qid);
    const StarkShape& sh = shapes[i];
    const uint32_t t = qid - cq[i];
    const uint32_t pos = blk[sh.o_qs + t] + (s2 ? 1u << (sh.log_M - 1) : 0u);
    const uint32_t* qb = blk + sh.base + sh.at_queries + (uint64_t)t * sh.qsize;
    E4 A0 = bb::e_zero(), A1 = bb::e_zero();
    for (uint32_t si = 0; si < 5; si++) {
      const uint32_t m = sh.sel_mat[si], width = sh.widths[m];
      const E4 acc = pcs_row_dot(blk + sh.o_gamma + 4 * (uint64_t)sh.sel_e0[si], qb + sh.rec_off[m] + s2 * (width + 4 * sh.log_M), width, lane);
      if (sh.sel_point[si] == 0) A0 = bb::e_add(A0, acc); else A1 = bb::e_add(A1, acc);
    }
    pcs_wave_sum(A0, A1);
    const E4 want = pcs_point_sum(2, sh.z_m, sh.a_m, A0, A1, sh.wM_m, pos);
    const E4 v = pcs_load_m(qb + sh.lay0_off + 4 * s2);
    if (lane == 0) flags24[blockIdx.x] = pcs_differ(v, want) ? 1u : 0u;
    return;
  }
  const uint32_t id = (blockIdx.x - n_waves) * 64 + lane;
  if (id >= n_folds) return;
  const uint32_t i = stark_proof_of(fj, n, id);
  const StarkShape& sh = shapes[i];
  const uint32_t local = id - fj[i], t = local / sh.n_layers, j = local - t * sh.n_layers;
  const uint32_t* w = blk + sh.base;
  const uint32_t* qb = w + sh.at_queries + (uint64_t)t * sh.qsize;
  const uint32_t* L = blk + sh.o_ltab + PCS_LAYER_WORDS * j;
  const uint32_t idx = blk[sh.o_qs + t] & ((1u << L[PCS_L_DEPTH]) - 1u);
  const E4 got = pcs_fold_lane(qb + L[PCS_L_OFF], L, blk + sh.o_betas + 4 * j, idx);
  const uint32_t* nxt = j + 1 < sh.n_layers ? qb + L[PCS_LAYER_WORDS + PCS_L_OFF] + 4 * (idx >> L[PCS_LAYER_WORDS + PCS_L_DEPTH]) : w + sh.at_fin + 4 * (idx & sh.fin_mask);
  flags_fold[id] = pcs_differ(pcs_load_m(nxt), got) ? 1u : 0u;
}

// One proof's verdict from its flags (fh: n_full n_slots hash flags, f24: 2 n_full, ff: n_full n_layers), with check 20 from the proof's own index words, in the host loop's
// order: for t rising — 20; 21 (main at q, at q + N); 27 (aux); 22 (quotient); per layer j: 23, then 24 (j = 0) or 25 (j > 0); 26.
int stark_resolve(const zkir::StarkQueries& Q, uint32_t n_full, const uint32_t* fh, const uint32_t* f24, const uint32_t* ff) {
  const uint32_t nl = Q.n_layers, n_slots = 6 + nl;
  for (uint32_t t = 0; t < n_full; t++) {
    if (Q.w[Q.at_queries + (uint64_t)t * Q.qsize] != Q.qs[t]) return 20;
    const uint32_t* h = fh + (size_t)t * n_slots;
    if (h[0] | h[1]) return 21;
    if (h[2] | h[3]) return 27;
    if (h[4] | h[5]) return 22;
    for (uint32_t j = 0; j < nl; j++) {
      if (h[6 + j]) return 23;
      if (j == 0 ? (f24[2 * t] | f24[2 * t + 1]) : ff[(size_t)t * nl + j - 1]) return j == 0 ? 24 : 25;
    }
    if (ff[(size_t)t * nl + nl - 1]) return 26;
  }
  return 0;
}

// ZKIR_VERIFY_QUERIES_TIMES (measurements: scripts/time_verify.py --queries): the stage synchronises after the upload and after the kernels and keeps host clocks of its parts
thread_local double stark_last_ms[3] = {0, 0, 0};               // upload, kernels, download

// The device form of the STARK query stage.
struct StarkDeviceStage {
  hipStream_t s;
  uint64_t hash_jobs = 0, value_jobs = 0, uploaded_words = 0; uint32_t launches = 0;      // what the run launched (zkir_verify_queries_last)
  int run(const zkir::StarkQueries* list, uint32_t n, int* codes) {
    if (!n) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_verify_*_on_device: no current HIP device"}); return -ZKIR_ERR_DEVICE; }
    VerifyDevice& V = verify_device(dev);
    std::lock_guard<std::mutex> lock(V.mu);
    V.pin.reset();
    // ---- the shapes and the layout: every offset from checked words ----
    std::vector<StarkShape> shapes(n);
    std::vector<uint32_t> pre(3 * ((size_t)n + 1), 0), n_full(n);
    uint32_t *hj = pre.data(), *cq = hj + n + 1, *fj = cq + n + 1;
    const size_t o_pre = al256((size_t)n * sizeof(StarkShape)), o_tab = o_pre + al256(pre.size() * 4);
    size_t at = o_tab / 4;                                       // (words of the block)
    std::vector<uint32_t> ltab((size_t)n * zkir::PCS_MAX_LAYERS * PCS_LAYER_WORDS, 0);
    for (uint32_t i = 0; i < n; i++) {
      const zkir::StarkQueries& Q = list[i];
      StarkShape& sh = shapes[i];
      memset(&sh, 0, sizeof sh);
      const uint32_t nl = Q.n_layers, WT = Q.WM + Q.WA, log_M = Q.log_n + 1;
      if (nl < 1 || nl > zkir::PCS_MAX_LAYERS || Q.num_queries > 128 || Q.log_n > 26 || Q.at_queries > Q.len || Q.at_roots >= Q.at_queries || Q.qs.size() != Q.num_queries || Q.betas_m.size() != 4 * (size_t)nl ||
          Q.gamma_m.size() != 4 * (2 * (size_t)WT + 4) || !Q.qsize) {
        zkir::set_last_error({ZKIR_ERR_OTHER, "zkir_verify_*_on_device: a query description is not a checked proof's"}); return -ZKIR_ERR_OTHER;
      }
      n_full[i] = (uint32_t)std::min<uint64_t>(Q.num_queries, (Q.len - Q.at_queries) / Q.qsize);
      hj[i + 1] = hj[i] + n_full[i] * (6 + nl); cq[i + 1] = cq[i] + n_full[i]; fj[i + 1] = fj[i] + n_full[i] * nl;
      sh.at_queries = (uint32_t)(Q.at_queries - Q.at_roots); sh.qsize = (uint32_t)Q.qsize; sh.at_fin = (uint32_t)(Q.at_fin - Q.at_roots);
      sh.n_layers = nl; sh.n_slots = 6 + nl; sh.log_M = log_M; sh.fin_mask = (4u << 1) - 1u; sh.wM_m = bb::to_mont(bb::root_of_unity((int)log_M));
      const uint32_t widths[3] = {Q.WM, Q.WA, 4};
      uint32_t off = 1;                                          // (the index word)
      for (uint32_t m = 0; m < 3; m++) {
        sh.widths[m] = widths[m]; sh.rec_off[m] = off;
        for (uint32_t s2 = 0; s2 < 2; s2++) {
          const uint32_t sl = 2 * m + s2;
          sh.leaf_off[sl] = off; sh.leaf_words[sl] = widths[m]; sh.depth[sl] = log_M; sh.root_at[sl] = 4 * m; sh.idx_add[sl] = s2 ? 1u << Q.log_n : 0u;
          off += widths[m] + 4 * log_M;
        }
      }
      uint32_t* lt = ltab.data() + (size_t)i * zkir::PCS_MAX_LAYERS * PCS_LAYER_WORDS;
      uint32_t shift = bb::GEN, log_m = log_M;
      for (uint32_t j = 0; j < nl; j++) {
        const uint32_t k = Q.ks[j];
        if (k < 1 || k > 3 || k > log_m) { zkir::set_last_error({ZKIR_ERR_OTHER, "zkir_verify_*_on_device: a query description is not a checked proof's"}); return -ZKIR_ERR_OTHER; }
        const uint32_t depth = log_m - k, sl = 6 + j;
        sh.leaf_off[sl] = off; sh.leaf_words[sl] = 4u << k; sh.depth[sl] = depth; sh.root_at[sl] = (uint32_t)(Q.at_lroots - Q.at_roots) + 4 * j; sh.idx_add[sl] = 0;
        uint32_t* L = lt + PCS_LAYER_WORDS * j;
        L[PCS_L_OFF] = off; L[PCS_L_K] = k; L[PCS_L_DEPTH] = depth; L[PCS_L_LOG_M] = log_m;
        if (j == 0) sh.lay0_off = off;
        for (uint32_t f = 0; f < k; f++) {
          L[PCS_L_INV2SHIFT + f] = bb::to_mont(bb::inv(bb::mul(2, shift))); L[PCS_L_WM + f] = bb::to_mont(bb::root_of_unity((int)log_m));
          shift = bb::mul(shift, shift); log_m--;
        }
        off += (4u << k) + 4 * depth;
      }
      if (off != Q.qsize || Q.at_lroots < Q.at_roots + 12 || Q.at_fin != Q.at_lroots + 4 * (uint64_t)nl || Q.at_queries != Q.at_fin + 4 * 8 + 1) {
        zkir::set_last_error({ZKIR_ERR_OTHER, "zkir_verify_*_on_device: the query section is not the header's"}); return -ZKIR_ERR_OTHER;
      }
      // the rule as data: A = main | aux | quotient at gamma^0.., B = main | aux at gamma^WT..
      const uint32_t sp[5] = {0, 0, 0, 1, 1}, sm[5] = {0, 1, 2, 0, 1}, se[5] = {0, Q.WM, 2 * WT, WT, WT + Q.WM};
      for (int k = 0; k < 5; k++) { sh.sel_point[k] = sp[k]; sh.sel_mat[k] = sm[k]; sh.sel_e0[k] = se[k]; }
      memcpy(sh.z_m[0], Q.zeta_m, 16); memcpy(sh.z_m[1], Q.zeta_w_m, 16); memcpy(sh.a_m[0], Q.a0_m, 16); memcpy(sh.a_m[1], Q.b0_m, 16);
      sh.o_qs = (uint32_t)at; at += (Q.num_queries + 3) & ~3u;
      sh.o_gamma = (uint32_t)at; at += Q.gamma_m.size();
      sh.o_betas = (uint32_t)at; at += 4 * (size_t)nl;
      sh.o_ltab = (uint32_t)at; at += (size_t)nl * PCS_LAYER_WORDS;
      if (at >> 31) { zkir::set_last_error({ZKIR_ERR_OTHER, "zkir_verify_*_on_device: the batch's tables are too large"}); return -ZKIR_ERR_OTHER; }
    }
    const size_t o_words = al256(at * 4);
    at = o_words / 4;
    for (uint32_t i = 0; i < n; i++) {
      const zkir::StarkQueries& Q = list[i];
      shapes[i].base = at;
      const uint64_t nw = n_full[i] ? (Q.at_queries - Q.at_roots) + (uint64_t)n_full[i] * Q.qsize : 0;      // (a proof without a whole query sends nothing)
      at += (size_t)((nw + 3) & ~(uint64_t)3);
    }
    const uint64_t n_hash = hj[n], n_q = cq[n], n_fold = fj[n];
    if ((n_hash * 16) >> 31) { zkir::set_last_error({ZKIR_ERR_OTHER, "zkir_verify_*_on_device: too many jobs for one batch"}); return -ZKIR_ERR_OTHER; }
    for (uint32_t i = 0; i < n; i++) codes[i] = 0;
    if (n_q) {
      const size_t o_flags = al256(at * 4), n_flags = (size_t)(n_hash + 2 * n_q + n_fold), total = o_flags + al256(n_flags * 4);
      // ---- one staged upload ----
      const bool timed = getenv("ZKIR_VERIFY_QUERIES_TIMES") != nullptr;
      auto now = [] { return std::chrono::steady_clock::now(); };
      auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
      const auto t0 = now();
      const int erc = V.ensure(total);
      if (erc) return -erc;
      unsigned char* h = (unsigned char*)V.pin.take(o_flags);
      uint32_t* h_flags = V.pin.take_n<uint32_t>(n_flags);
      if (!h || !h_flags) { zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_verify_*_on_device: no pinned host memory"}); return -ZKIR_ERR_DEVICE; }
      memcpy(h, shapes.data(), (size_t)n * sizeof(StarkShape)); memcpy(h + o_pre, pre.data(), pre.size() * 4);
      uint32_t* hw = (uint32_t*)h;
      for (uint32_t i = 0; i < n; i++) {
        const zkir::StarkQueries& Q = list[i]; const StarkShape& sh = shapes[i];
        memcpy(hw + sh.o_qs, Q.qs.data(), (size_t)Q.num_queries * 4); memcpy(hw + sh.o_gamma, Q.gamma_m.data(), Q.gamma_m.size() * 4); memcpy(hw + sh.o_betas, Q.betas_m.data(), Q.betas_m.size() * 4);
        memcpy(hw + sh.o_ltab, ltab.data() + (size_t)i * zkir::PCS_MAX_LAYERS * PCS_LAYER_WORDS, (size_t)Q.n_layers * PCS_LAYER_WORDS * 4);
        if (n_full[i]) memcpy(hw + sh.base, Q.w + Q.at_roots, (size_t)((Q.at_queries - Q.at_roots) + (uint64_t)n_full[i] * Q.qsize) * 4);
      }
      if (hipMemcpyAsync(V.d, h, o_flags, hipMemcpyHostToDevice, s) != hipSuccess) { (void)check_launch("zkir_verify_*_on_device: upload"); return -ZKIR_ERR_DEVICE; }
      if (timed && hipStreamSynchronize(s) != hipSuccess) return -ZKIR_ERR_DEVICE;
      const auto t1 = now();
      // ---- two launches ----
      const uint32_t* d_blk = (const uint32_t*)V.d; const StarkShape* d_shapes = (const StarkShape*)V.d;
      const uint32_t *d_hj = (const uint32_t*)(V.d + o_pre), *d_cq = d_hj + n + 1, *d_fj = d_cq + n + 1;
      uint32_t* d_flags = (uint32_t*)(V.d + o_flags);
      uint32_t *d_f24 = d_flags + n_hash, *d_ff = d_f24 + 2 * n_q;
      hipLaunchKernelGGL(stark_hash_jobs_kernel, dim3(grid_for(n_hash * 16, NT_MV)), dim3(NT_MV), 0, s, V.d_p2, d_blk, d_shapes, d_hj, n, (uint32_t)n_hash, d_flags);
      hipLaunchKernelGGL(stark_value_kernel, dim3((unsigned)(2 * n_q) + grid_for(n_fold, 64)), dim3(64), 0, s, d_blk, d_shapes, d_cq, d_fj, n, (uint32_t)(2 * n_q), (uint32_t)n_fold, d_f24, d_ff);
      hash_jobs = n_hash; value_jobs = 2 * n_q + n_fold; launches = 2; uploaded_words = o_flags / 4;
      if (timed && hipStreamSynchronize(s) != hipSuccess) { (void)check_launch("zkir_verify_*_on_device: kernels"); return -ZKIR_ERR_DEVICE; }
      const auto t2 = now();
      // ---- one download, one synchronisation ----
      if (hipMemcpyAsync(h_flags, d_flags, n_flags * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess || check_launch("zkir_verify_*_on_device: query stage") != ZKIR_OK) {
        (void)check_launch("zkir_verify_*_on_device: query stage"); return -ZKIR_ERR_DEVICE;
      }
      const auto t3 = now();
      if (timed) { stark_last_ms[0] = ms(t0, t1); stark_last_ms[1] = ms(t1, t2); stark_last_ms[2] = ms(t2, t3); }
      for (uint32_t i = 0; i < n; i++) codes[i] = stark_resolve(list[i], n_full[i], h_flags + hj[i], h_flags + n_hash + 2 * (size_t)cq[i], h_flags + n_hash + 2 * n_q + fj[i]);
    }
    // the queries a short proof cuts: the host loop's codes, behind the whole queries' (query order)
    for (uint32_t i = 0; i < n; i++) if (!codes[i] && n_full[i] < list[i].num_queries) codes[i] = zkir::stark_host_queries_from(list[i], n_full[i]);
    return 0;
  }
  void note() const { zkir::verify_note_queries(hash_jobs, value_jobs, launches, uploaded_words); }
};
int stark_device_run(void* p, const zkir::StarkQueries* list, uint32_t n, int* codes) { return guarded([&] { return static_cast<StarkDeviceStage*>(p)->run(list, n, codes); }); }

int stark_refuse(const char* m) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, m}); return ZKIR_ERR_ARGUMENT; }

}  // namespace

extern "C" {

int zkir_verify_on_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, void* stream) {
  stark_last_ms[0] = stark_last_ms[1] = stark_last_ms[2] = 0;
  return guarded([&]() -> int {
    zkir::StarkQueries Q;
    uint32_t stages_run = 0;
    const int rc = verify_device_part(proof, proof_words, expect, stream, &Q, &stages_run);
    zkir::verify_note_device_stages(stages_run);
    if (rc) return rc;
    StarkDeviceStage st{(hipStream_t)stream};
    int code = 0;
    const int src = st.run(&Q, 1, &code);
    if (src) return src;
    st.note();
    return code ? code : zkir::stark_length_check(Q);
  });
}

int zkir_verify_many_on_device(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts, void* stream) {
  stark_last_ms[0] = stark_last_ms[1] = stark_last_ms[2] = 0;
  if (!proofs || !proof_words || !verdicts) return stark_refuse("zkir_verify_many_on_device: null proofs, proof_words or verdicts");
  if (n < 1 || n > 1024) return stark_refuse("zkir_verify_many_on_device: n must be 1 .. 1024");
  return guarded([&]() -> int {
    std::vector<int32_t> out(n, 0);
    std::vector<zkir::StarkQueries> list;
    std::vector<uint32_t> who;
    uint32_t stages_total = 0;
    for (uint32_t i = 0; i < n; i++) {                           // the host parts, proof after proof (a mode-4 proof's tapes through the device tape stages, which reset the
      zkir::StarkQueries Q;                                      //  per-device staging: a description owns its draws)
      uint32_t stages_run = 0;
      const int rc = verify_device_part(proofs[i], proof_words[i], expects ? expects[i] : nullptr, stream, &Q, &stages_run);
      stages_total += stages_run;
      if (rc < 0) return rc;
      out[i] = rc;
      if (!rc) { list.push_back(std::move(Q)); who.push_back(i); }
    }
    zkir::verify_note_device_stages(stages_total);
    StarkDeviceStage st{(hipStream_t)stream};
    std::vector<int> codes(list.size() + 1, 0);
    if (!list.empty()) {                                         // (no proof reached its queries: nothing is launched)
      const int src = st.run(list.data(), (uint32_t)list.size(), codes.data());
      if (src) return src;
    }
    st.note();
    for (size_t k = 0; k < list.size(); k++) out[who[k]] = codes[k] ? codes[k] : zkir::stark_length_check(list[k]);
    memcpy(verdicts, out.data(), (size_t)n * sizeof(int32_t));
    return 0;
  });
}

int zkir_verify_chain_on_device(const uint32_t* const* proofs, const uint64_t* proof_words, uint32_t n_segments, const zkir_public_inputs* expect, void* stream) {
  if (proofs && proof_words && n_segments == 1 && proofs[0] && proof_words[0] > 9 && proofs[0][9] >= 3) return zkir_verify_on_device(proofs[0], proof_words[0], expect, stream);      // a whole run by itself
  stark_last_ms[0] = stark_last_ms[1] = stark_last_ms[2] = 0;
  StarkDeviceStage st{(hipStream_t)stream};
  const int rc = guarded([&] { return zkir::verify_chain_with_stage(proofs, proof_words, n_segments, expect, zkir::StarkQueryStage{&st, stark_device_run}); });
  zkir::verify_note_device_stages(0);
  if (rc >= 0) st.note();
  return rc;
}

int zkir_verify_queries_last_stage_ms(double ms[3]) {
  if (!ms) return ZKIR_ERR_ARGUMENT;
  for (int k = 0; k < 3; k++) ms[k] = stark_last_ms[k];
  return ZKIR_OK;
}

int zkir_stark_query_stage_probe(const uint32_t* proof, uint64_t proof_words, uint32_t what, uint32_t index, int device, void* stream) {
  return guarded([&]() -> int {
    zkir::StarkQueries Q;
    const int rc = zkir::stark_verify_collect(proof, proof_words, nullptr, true, nullptr, &Q);
    if (rc) return rc;
    auto bump = [](uint32_t* e) { e[0] = bb::add(e[0], bb::R1); };      // + 1 on a Montgomery E4
    switch (what) {
      case 0: break;
      case 1: bump(Q.a0_m); break;
      case 2: bump(Q.b0_m); break;
      case 3: bump(Q.zeta_m); break;
      case 4: if (index >= Q.n_layers) return -stark_refuse("zkir_stark_query_stage_probe: no such layer"); bump(Q.betas_m.data() + 4 * (size_t)index); break;
      case 5: if (index >= Q.num_queries) return -stark_refuse("zkir_stark_query_stage_probe: no such query"); Q.qs[index] ^= 1u; break;
      default: return -stark_refuse("zkir_stark_query_stage_probe: what must be 0 .. 5");
    }
    int code = 0;
    if (device) {
      StarkDeviceStage st{(hipStream_t)stream};
      const int src = st.run(&Q, 1, &code);
      if (src) return src;
      st.note();
    } else {
      const zkir::StarkQueryStage hs = zkir::host_stark_query_stage();
      const int src = hs.run(hs.self, &Q, 1, &code);
      if (src) return src;
    }
    return code ? code : zkir::stark_length_check(Q);
  });
}

}  // extern "C"
