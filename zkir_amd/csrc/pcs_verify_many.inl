// pcs_verify_many.inl — the commitment layer's QUERY STAGE (verify_stages.h: checks 6 .. 11 of all queries) for a LIST of proofs whose shapes differ, and the entries over it
// (include/zkir_amd.h): zkir_verify_rate_segment_device, zkir_verify_rate_chain_device, zkir_verify_rate_many_device, zkir_pcs_verify_many_device.  Included by stark.hip at
// file scope, after pcs_verify.inl (whose __device__ pieces the two kernels call) and stark_verify.inl (stark_proof_of: the proof a job belongs to).
//
// Everything before the stage is verify.cpp's host code, run first, proof after proof, with a COLLECTING stage (verify_stages.h: PcsCollected) in place of the queries: the
// shape, the expectations, the word range, the whole transcript, the final-degree check, grinding, the sampling — for a 'ZKSR' proof the whole STARK front and the
// constraints at zeta before that.  One stage run then serves n 'ZKLD' / 'ZKEV' / 'ZKBE' proofs that may differ in log_M, the rate b (so the final layer's size and the
// schedule), the number of matrices (1 .. 4) and their widths, the points (0 .. 2), the selections (<= 8) and the number of queries: the shape is a per-proof record in
// device memory (PcsManyShape: the union of pcs_verify.inl's by-value PcsHashShape and PcsValueShape, plus where the proof's words and tables lie in the block), and a job
// finds its proof by a binary search in a prefix table the host writes.  ONE staged upload, TWO launches, one download of the flags, one synchronisation on the caller's
// stream, however many proofs; nothing is launched for an empty list:
//   pcs_hash_jobs_many_kernel   sum_i nq_i (2 n_mats_i + n_layers_i) jobs, a row of 16 lanes each: a matrix record's row or a FRI layer's values hashed and walked up to its root
//   pcs_value_many_kernel       a wave per (proof, query, half): the layer-0 value by the proof's own rule; a lane per (proof, query, layer): the layer's values folded and
//                               compared with the next layer's word or the final layer
// and the host picks each proof's verdict in the order the host loop returns it (pcs_resolve).
//
// THE BLOCK.  [shapes: n PcsManyShape][prefix tables: hash jobs, queries, fold lanes, n + 1 words each][per proof: samples, gamma table, betas, layer table][per proof: its
// words][flags: hash jobs | layer-0 waves | fold lanes].  Everything before the flags is the one upload.  Only the 'ZKLD' / 'ZKEV' / 'ZKBE' words go up: of a 'ZKSR' proof
// the embedded evaluation proof, never the program, the cells or the tapes in front of it.
//
// UNTRUSTED INPUT.  The stage runs after checks 1 and 3 of every proof: its length is EXACTLY what its header states and every word is below p.  The query section has a
// fixed stride, so every offset and extent is a function of the checked header alone (run() recomputes the stride and refuses a description whose sections do not add up to
// the length); the row a job reads its Merkle index from is the transcript's sample, never the proof's index word, which only the host compares (check 6).
namespace {

// One proof's shape, DEVICE MEMORY.  Offsets of the proof's words are counted from its first word, which stands at word `base` of the block.
struct PcsManyShape {
  uint64_t base;
  uint32_t o_qs, o_gamma, o_betas, o_ltab;                       // the proof's tables, words of the block
  uint32_t at_queries, qsize, at_fin;
  uint32_t n_layers, n_slots, log_M, fin_mask, n_points, n_sel, wM_m, lay0_off;
  uint32_t leaf_off[PCS_MAX_SLOTS], leaf_words[PCS_MAX_SLOTS], depth[PCS_MAX_SLOTS], root_at[PCS_MAX_SLOTS], idx_add[PCS_MAX_SLOTS];
  uint32_t widths[zkir::PCS_MAX_MATS], rec_off[zkir::PCS_MAX_MATS];      // the record at q (the one at q + M/2 follows it, widths[m] + 4 log_M words on)
  uint32_t sel_point[zkir::PCS_MAX_SEL], sel_mat[zkir::PCS_MAX_SEL], sel_e0[zkir::PCS_MAX_SEL];
  uint32_t z_m[2][4], a_m[2][4];
};

// A row of 16 lanes per leaf-and-path job; job -> (proof i, query t, slot).  flags[job] = 0 / 1.
__global__ __launch_bounds__(NT_MV) void pcs_hash_jobs_many_kernel(const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ blk, const PcsManyShape* __restrict__ shapes,
                                                                   const uint32_t* __restrict__ hj, uint32_t n, uint32_t n_jobs, uint32_t* __restrict__ flags) {
  const uint32_t job = (blockIdx.x * NT_MV + threadIdx.x) / 16;
  const uint32_t l = threadIdx.x & 15;
  if (job >= n_jobs) return;                                     // (whole rows)
  const uint32_t i = stark_proof_of(hj, n, job);
  const PcsManyShape& sh = shapes[i];
  const uint32_t local = job - hj[i], t = local / sh.n_slots, slot = local - t * sh.n_slots;
  const uint32_t* w = blk + sh.base;
  const uint32_t depth = sh.depth[slot], width = sh.leaf_words[slot];
  const uint32_t j = (blk[sh.o_qs + t] + sh.idx_add[slot]) & ((1u << depth) - 1u);
  const uint32_t* r = w + sh.at_queries + (uint64_t)t * sh.qsize + sh.leaf_off[slot];
  const uint32_t eq = pcs_row16_hashes_to(cp, r, width, depth, j, w + sh.root_at[slot], l);
  if (l == 0) flags[job] = eq ? 0u : 1u;
}

// Workgroups [0, n_waves): a WAVE per (proof, query t, half s2), wave id = 2 (cq[i] + t) + s2 — the layer-0 value at row q + s2 M/2 by the proof's rule against layer 0's
// value s2 (check 8): flags8[wave].  The workgroups behind them: a LANE per (proof, query t, layer j), lane id = fj[i] + t n_layers + j — layer j's own values folded and
// compared with the next layer's v[slot] (check 10 of layer j + 1) or the final layer's value (check 11): flags_fold[lane id].
__global__ __launch_bounds__(64) void pcs_value_many_kernel(const uint32_t* __restrict__ blk, const PcsManyShape* __restrict__ shapes, const uint32_t* __restrict__ cq,
                                                            const uint32_t* __restrict__ fj, uint32_t n, uint32_t n_waves, uint32_t n_folds, uint32_t* __restrict__ flags8,
                                                            uint32_t* __restrict__ flags_fold) {
  const uint32_t lane = threadIdx.x;
  if (blockIdx.x < n_waves) {
    const uint32_t qid = blockIdx.x >> 1, s2 = blockIdx.x & 1u;
    const uint32_t i = stark_proof_of(cq, n, qid);
    const PcsManyShape& sh = shapes[i];
    const uint32_t t = qid - cq[i];
    const uint32_t pos = blk[sh.o_qs + t] + (s2 ? 1u << (sh.log_M - 1) : 0u);
    const uint32_t* qb = blk + sh.base + sh.at_queries + (uint64_t)t * sh.qsize;
    E4 A0 = bb::e_zero(), A1 = bb::e_zero();
    for (uint32_t si = 0; si < sh.n_sel; si++) {
      const uint32_t m = sh.sel_mat[si], width = sh.widths[m];
      const E4 acc = pcs_row_dot(blk + sh.o_gamma + 4 * (uint64_t)sh.sel_e0[si], qb + sh.rec_off[m] + s2 * (width + 4 * sh.log_M), width, lane);
      if (sh.sel_point[si] == 0) A0 = bb::e_add(A0, acc); else A1 = bb::e_add(A1, acc);
    }
    pcs_wave_sum(A0, A1);
    const E4 want = sh.n_points == 0 ? bb::e_to_mont(A0) : pcs_point_sum(sh.n_points, sh.z_m, sh.a_m, A0, A1, sh.wM_m, pos);
    const E4 v = pcs_load_m(qb + sh.lay0_off + 4 * s2);
    if (lane == 0) flags8[blockIdx.x] = pcs_differ(v, want) ? 1u : 0u;
    return;
  }
  const uint32_t id = (blockIdx.x - n_waves) * 64 + lane;
  if (id >= n_folds) return;
  const uint32_t i = stark_proof_of(fj, n, id);
  const PcsManyShape& sh = shapes[i];
  const uint32_t local = id - fj[i], t = local / sh.n_layers, j = local - t * sh.n_layers;
  const uint32_t* w = blk + sh.base;
  const uint32_t* qb = w + sh.at_queries + (uint64_t)t * sh.qsize;
  const uint32_t* L = blk + sh.o_ltab + PCS_LAYER_WORDS * j;
  const uint32_t idx = blk[sh.o_qs + t] & ((1u << L[PCS_L_DEPTH]) - 1u);
  const E4 got = pcs_fold_lane(qb + L[PCS_L_OFF], L, blk + sh.o_betas + 4 * j, idx);
  const uint32_t* nxt = j + 1 < sh.n_layers ? qb + L[PCS_LAYER_WORDS + PCS_L_OFF] + 4 * (idx >> L[PCS_LAYER_WORDS + PCS_L_DEPTH]) : w + sh.at_fin + 4 * (idx & sh.fin_mask);
  flags_fold[id] = pcs_differ(pcs_load_m(nxt), got) ? 1u : 0u;
}

// The device form of the list stage.
struct PcsManyDeviceStage {
  hipStream_t s;
  uint64_t hash_jobs = 0, value_jobs = 0, uploaded_words = 0; uint32_t launches = 0;      // what the run launched (zkir_verify_queries_last)
  int run(const zkir::PcsCollected* list, uint32_t n, int* codes) {
    if (!n) return 0;
    auto refuse = [](const char* m) { zkir::set_last_error({ZKIR_ERR_OTHER, m}); return -(int)ZKIR_ERR_OTHER; };
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_*_many_device: no current HIP device"}); return -ZKIR_ERR_DEVICE; }
    VerifyDevice& V = verify_device(dev);
    std::lock_guard<std::mutex> lock(V.mu);
    V.pin.reset();
    // ---- the shapes and the layout: every offset from the checked header ----
    std::vector<PcsManyShape> shapes(n);
    std::vector<uint32_t> pre(3 * ((size_t)n + 1), 0);
    uint32_t *hj = pre.data(), *cq = hj + n + 1, *fj = cq + n + 1;
    const size_t o_pre = al256((size_t)n * sizeof(PcsManyShape)), o_tab = o_pre + al256(pre.size() * 4);
    size_t at = o_tab / 4;                                       // (words of the block)
    std::vector<uint32_t> ltab((size_t)n * zkir::PCS_MAX_LAYERS * PCS_LAYER_WORDS, 0);
    for (uint32_t i = 0; i < n; i++) {
      const zkir::PcsQueries& Q = list[i].q;
      PcsManyShape& sh = shapes[i];
      memset(&sh, 0, sizeof sh);
      const uint32_t nl = Q.n_layers, nq = Q.num_queries, n_fin = 4u << Q.b;
      if (!list[i].filled || !Q.w || nl < 1 || nl > zkir::PCS_MAX_LAYERS || Q.n_mats < 1 || Q.n_mats > zkir::PCS_MAX_MATS || nq < 1 || nq > 128 || Q.b < 1 || Q.b > 3 || Q.log_M < 2 || Q.log_M > 27 ||
          Q.n_points > 2 || Q.n_sel > zkir::PCS_MAX_SEL || Q.len >> 31 || list[i].qs.size() != nq || list[i].betas_m.size() != 4 * (size_t)nl || list[i].gamma_m.size() != 4 * (size_t)Q.n_gamma ||
          Q.at_roots + 4 * (uint64_t)Q.n_mats > Q.len || Q.at_lroots + 4 * (uint64_t)nl > Q.len || Q.at_fin + 4 * (uint64_t)n_fin > Q.at_queries || Q.at_queries > Q.len) return refuse("zkir_*_many_device: a query description is not a checked proof's");
      hj[i + 1] = hj[i] + nq * (2 * Q.n_mats + nl); cq[i + 1] = cq[i] + nq; fj[i + 1] = fj[i] + nq * nl;
      sh.at_queries = (uint32_t)Q.at_queries; sh.qsize = (uint32_t)Q.qsize; sh.at_fin = (uint32_t)Q.at_fin;
      sh.n_layers = nl; sh.n_slots = 2 * Q.n_mats + nl; sh.log_M = Q.log_M; sh.fin_mask = n_fin - 1u; sh.n_points = Q.n_points;
      uint32_t off = 1;                                          // (the index word)
      for (uint32_t m = 0; m < Q.n_mats; m++) {
        if (Q.widths[m] < 1 || Q.widths[m] > 512) return refuse("zkir_*_many_device: a query description is not a checked proof's");
        sh.widths[m] = Q.widths[m]; sh.rec_off[m] = off;
        for (uint32_t s2 = 0; s2 < 2; s2++) {
          const uint32_t sl = 2 * m + s2;
          sh.leaf_off[sl] = off; sh.leaf_words[sl] = Q.widths[m]; sh.depth[sl] = Q.log_M; sh.root_at[sl] = (uint32_t)Q.at_roots + 4 * m; sh.idx_add[sl] = s2 ? 1u << (Q.log_M - 1) : 0u;
          off += Q.widths[m] + 4 * Q.log_M;
        }
      }
      uint32_t* lt = ltab.data() + (size_t)i * zkir::PCS_MAX_LAYERS * PCS_LAYER_WORDS;
      uint32_t shift = bb::GEN, log_m = Q.log_M;
      for (uint32_t j = 0; j < nl; j++) {
        const uint32_t k = Q.ks[j];
        if (k < 1 || k > 3 || k > log_m) return refuse("zkir_*_many_device: a query description is not a checked proof's");
        const uint32_t depth = log_m - k, sl = 2 * Q.n_mats + j;
        sh.leaf_off[sl] = off; sh.leaf_words[sl] = 4u << k; sh.depth[sl] = depth; sh.root_at[sl] = (uint32_t)Q.at_lroots + 4 * j; sh.idx_add[sl] = 0;
        uint32_t* L = lt + PCS_LAYER_WORDS * j;
        L[PCS_L_OFF] = off; L[PCS_L_K] = k; L[PCS_L_DEPTH] = depth; L[PCS_L_LOG_M] = log_m;
        if (j == 0) sh.lay0_off = off;
        for (uint32_t f = 0; f < k; f++) {
          L[PCS_L_INV2SHIFT + f] = bb::to_mont(bb::inv(bb::mul(2, shift))); L[PCS_L_WM + f] = bb::to_mont(bb::root_of_unity((int)log_m));
          shift = bb::mul(shift, shift); log_m--;
        }
        off += (4u << k) + 4 * depth;
      }
      if (off != Q.qsize || Q.at_queries + (uint64_t)nq * Q.qsize != Q.len) return refuse("zkir_*_many_device: the query section is not the header's");
      // the layer-0 rule as data (n_points = 0: one selected pair, the plain sum over matrix 0); every selection stays inside the gamma table
      if (Q.n_points == 0) { sh.n_sel = 1; if (Q.n_gamma < Q.widths[0]) return refuse("zkir_*_many_device: a query description is not a checked proof's"); }
      else {
        sh.n_sel = Q.n_sel;
        for (uint32_t k = 0; k < Q.n_sel; k++) {
          if (Q.sel[k].point >= Q.n_points || Q.sel[k].mat >= Q.n_mats || (uint64_t)Q.sel[k].e0 + Q.widths[Q.sel[k].mat] > Q.n_gamma) return refuse("zkir_*_many_device: a query description is not a checked proof's");
          sh.sel_point[k] = Q.sel[k].point; sh.sel_mat[k] = Q.sel[k].mat; sh.sel_e0[k] = Q.sel[k].e0;
        }
        memcpy(sh.z_m, Q.z_m, sizeof sh.z_m); memcpy(sh.a_m, Q.a_m, sizeof sh.a_m);
        sh.wM_m = bb::to_mont(bb::root_of_unity((int)Q.log_M));
      }
      sh.o_qs = (uint32_t)at; at += (nq + 3) & ~3u;
      sh.o_gamma = (uint32_t)at; at += list[i].gamma_m.size();
      sh.o_betas = (uint32_t)at; at += 4 * (size_t)nl;
      sh.o_ltab = (uint32_t)at; at += ((size_t)nl * PCS_LAYER_WORDS + 3) & ~(size_t)3;
      if (at >> 31) return refuse("zkir_*_many_device: the batch's tables are too large");
    }
    const size_t o_words = al256(at * 4);
    at = o_words / 4;
    for (uint32_t i = 0; i < n; i++) { shapes[i].base = at; at += (size_t)((list[i].q.len + 3) & ~(uint64_t)3); }
    const uint64_t n_hash = hj[n], n_q = cq[n], n_fold = fj[n];
    if ((n_hash * 16) >> 31) return refuse("zkir_*_many_device: too many jobs for one batch");
    const size_t o_flags = al256(at * 4), n_flags = (size_t)(n_hash + 2 * n_q + n_fold), total = o_flags + al256(n_flags * 4);
    // ---- one staged upload ----
    const int erc = V.ensure(total);
    if (erc) return -erc;
    unsigned char* h = (unsigned char*)V.pin.take(o_flags);
    uint32_t* h_flags = V.pin.take_n<uint32_t>(n_flags);
    if (!h || !h_flags) { zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_*_many_device: no pinned host memory"}); return -ZKIR_ERR_DEVICE; }
    memcpy(h, shapes.data(), (size_t)n * sizeof(PcsManyShape)); memcpy(h + o_pre, pre.data(), pre.size() * 4);
    uint32_t* hw = (uint32_t*)h;
    for (uint32_t i = 0; i < n; i++) {
      const zkir::PcsCollected& C = list[i]; const PcsManyShape& sh = shapes[i];
      memcpy(hw + sh.o_qs, C.qs.data(), C.qs.size() * 4); memcpy(hw + sh.o_gamma, C.gamma_m.data(), C.gamma_m.size() * 4); memcpy(hw + sh.o_betas, C.betas_m.data(), C.betas_m.size() * 4);
      memcpy(hw + sh.o_ltab, ltab.data() + (size_t)i * zkir::PCS_MAX_LAYERS * PCS_LAYER_WORDS, (size_t)C.q.n_layers * PCS_LAYER_WORDS * 4);
      memcpy(hw + sh.base, C.q.w, (size_t)C.q.len * 4);
    }
    if (hipMemcpyAsync(V.d, h, o_flags, hipMemcpyHostToDevice, s) != hipSuccess) { (void)check_launch("zkir_*_many_device: upload"); return -ZKIR_ERR_DEVICE; }
    // ---- two launches ----
    const uint32_t* d_blk = (const uint32_t*)V.d; const PcsManyShape* d_shapes = (const PcsManyShape*)V.d;
    const uint32_t *d_hj = (const uint32_t*)(V.d + o_pre), *d_cq = d_hj + n + 1, *d_fj = d_cq + n + 1;
    uint32_t* d_flags = (uint32_t*)(V.d + o_flags);
    uint32_t *d_f8 = d_flags + n_hash, *d_ff = d_f8 + 2 * n_q;
    hipLaunchKernelGGL(pcs_hash_jobs_many_kernel, dim3(grid_for(n_hash * 16, NT_MV)), dim3(NT_MV), 0, s, V.d_p2, d_blk, d_shapes, d_hj, n, (uint32_t)n_hash, d_flags);
    hipLaunchKernelGGL(pcs_value_many_kernel, dim3((unsigned)(2 * n_q) + grid_for(n_fold, 64)), dim3(64), 0, s, d_blk, d_shapes, d_cq, d_fj, n, (uint32_t)(2 * n_q), (uint32_t)n_fold, d_f8, d_ff);
    hash_jobs = n_hash; value_jobs = 2 * n_q + n_fold; launches = 2; uploaded_words = o_flags / 4;
    // ---- one download, one synchronisation ----
    if (hipMemcpyAsync(h_flags, d_flags, n_flags * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess || check_launch("zkir_*_many_device: query stage") != ZKIR_OK) {
      (void)check_launch("zkir_*_many_device: query stage"); return -ZKIR_ERR_DEVICE;
    }
    for (uint32_t i = 0; i < n; i++) codes[i] = pcs_resolve(list[i].q, h_flags + hj[i], h_flags + n_hash + 2 * (size_t)cq[i], h_flags + n_hash + 2 * n_q + fj[i]);
    return 0;
  }
  void note() const { zkir::verify_note_queries(hash_jobs, value_jobs, launches, uploaded_words); }
};
int pcs_many_device_run(void* p, const zkir::PcsCollected* list, uint32_t n, int* codes) { return guarded([&] { return static_cast<PcsManyDeviceStage*>(p)->run(list, n, codes); }); }

int pcs_many_refuse(const char* m) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, m}); return ZKIR_ERR_ARGUMENT; }

// What zkir_verify_rate_many_device and zkir_pcs_verify_many_device share: front(i, stage) runs proof i's host front with the collecting stage and answers its verdict so far
// (negative: no verdict for the call); then one stage run over the proofs that reached their queries; `lift` turns a query code into the entry's (100 + c for a 'ZKSR' proof).
template <typename Front>
int pcs_many_verify(uint32_t n, int32_t* verdicts, void* stream, int lift, Front front) {
  return guarded([&]() -> int {
    std::vector<int32_t> out(n, 0);
    std::vector<zkir::PcsCollected> list(n);
    std::vector<uint32_t> who;
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; i++) {
      list[k] = zkir::PcsCollected{};
      const int rc = front(i, zkir::pcs_collect_stage(&list[k]));
      if (rc < 0) return rc;
      out[i] = rc;
      if (!rc && !list[k].filled) { zkir::set_last_error({ZKIR_ERR_OTHER, "zkir_*_many_device: a front accepted a proof without reaching its queries"}); return -(int)ZKIR_ERR_OTHER; }
      if (!rc) { who.push_back(i); k++; }
    }
    PcsManyDeviceStage st{(hipStream_t)stream};
    std::vector<int> codes((size_t)k + 1, 0);
    if (k) { const int src = st.run(list.data(), k, codes.data()); if (src) return src; }      // (no proof reached its queries: nothing is launched)
    st.note();
    for (uint32_t j = 0; j < k; j++) out[who[j]] = codes[j] ? lift + codes[j] : 0;
    memcpy(verdicts, out.data(), (size_t)n * sizeof(int32_t));
    return 0;
  });
}

}  // namespace

extern "C" {

int zkir_verify_rate_segment_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits, uint32_t first_state[68],
                                    uint32_t last_state[68], void* stream) {
  uint32_t st[2 * 68];
  int32_t verdict = 0;
  const int rc = pcs_many_verify(1, &verdict, stream, 100, [&](uint32_t, const zkir::QueryStage& collect) {
    return zkir::rate_segment_verify_with_stage(proof, proof_words, expect, min_queries, min_pow_bits, collect, st, nullptr);
  });
  zkir::verify_note_device_stages(0);
  if (rc) return rc > 0 ? -rc : rc;                              // (a batch of one has no argument of its own to refuse: whatever fails here is no verdict)
  if (verdict == 0) { if (first_state) memcpy(first_state, st, sizeof st / 2); if (last_state) memcpy(last_state, st + 68, sizeof st / 2); }
  return verdict;
}

int zkir_verify_rate_chain_device(const uint32_t* const* proofs, const uint64_t* proof_words, uint32_t n_segments, const zkir_public_inputs* expect, uint32_t min_queries,
                                  uint32_t min_pow_bits, void* stream) {
  if (proofs && proof_words && n_segments == 1 && proofs[0] && proof_words[0] > 9 && proofs[0][9] >= 3) return zkir_verify_rate_device(proofs[0], proof_words[0], expect, min_queries, min_pow_bits, stream);      // a whole run by itself
  PcsManyDeviceStage st{(hipStream_t)stream};
  const int rc = guarded([&] { return zkir::rate_chain_with_stage(proofs, proof_words, n_segments, expect, min_queries, min_pow_bits, zkir::PcsManyStage{&st, pcs_many_device_run}); });
  zkir::verify_note_device_stages(0);
  if (rc >= 0) st.note();
  return rc;
}

int zkir_verify_rate_many_device(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, const uint32_t* min_queries,
                                 const uint32_t* min_pow_bits, uint32_t n, int32_t* verdicts, void* stream) {
  if (!proofs || !proof_words || !verdicts) return pcs_many_refuse("zkir_verify_rate_many_device: null proofs, proof_words or verdicts");
  if (n < 1 || n > 1024) return pcs_many_refuse("zkir_verify_rate_many_device: n must be 1 .. 1024");
  uint32_t stages_total = 0;
  const int rc = pcs_many_verify(n, verdicts, stream, 100, [&](uint32_t i, const zkir::QueryStage& collect) -> int {
    const uint32_t* w = proofs[i]; const uint64_t len = proof_words[i];
    const zkir_public_inputs* expect = expects ? expects[i] : nullptr;
    const uint32_t mq = min_queries ? min_queries[i] : 1u, mb = min_pow_bits ? min_pow_bits[i] : 0u;
    if (!w || len < 10 || w[9] != 4) return zkir::rate_verify_with_stage(w, len, expect, mq, mb, collect);
    // mode 4: the three tape stages on the device as in zkir_verify_rate_device, under the device state's mutex for this proof's front (a description owns its draws, so
    // the staging the tape stages leave behind is free for the next proof and for the shared query stage)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_verify_rate_many_device: no current HIP device"}); return -ZKIR_ERR_DEVICE; }
    VerifyDevice& V = verify_device(dev);
    std::lock_guard<std::mutex> lock(V.mu);
    V.pin.reset();
    DeviceTapes dt(V, (hipStream_t)stream);
    const zkir::TapeStages tapes{&dt, dt_hash_check, dt_wide_check, dt_digests, dt_hash_side, dt_wide_side};
    const int frc = zkir::rate_verify_with_stage(w, len, expect, mq, mb, collect, &tapes);
    if (dt.stages_run) (void)hipStreamSynchronize((hipStream_t)stream);      // (a verdict reached before a stage's own synchronisation: nothing of this proof stays in flight)
    stages_total += dt.stages_run;
    return frc;
  });
  zkir::verify_note_device_stages(stages_total);
  return rc;
}

int zkir_pcs_verify_many_device(const uint32_t* kinds, const uint32_t* const* proofs, const uint64_t* proof_words, const uint32_t* const* expect_roots, const uint32_t* const* expect_points,
                                const uint32_t* const* expect_evals, uint32_t n, int32_t* verdicts, void* stream) {
  if (!kinds || !proofs || !proof_words || !verdicts) return pcs_many_refuse("zkir_pcs_verify_many_device: null kinds, proofs, proof_words or verdicts");
  if (n < 1 || n > 1024) return pcs_many_refuse("zkir_pcs_verify_many_device: n must be 1 .. 1024");
  for (uint32_t i = 0; i < n; i++) if (kinds[i] > 2) return pcs_many_refuse("zkir_pcs_verify_many_device: a kind must be 0 ('ZKLD'), 1 ('ZKEV') or 2 ('ZKBE')");
  const int rc = pcs_many_verify(n, verdicts, stream, 0, [&](uint32_t i, const zkir::QueryStage& collect) {
    return zkir::pcs_verify_with_stage((int)kinds[i], proofs[i], proof_words[i], expect_roots ? expect_roots[i] : nullptr, expect_points ? expect_points[i] : nullptr,
                                       expect_evals ? expect_evals[i] : nullptr, collect);
  });
  zkir::verify_note_device_stages(0);
  return rc;
}

}  // extern "C"
