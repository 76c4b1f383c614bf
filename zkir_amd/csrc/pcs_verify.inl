// pcs_verify.inl — zkir_lowdeg_verify_device, zkir_eval_verify_device, zkir_batch_eval_verify_device (include/zkir_amd.h): the verifiers of the commitment layer with their
// QUERY STAGE (verify_stages.h: checks 6 .. 11 of all queries) on the device.  Included by stark.hip at file scope, after verify_device.inl (whose per-device state it uses)
// and merkle_open.inl (whose row-of-16 chain the hash kernel repeats).  The kernels'
// __device__ pieces (pcs_row16_hashes_to, pcs_row_dot, pcs_wave_sum, pcs_point_sum, pcs_fold_step, pcs_fold_lane) are shared with stark_verify.inl.
//
// Everything before the stage — shape, expectations, word range, the whole transcript, the final-degree check, grinding, the sampling — is verify.cpp's host code, run
// first and unchanged.  The stage uploads the proof as it stands with the transcript's samples and the gamma table, launches TWO kernels and downloads one flag per job:
//   pcs_hash_jobs_kernel   num_queries (2 n_mats + n_layers) jobs, a row of 16 lanes each: a leaf (a matrix record's row, a FRI layer's values) hashed and walked up to its root
//   pcs_value_kernel       per query two layer-0 values (a wave each: lanes over the columns) and one fold per layer (a lane each), compared with the proof's own words
// and the host picks the verdict in the order the host loop returns it (pcs_resolve).
//
// UNTRUSTED INPUT.  The stage runs after checks 1 and 3: the proof's length is EXACTLY what its header states and every word is below p.  The query section has a fixed
// stride, so every offset and extent below is a function of the checked header alone; the row a job reads its Merkle index from is the transcript's sample (below M / 2 by
// construction), never the proof's index word, which only the host compares (check 6).  No kernel reads outside the uploaded words, no word >= p is an operand.
namespace {

constexpr uint32_t PCS_MAX_SLOTS = 2 * zkir::PCS_MAX_MATS + zkir::PCS_MAX_LAYERS;      // the hash jobs of one query: 17

// Job -> (query t, slot): a slot below 2 n_mats is matrix slot / 2's record at row q (even) or q + M/2 (odd); the others are the FRI layers in order.  Offsets are words from
// the query's first word.  The leaf's Merkle index is (q + idx_add) mod 2^depth: the carried index of a FRI layer only ever drops high bits of q.
// (SLOTS: the most slots a query of the proof's kind can have — PCS_MAX_SLOTS here, zkir::MIXED_MAX_SLOTS in mixed_verify.inl, whose slot order is its own.)
template <uint32_t SLOTS> struct PcsHashShapeT {
  uint64_t at_queries, qsize;
  uint32_t n_slots, n_jobs;
  uint32_t leaf_off[SLOTS], leaf_words[SLOTS], depth[SLOTS], root_at[SLOTS], idx_add[SLOTS];
};
using PcsHashShape = PcsHashShapeT<PCS_MAX_SLOTS>;

// merkle_verify_row16_kernel's chain (a SECOND COPY: that kernel's code is left as it is) on a leaf read in place: lane l of a row of 16 holds state word l; link
// t < n_sponge absorbs block t of the leaf r (width words, its 4 depth sibling words behind it), link n_sponge + lvl compresses with the sibling of level lvl of Merkle
// index j.  Scale factors and the ragged-last-block rule are leaf_hash_kernel's.  A leaf has at least one word and every word is canonical, so there is no verdict but
// "hashes to the root" or not: non-zero on the row's lane 0 when it does.  Shared by pcs_hash_jobs_kernel and stark_hash_jobs_kernel (stark_verify.inl).
__device__ __forceinline__ uint32_t pcs_row16_hashes_to(const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ r, uint32_t width, uint32_t depth, uint32_t j, const uint32_t* __restrict__ root,
                                                        uint32_t l) {
  const uint32_t* path = r + width;
  const uint32_t k_in = cp->in_scale, carry = cp->carry, out_scale = cp->out_scale;
  const uint32_t q = l & 3;
  const uint32_t root_q = root[q];
  const uint32_t n_sponge = (width + p2::RATE - 1) / p2::RATE, n_links = n_sponge + depth;
  uint32_t s = 0;
  for (uint32_t lk = 0; lk < n_links; lk++) {
    if (lk < n_sponge) {
      const uint32_t off = lk * p2::RATE;
      s = (l < (uint32_t)p2::RATE && off + l < width) ? bb::mont_mul_lazy(r[off + l], k_in) : bb::mont_mul_lazy(s, carry);
    } else {
      const uint32_t lvl = lk - n_sponge, right = (j >> lvl) & 1u;
      const uint32_t from = (uint32_t)__shfl((int)s, (int)q, 16);            // the node's word q (lanes 0-3 of the last output), on every lane
      const uint32_t nd = bb::mont_mul_lazy(from, carry);
      const uint32_t sib = bb::mont_mul_lazy(path[4 * lvl + q], k_in);
      s = l >= 8 ? 0u : ((l >> 2) == right ? nd : sib);          // lanes 0-3 = left child, 4-7 = right child
    }
    s = p2::permute_row16_scaled(s, (int)l, *cp);
  }
  uint32_t eq = bb::mont_mul(s, out_scale) == root_q;            // "my word of the digest is the root's" (lanes 0-3 count)
  eq &= (uint32_t)__shfl_xor((int)eq, 1, 16); eq &= (uint32_t)__shfl_xor((int)eq, 2, 16);
  return eq;
}

// One leaf-and-path job a row of 16 lanes: flags[job] = 0 / 1, one plain store.
template <uint32_t SLOTS>
__global__ __launch_bounds__(NT_MV) void pcs_hash_jobs_kernel(const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ w, const uint32_t* __restrict__ qs, PcsHashShapeT<SLOTS> sh, uint32_t* __restrict__ flags) {
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

// What pcs_value_kernel needs of PcsQueries (verify_stages.h), by value.  n_points = 0: one selected pair (point 0, matrix 0, exponent 0) and the value is the plain sum.
// The LAYER TABLE (device memory, PCS_LAYER_WORDS words a layer: a lane picks its layer, and a by-value array indexed per lane would live in scratch): the values' offset
// in a query, k folds, the tree's depth, log2 of the domain the layer starts on, and for fold step f the Montgomery constants 1 / (2 shift) and w (the root of unity of the
// step's domain, order 2^(log_m - f)): 1 / (2 x) for x = shift w^e is their product with w^(2^(log_m - f) - e) — the same field element as the host's Fermat inverse.
constexpr uint32_t PCS_LAYER_WORDS = 12, PCS_L_OFF = 0, PCS_L_K = 1, PCS_L_DEPTH = 2, PCS_L_LOG_M = 3, PCS_L_INV2SHIFT = 4, PCS_L_WM = 7;
struct PcsValueShape {
  uint64_t at_queries, qsize, at_fin;
  uint32_t n_layers, num_queries, log_M, fin_mask, n_points, n_sel;
  uint32_t widths[zkir::PCS_MAX_MATS], rec_off[zkir::PCS_MAX_MATS];
  uint32_t sel_point[zkir::PCS_MAX_SEL], sel_mat[zkir::PCS_MAX_SEL], sel_e0[zkir::PCS_MAX_SEL];
  uint32_t z_m[2][4], a_m[2][4];
  uint32_t wM_m;
  uint32_t lay0_off;                                             // layer 0's values in a query
};

__device__ __forceinline__ uint32_t pcs_pow_m(uint32_t base_m, uint32_t e) {      // Montgomery in and out
  uint32_t r = bb::R1;
  while (e) { if (e & 1u) r = bb::mont_mul(r, base_m); base_m = bb::mont_mul(base_m, base_m); e >>= 1; }
  return r;
}
__device__ __forceinline__ E4 pcs_load_m(const uint32_t* at) { return bb::e_to_mont(E4{{at[0], at[1], at[2], at[3]}}); }      // proof words -> Montgomery E4
__device__ __forceinline__ uint32_t pcs_differ(const E4& a, const E4& b) { return (a.c[0] ^ b.c[0]) | (a.c[1] ^ b.c[1]) | (a.c[2] ^ b.c[2]) | (a.c[3] ^ b.c[3]); }

// fold step F of a layer whose value t2 rests at position t2 << sl of eight: position p is paired with p + (4 >> F); beta is squared for the next step
template <uint32_t F>
__device__ __forceinline__ void pcs_fold_step(E4 (&v)[8], E4& beta, const uint32_t* __restrict__ L, uint32_t log_m, uint32_t idx, uint32_t sl, uint32_t depth) {
  const uint32_t half_m = bb::to_mont((bb::P + 1) / 2);
  const uint32_t lm = log_m - F, inv2shift = L[PCS_L_INV2SHIFT + F], wm = L[PCS_L_WM + F];
#pragma unroll
  for (uint32_t p = 0; p < (4u >> F); p++) {
    if ((p & ((1u << sl) - 1u)) == 0) {
      const uint32_t e = idx + ((p >> sl) << depth);             // x = shift w^e, e < 2^lm
      const uint32_t inv2x = bb::mont_mul(inv2shift, pcs_pow_m(wm, ((1u << lm) - e) & ((1u << lm) - 1u)));
      const E4 a = v[p], b = v[p + (4u >> F)];
      v[p] = bb::e_add(bb::e_mul_fm(bb::e_add(a, b), half_m), bb::e_mul_m(beta, bb::e_mul_fm(bb::e_sub(a, b), inv2x)));      // (a + b) / 2 + beta (a - b) / (2 x)
    }
  }
  beta = bb::e_mul_m(beta, beta);
}

// The pieces of a layer-0 wave and of a fold lane, shared by pcs_value_kernel and stark_value_kernel (stark_verify.inl).
// sum_k gamma^(e0 + k) row[k] (g: the gamma table at e0, Montgomery; row: canonical words), lanes over the columns: this lane's share
__device__ __forceinline__ E4 pcs_row_dot(const uint32_t* __restrict__ g, const uint32_t* __restrict__ row, uint32_t width, uint32_t lane) {
  E4 acc = bb::e_zero();
  for (uint32_t k = lane; k < width; k += 64) acc = bb::e_add(acc, bb::e_mul_fm(E4{{g[4 * k], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3]}}, row[k]));
  return acc;
}
// exact field sums over the wave (any order gives the same words): a butterfly, every lane ends with both totals
__device__ __forceinline__ void pcs_wave_sum(E4& A0, E4& A1) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      A0.c[c] = bb::add(A0.c[c], (uint32_t)__shfl_xor((int)A0.c[c], d, 64));
      A1.c[c] = bb::add(A1.c[c], (uint32_t)__shfl_xor((int)A1.c[c], d, 64));
    }
}
// sum_i (a_i - A_i) / (z_i - x) over n_points <= 2 points, x = 31 w_M^pos (wM_m: Montgomery); A_i canonical-scaled sums as pcs_row_dot leaves them; z_m, a_m Montgomery
__device__ __forceinline__ E4 pcs_point_sum(uint32_t n_points, const uint32_t (*z_m)[4], const uint32_t (*a_m)[4], const E4& A0, const E4& A1, uint32_t wM_m, uint32_t pos) {
  const uint32_t x_m = bb::mont_mul(bb::to_mont(bb::GEN), pcs_pow_m(wM_m, pos));      // x = 31 w_M^pos
  E4 want = bb::e_zero();
#pragma unroll
  for (uint32_t i = 0; i < 2; i++) {
    if (i >= n_points) break;
    E4 d{{z_m[i][0], z_m[i][1], z_m[i][2], z_m[i][3]}};
    const E4 a{{a_m[i][0], a_m[i][1], a_m[i][2], a_m[i][3]}};
    d.c[0] = bb::sub(d.c[0], x_m);
    want = bb::e_add(want, bb::e_mul_m(bb::e_sub(a, bb::e_to_mont(i ? A1 : A0)), bb::e_inv_m(d)));
  }
  return want;
}
// A layer's own 2^k values (at vals, proof words) folded k times with beta (Montgomery words at beta_at), L: the layer's row of the layer table, idx: the carried index
// below 2^depth.  Value t2 of the 2^k rests at position t2 << (3 - k) of eight: fold step f then pairs position p with p + (4 >> f), whatever k is (register indices only).
__device__ __forceinline__ E4 pcs_fold_lane(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ L, const uint32_t* __restrict__ beta_at, uint32_t idx) {
  const uint32_t k = L[PCS_L_K], depth = L[PCS_L_DEPTH], log_m = L[PCS_L_LOG_M];
  const uint32_t sl = 3 - k;
  E4 v[8];
#pragma unroll
  for (uint32_t p = 0; p < 8; p++) v[p] = (p & ((1u << sl) - 1u)) == 0 ? pcs_load_m(vals + 4 * (p >> sl)) : bb::e_zero();
  E4 beta{{beta_at[0], beta_at[1], beta_at[2], beta_at[3]}};
  if (k > 0) pcs_fold_step<0>(v, beta, L, log_m, idx, sl, depth);
  if (k > 1) pcs_fold_step<1>(v, beta, L, log_m, idx, sl, depth);
  if (k > 2) pcs_fold_step<2>(v, beta, L, log_m, idx, sl, depth);
  return v[0];
}

// Workgroups [0, 2 num_queries): one WAVE per (query t, half s2) — the layer-0 value at row q + s2 M/2 from all the opened rows: lanes over the columns, gamma^e (Montgomery)
// times the canonical word, exact field sums, a butterfly over the wave; then sum_i (a_i - A_i) / (z_i - x) on every lane alike and the comparison with layer 0's value s2
// (check 8): flags8[2 t + s2].
// The workgroups behind them: one LANE per (query t, layer j) — layer j's own 2^k values folded k times with beta_j and compared with the next layer's v[slot] (check 10 of
// layer j + 1) or, for the last layer, with the final layer's value (check 11): flags_fold[t n_layers + j].  A fold starts from the proof's words, never from a carried value.
__global__ __launch_bounds__(64) void pcs_value_kernel(const uint32_t* __restrict__ w, const uint32_t* __restrict__ qs, const uint32_t* __restrict__ gamma_m,
                                                       const uint32_t* __restrict__ betas_m, const uint32_t* __restrict__ ltab, PcsValueShape sh, uint32_t* __restrict__ flags8,
                                                       uint32_t* __restrict__ flags_fold) {
  const uint32_t lane = threadIdx.x;
  if (blockIdx.x < 2 * sh.num_queries) {
    const uint32_t t = blockIdx.x >> 1, s2 = blockIdx.x & 1u;
    const uint32_t pos = qs[t] + (s2 ? 1u << (sh.log_M - 1) : 0u);
    const uint32_t* qb = w + sh.at_queries + (uint64_t)t * sh.qsize;
    E4 A0 = bb::e_zero(), A1 = bb::e_zero();
    for (uint32_t si = 0; si < sh.n_sel; si++) {
      const uint32_t m = sh.sel_mat[si], width = sh.widths[m];
      const E4 acc = pcs_row_dot(gamma_m + 4 * (uint64_t)sh.sel_e0[si], qb + sh.rec_off[m] + s2 * (width + 4 * sh.log_M), width, lane);
      if (sh.sel_point[si] == 0) A0 = bb::e_add(A0, acc); else A1 = bb::e_add(A1, acc);
    }
    pcs_wave_sum(A0, A1);
    const E4 want = sh.n_points == 0 ? bb::e_to_mont(A0) : pcs_point_sum(sh.n_points, sh.z_m, sh.a_m, A0, A1, sh.wM_m, pos);
    const E4 v = pcs_load_m(qb + sh.lay0_off + 4 * s2);
    if (lane == 0) flags8[blockIdx.x] = pcs_differ(v, want) ? 1u : 0u;
    return;
  }
  const uint32_t id = (blockIdx.x - 2 * sh.num_queries) * 64 + lane;
  if (id >= sh.num_queries * sh.n_layers) return;
  const uint32_t t = id / sh.n_layers, j = id - t * sh.n_layers;
  const uint32_t* qb = w + sh.at_queries + (uint64_t)t * sh.qsize;
  const uint32_t* L = ltab + PCS_LAYER_WORDS * j;
  const uint32_t idx = qs[t] & ((1u << L[PCS_L_DEPTH]) - 1u);
  const E4 got = pcs_fold_lane(qb + L[PCS_L_OFF], L, betas_m + 4 * j, idx);
  const uint32_t* nxt = j + 1 < sh.n_layers ? qb + L[PCS_LAYER_WORDS + PCS_L_OFF] + 4 * (idx >> L[PCS_LAYER_WORDS + PCS_L_DEPTH]) : w + sh.at_fin + 4 * (idx & sh.fin_mask);
  flags_fold[id] = pcs_differ(pcs_load_m(nxt), got) ? 1u : 0u;
}

// The verdict of checks 7 .. 11 from the flags, with check 6 from the proof's own index words: for t rising — 6; 7 for matrix 0 row q, matrix 0 row q + M/2, matrix 1 ...;
// 8; per layer j: 9 (j), then 10 (j) for j > 0; 11.  Exactly the order in which verify.cpp's loop returns.
int pcs_resolve(const zkir::PcsQueries& Q, const uint32_t* fh, const uint32_t* f8, const uint32_t* ff) {
  const uint32_t n_slots = 2 * Q.n_mats + Q.n_layers;
  for (uint32_t t = 0; t < Q.num_queries; t++) {
    if (Q.w[Q.at_queries + (uint64_t)t * Q.qsize] != Q.qs[t]) return 6;
    const uint32_t* h = fh + (size_t)t * n_slots;
    for (uint32_t sl = 0; sl < 2 * Q.n_mats; sl++) if (h[sl]) return 7;
    if (f8[2 * t] | f8[2 * t + 1]) return 8;
    for (uint32_t j = 0; j < Q.n_layers; j++) {
      if (h[2 * Q.n_mats + j]) return 9;
      if (j > 0 && ff[(size_t)t * Q.n_layers + j - 1]) return 10;
    }
    if (ff[(size_t)t * Q.n_layers + Q.n_layers - 1]) return 11;
  }
  return 0;
}

thread_local uint64_t pcs_last_jobs[2] = {0, 0};                 // what the calling thread's last *_verify_device call launched (zkir_pcs_verify_last_jobs)

// ZKIR_PCS_VERIFY_TIMES (measurements: scripts/time_pcs_verify.py): the stage synchronises after the upload and after the kernels and keeps host clocks of its parts
thread_local double pcs_last_ms[3] = {0, 0, 0};                  // upload, kernels, download

// The device form of the query stage.  Block: [proof][samples][gamma table][betas][layer table][flags: hash jobs | layer-0 | folds]; ONE staged upload, two launches, one download, one
// synchronisation on the caller's stream.
struct PcsDeviceStage {
  hipStream_t s;
  bool held = false;                                             // the caller holds the device state's mutex already (zkir_verify_rate_device on a mode-4 proof: the tape stages ran under it)
  int run(const zkir::PcsQueries& Q) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_*_verify_device: no current HIP device"}); return -ZKIR_ERR_DEVICE; }
    VerifyDevice& V = verify_device(dev);
    std::unique_lock<std::mutex> lock(V.mu, std::defer_lock);
    if (!held) lock.lock();
    V.pin.reset();                                               // (the tape stages are over by the time the queries run: they keep nothing in the staging or the block)
    const uint32_t nq = Q.num_queries, n_slots = 2 * Q.n_mats + Q.n_layers;
    const uint64_t hash_jobs = (uint64_t)nq * n_slots, value_jobs = (uint64_t)nq * (2 + Q.n_layers);
    const size_t n_flags = (size_t)hash_jobs + (size_t)value_jobs;
    const size_t o_qs = al256(Q.len * 4), o_gamma = o_qs + al256((size_t)nq * 4), o_betas = o_gamma + al256((size_t)Q.n_gamma * 16), o_ltab = o_betas + al256((size_t)Q.n_layers * 16), o_flags = o_ltab + al256((size_t)Q.n_layers * PCS_LAYER_WORDS * 4), total = o_flags + al256(n_flags * 4);
    // ---- the shapes: every offset from the checked header ----
    PcsHashShape hs{};
    PcsValueShape vs{};
    hs.at_queries = vs.at_queries = Q.at_queries; hs.qsize = vs.qsize = Q.qsize; vs.at_fin = Q.at_fin;
    hs.n_slots = n_slots; hs.n_jobs = (uint32_t)hash_jobs;
    vs.n_layers = Q.n_layers; vs.num_queries = nq; vs.log_M = Q.log_M; vs.fin_mask = (4u << Q.b) - 1u; vs.n_points = Q.n_points;
    uint32_t off = 1;                                            // (the index word)
    for (uint32_t m = 0; m < Q.n_mats; m++) {
      vs.widths[m] = Q.widths[m]; vs.rec_off[m] = off;
      for (uint32_t s2 = 0; s2 < 2; s2++) {
        const uint32_t sl = 2 * m + s2;
        hs.leaf_off[sl] = off; hs.leaf_words[sl] = Q.widths[m]; hs.depth[sl] = Q.log_M; hs.root_at[sl] = (uint32_t)Q.at_roots + 4 * m; hs.idx_add[sl] = s2 ? 1u << (Q.log_M - 1) : 0u;
        off += Q.widths[m] + 4 * Q.log_M;
      }
    }
    uint32_t ltab[zkir::PCS_MAX_LAYERS * PCS_LAYER_WORDS] = {0};
    uint32_t shift = bb::GEN, log_m = Q.log_M;
    for (uint32_t j = 0; j < Q.n_layers; j++) {
      const uint32_t k = Q.ks[j], depth = log_m - k, sl = 2 * Q.n_mats + j;
      hs.leaf_off[sl] = off; hs.leaf_words[sl] = 4u << k; hs.depth[sl] = depth; hs.root_at[sl] = (uint32_t)Q.at_lroots + 4 * j; hs.idx_add[sl] = 0;
      uint32_t* L = ltab + PCS_LAYER_WORDS * j;
      L[PCS_L_OFF] = off; L[PCS_L_K] = k; L[PCS_L_DEPTH] = depth; L[PCS_L_LOG_M] = log_m;
      if (j == 0) vs.lay0_off = off;
      for (uint32_t f = 0; f < k; f++) {
        L[PCS_L_INV2SHIFT + f] = bb::to_mont(bb::inv(bb::mul(2, shift))); L[PCS_L_WM + f] = bb::to_mont(bb::root_of_unity((int)log_m));
        shift = bb::mul(shift, shift); log_m--;
      }
      off += (4u << k) + 4 * depth;
    }
    if (off != Q.qsize || Q.at_queries + (uint64_t)nq * Q.qsize != Q.len) { zkir::set_last_error({ZKIR_ERR_OTHER, "zkir_*_verify_device: the query section is not the header's"}); return -ZKIR_ERR_OTHER; }
    if (Q.n_points == 0) { vs.n_sel = 1; vs.sel_point[0] = 0; vs.sel_mat[0] = 0; vs.sel_e0[0] = 0; }
    else {
      vs.n_sel = Q.n_sel;
      for (uint32_t i = 0; i < Q.n_sel; i++) { vs.sel_point[i] = Q.sel[i].point; vs.sel_mat[i] = Q.sel[i].mat; vs.sel_e0[i] = Q.sel[i].e0; }
      memcpy(vs.z_m, Q.z_m, sizeof vs.z_m); memcpy(vs.a_m, Q.a_m, sizeof vs.a_m);
      vs.wM_m = bb::to_mont(bb::root_of_unity((int)Q.log_M));
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
    if (!h || !h_flags) { zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_*_verify_device: no pinned host memory"}); return -ZKIR_ERR_DEVICE; }
    memcpy(h, Q.w, Q.len * 4); memcpy(h + o_qs, Q.qs, (size_t)nq * 4); memcpy(h + o_gamma, Q.gamma_m, (size_t)Q.n_gamma * 16);
    memcpy(h + o_betas, Q.betas_m, (size_t)Q.n_layers * 16); memcpy(h + o_ltab, ltab, (size_t)Q.n_layers * PCS_LAYER_WORDS * 4);
    if (hipMemcpyAsync(V.d, h, o_flags, hipMemcpyHostToDevice, s) != hipSuccess) { (void)check_launch("zkir_*_verify_device: upload"); return -ZKIR_ERR_DEVICE; }
    if (timed && hipStreamSynchronize(s) != hipSuccess) return -ZKIR_ERR_DEVICE;
    const auto t1 = now();
    // ---- two launches ----
    const uint32_t* d_w = (const uint32_t*)V.d; const uint32_t* d_qs = (const uint32_t*)(V.d + o_qs); const uint32_t* d_gamma = (const uint32_t*)(V.d + o_gamma);
    const uint32_t* d_betas = (const uint32_t*)(V.d + o_betas); const uint32_t* d_ltab = (const uint32_t*)(V.d + o_ltab);
    uint32_t* d_flags = (uint32_t*)(V.d + o_flags);
    uint32_t *d_f8 = d_flags + hash_jobs, *d_ff = d_f8 + 2 * (size_t)nq;
    hipLaunchKernelGGL(pcs_hash_jobs_kernel<PCS_MAX_SLOTS>, dim3(grid_for(hash_jobs * 16, NT_MV)), dim3(NT_MV), 0, s, V.d_p2, d_w, d_qs, hs, d_flags);
    hipLaunchKernelGGL(pcs_value_kernel, dim3(2 * nq + grid_for((uint64_t)nq * Q.n_layers, 64)), dim3(64), 0, s, d_w, d_qs, d_gamma, d_betas, d_ltab, vs, d_f8, d_ff);
    pcs_last_jobs[0] = hash_jobs; pcs_last_jobs[1] = value_jobs;
    if (timed && hipStreamSynchronize(s) != hipSuccess) { (void)check_launch("zkir_*_verify_device: kernels"); return -ZKIR_ERR_DEVICE; }
    const auto t2 = now();
    // ---- one download, one synchronisation ----
    if (hipMemcpyAsync(h_flags, d_flags, n_flags * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess || check_launch("zkir_*_verify_device: query stage") != ZKIR_OK) {
      (void)check_launch("zkir_*_verify_device: query stage"); return -ZKIR_ERR_DEVICE;
    }
    const auto t3 = now();
    if (timed) { pcs_last_ms[0] = ms(t0, t1); pcs_last_ms[1] = ms(t1, t2); pcs_last_ms[2] = ms(t2, t3); }
    return pcs_resolve(Q, h_flags, h_flags + hash_jobs, h_flags + hash_jobs + 2 * (size_t)nq);
  }
};
int pcs_device_run(void* p, const zkir::PcsQueries& Q) { return guarded([&] { return static_cast<PcsDeviceStage*>(p)->run(Q); }); }

int pcs_verify_device(int kind, const uint32_t* proof, uint64_t n_words, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals, void* stream) {
  pcs_last_jobs[0] = pcs_last_jobs[1] = 0;
  pcs_last_ms[0] = pcs_last_ms[1] = pcs_last_ms[2] = 0;
  PcsDeviceStage st{(hipStream_t)stream};
  return guarded([&] { return zkir::pcs_verify_with_stage(kind, proof, n_words, expect_roots, expect_points, expect_evals, zkir::QueryStage{&st, pcs_device_run}); });
}

}  // namespace

extern "C" {

int zkir_lowdeg_verify_device(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_root, void* stream) { return pcs_verify_device(0, proof, n_words, expect_root, nullptr, nullptr, stream); }
int zkir_eval_verify_device(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_root, const uint32_t* expect_points, const uint32_t* expect_evals, void* stream) {
  return pcs_verify_device(1, proof, n_words, expect_root, expect_points, expect_evals, stream);
}
int zkir_batch_eval_verify_device(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals, void* stream) {
  return pcs_verify_device(2, proof, n_words, expect_roots, expect_points, expect_evals, stream);
}

// zkir_verify_rate with the embedded evaluation proof's query stage on the device: the same function, the same verdict for every input
int zkir_verify_rate_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits, void* stream) {
  pcs_last_jobs[0] = pcs_last_jobs[1] = 0;
  pcs_last_ms[0] = pcs_last_ms[1] = pcs_last_ms[2] = 0;
  PcsDeviceStage st{(hipStream_t)stream};
  // modes 0 - 3 have no tapes (and a proof too short to name its mode has no verdict that depends on them): the host front, the query stage on the device
  if (!proof || proof_words < 10 || proof[9] != 4) return guarded([&] { return zkir::rate_verify_with_stage(proof, proof_words, expect, min_queries, min_pow_bits, zkir::QueryStage{&st, pcs_device_run}); });
  // mode 4: the three tape stages on the device as in zkir_verify_device (verify_device.inl), under the device state's mutex for the whole call
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_verify_rate_device: no current HIP device"}); return -ZKIR_ERR_DEVICE; }
  VerifyDevice* Vp = nullptr;
  const int src = guarded([&] { Vp = &verify_device(dev); return 0; });
  if (src) return src;
  std::lock_guard<std::mutex> lock(Vp->mu);
  Vp->pin.reset();
  DeviceTapes dt(*Vp, (hipStream_t)stream);
  const zkir::TapeStages tapes{&dt, dt_hash_check, dt_wide_check, dt_digests, dt_hash_side, dt_wide_side};
  st.held = true;
  const int rc = guarded([&] { return zkir::rate_verify_with_stage(proof, proof_words, expect, min_queries, min_pow_bits, zkir::QueryStage{&st, pcs_device_run}, &tapes); });
  if (dt.stages_run) (void)hipStreamSynchronize((hipStream_t)stream);      // (a verdict reached before a stage's own synchronisation: nothing of this call stays in flight)
  zkir::verify_note_device_stages(dt.stages_run);
  return rc;
}

int zkir_pcs_verify_last_jobs(uint64_t* hash_jobs, uint64_t* value_jobs) {
  if (hash_jobs) *hash_jobs = pcs_last_jobs[0];
  if (value_jobs) *value_jobs = pcs_last_jobs[1];
  return ZKIR_OK;
}
int zkir_pcs_verify_last_stage_ms(double ms[3]) {
  if (!ms) return ZKIR_ERR_ARGUMENT;
  for (int k = 0; k < 3; k++) ms[k] = pcs_last_ms[k];
  return ZKIR_OK;
}

}  // extern "C"
