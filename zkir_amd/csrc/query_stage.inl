// query_stage.inl — the ONE device form of a verifier's QUERY STAGE (verify_stages.h), shared by pcs_verify.inl, pcs_verify_many.inl, stark_verify.inl and (its __device__
// pieces and its layout builder) mixed_verify.inl.  Included by stark.hip at file scope, after verify_device.inl (whose per-device state it uses) and merkle_open.inl
// (whose row-of-16 chain the hash kernel repeats), ahead of the four files that use it.
//
// A stage run serves n proofs whose SHAPES DIFFER (the kind, log_M, the rate, the matrices and their widths, the points, the selections, the number of queries): the shape
// is a per-proof record in device memory (QueryShape) and a job finds its proof by a binary search in a prefix table the host writes.  A single proof is a batch of one.
// ONE staged upload, TWO launches, one download of the flags, one synchronisation on the caller's stream, however many proofs:
//   query_hash_jobs_kernel   sum_i n_full_i n_slots_i jobs, a row of 16 lanes each: a matrix record's row or a FRI layer's values hashed and walked up to its root
//   query_value_kernel       a wave per (proof, query, half): the layer-0 value by the proof's own rule; a lane per (proof, query, layer): the layer's values folded and
//                            compared with the next layer's word or the final layer
// and the calling stage picks each proof's verdict from the flags in the order its host loop returns it (pcs_resolve, stark_resolve).
//
// THE BLOCK.  [shapes: n QueryShape][prefix tables: hash jobs, queries, fold lanes, n + 1 words each][per proof: samples, gamma table, betas, layer table][per proof: the
// span of its words the stage names][flags: hash jobs | layer-0 waves | fold lanes].  Everything before the flags is the one upload.
//
// UNTRUSTED INPUT — the contract of every stage over this file.  A stage runs after its verifier's word-range check (every uploaded word is below p) and its header
// checks, and describes the query section by CHECKED words alone.  The section has a fixed stride: query_layout recomputes it from the schedule and the matrix records and
// refuses a description whose stride is not the header's, a fold count outside 1 .. 3 or a schedule that does not end on the final layer; a stage checks that the whole
// queries it names lie inside the span it uploads.  So every offset and extent a kernel uses is a function of checked words.  The row a job opens is the transcript's
// sample, never the proof's index word, which only the host compares.  No kernel reads outside the uploaded words, no word >= p is an operand.
namespace {

constexpr uint32_t PCS_MAX_SLOTS = 2 * zkir::PCS_MAX_MATS + zkir::PCS_MAX_LAYERS;      // the hash jobs of one query: 17
static_assert(PCS_MAX_SLOTS >= 2 * zkir::PCS_MAX_MATS + zkir::PCS_MAX_LAYERS && PCS_MAX_SLOTS >= 6 + zkir::PCS_MAX_LAYERS,
              "a record's slots hold a commitment proof's (matrices at two rows, the layers) and a STARK proof's (three matrices at two rows, the layers)");

// ---- the __device__ pieces ----

// merkle_verify_row16_kernel's chain (a SECOND COPY: that kernel's code is left as it is) on a leaf read in place: lane l of a row of 16 holds state word l; link
// t < n_sponge absorbs block t of the leaf r (width words, its 4 depth sibling words behind it), link n_sponge + lvl compresses with the sibling of level lvl of Merkle
// index j.  Scale factors and the ragged-last-block rule are leaf_hash_kernel's.  A leaf has at least one word and every word is canonical, so there is no verdict but
// "hashes to the root" or not: non-zero on the row's lane 0 when it does.
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

// The LAYER TABLE (device memory, PCS_LAYER_WORDS words a layer: a lane picks its layer, and a by-value array indexed per lane would live in scratch): the values' offset
// in a query, k folds, the tree's depth, log2 of the domain the layer starts on, and for fold step f the Montgomery constants 1 / (2 shift) and w (the root of unity of the
// step's domain, order 2^(log_m - f)): 1 / (2 x) for x = shift w^e is their product with w^(2^(log_m - f) - e) — the same field element as the host's Fermat inverse.
// (Word 10 is the mixed stage's: MIXED_L_ADD, mixed_verify.inl.)
constexpr uint32_t PCS_LAYER_WORDS = 12, PCS_L_OFF = 0, PCS_L_K = 1, PCS_L_DEPTH = 2, PCS_L_LOG_M = 3, PCS_L_INV2SHIFT = 4, PCS_L_WM = 7;

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

// The pieces of a layer-0 wave and of a fold lane.
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

// the proof a job belongs to: the largest i < n with prefix[i] <= id (prefix[0] = 0, prefix rising; a proof without jobs has an empty range and is never found)
__device__ __forceinline__ uint32_t query_proof_of(const uint32_t* __restrict__ prefix, uint32_t n, uint32_t id) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (prefix[mid] <= id) lo = mid; else hi = mid; }
  return lo;
}

// ---- the record and the kernel pair ----

// One proof's shape, DEVICE MEMORY.  Offsets of the proof's words are counted from the first UPLOADED word (a commitment proof's first word, a STARK proof's trace root),
// which stands at word `base` of the block.  Slot -> a hash job of a query: a slot below 2 n_mats is matrix slot / 2's record at row q (even) or q + M/2 (odd); the others
// are the FRI layers in order.  leaf_off: words from the query's first word.  The leaf's Merkle index is (q + idx_add) mod 2^depth: the carried index of a FRI layer only
// ever drops high bits of q.  THE LAYER-0 RULE AS DATA (PcsQueries' rule): n_points = 0 is one selected pair (point 0, matrix 0, exponent 0) and the plain sum; a STARK
// proof is 3 matrices, n_points = 2, n_sel = 5.
struct QueryShape {
  uint64_t base;
  uint32_t o_qs, o_gamma, o_betas, o_ltab;                       // the proof's tables, words of the block (the runner's)
  uint32_t at_queries, qsize, at_fin;
  uint32_t n_layers, n_slots, log_M, fin_mask, n_points, n_sel, wM_m, lay0_off;
  uint32_t leaf_off[PCS_MAX_SLOTS], leaf_words[PCS_MAX_SLOTS], depth[PCS_MAX_SLOTS], root_at[PCS_MAX_SLOTS], idx_add[PCS_MAX_SLOTS];
  uint32_t widths[zkir::PCS_MAX_MATS], rec_off[zkir::PCS_MAX_MATS];      // the record at q (the one at q + M/2 follows it, widths[m] + 4 log_M words on)
  uint32_t sel_point[zkir::PCS_MAX_SEL], sel_mat[zkir::PCS_MAX_SEL], sel_e0[zkir::PCS_MAX_SEL];
  uint32_t z_m[2][4], a_m[2][4];
};

// A row of 16 lanes per leaf-and-path job; job -> (proof i, query t, slot).  flags[job] = 0 / 1, one plain store.
__global__ __launch_bounds__(NT_MV) void query_hash_jobs_kernel(const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ blk, const QueryShape* __restrict__ shapes,
                                                                const uint32_t* __restrict__ hj, uint32_t n, uint32_t n_jobs, uint32_t* __restrict__ flags) {
  const uint32_t job = (blockIdx.x * NT_MV + threadIdx.x) / 16;
  const uint32_t l = threadIdx.x & 15;
  if (job >= n_jobs) return;                                     // (whole rows)
  const uint32_t i = query_proof_of(hj, n, job);
  const QueryShape& sh = shapes[i];
  const uint32_t local = job - hj[i], t = local / sh.n_slots, slot = local - t * sh.n_slots;
  const uint32_t* w = blk + sh.base;
  const uint32_t depth = sh.depth[slot], width = sh.leaf_words[slot];
  const uint32_t j = (blk[sh.o_qs + t] + sh.idx_add[slot]) & ((1u << depth) - 1u);
  const uint32_t* r = w + sh.at_queries + (uint64_t)t * sh.qsize + sh.leaf_off[slot];
  const uint32_t eq = pcs_row16_hashes_to(cp, r, width, depth, j, w + sh.root_at[slot], l);
  if (l == 0) flags[job] = eq ? 0u : 1u;
}

// Workgroups [0, n_waves): a WAVE per (proof, query t, half s2), wave id = 2 (cq[i] + t) + s2 — the layer-0 value at row q + s2 M/2 from all the opened rows by the proof's
// rule (lanes over the columns, gamma^e (Montgomery) times the canonical word, exact field sums, a butterfly over the wave, then sum_i (a_i - A_i) / (z_i - x) on every
// lane alike) against layer 0's value s2: flags0[wave].  The workgroups behind them: a LANE per (proof, query t, layer j), lane id = fj[i] + t n_layers + j — layer j's own
// 2^k values folded k times with beta_j and compared with the next layer's v[slot] or, for the last layer, with the final layer's value: flags_fold[lane id].  A fold
// starts from the proof's words, never from a carried value.
__global__ __launch_bounds__(64) void query_value_kernel(const uint32_t* __restrict__ blk, const QueryShape* __restrict__ shapes, const uint32_t* __restrict__ cq,
                                                         const uint32_t* __restrict__ fj, uint32_t n, uint32_t n_waves, uint32_t n_folds, uint32_t* __restrict__ flags0,
                                                         uint32_t* __restrict__ flags_fold) {
  const uint32_t lane = threadIdx.x;
  if (blockIdx.x < n_waves) {
    const uint32_t qid = blockIdx.x >> 1, s2 = blockIdx.x & 1u;
    const uint32_t i = query_proof_of(cq, n, qid);
    const QueryShape& sh = shapes[i];
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
    if (lane == 0) flags0[blockIdx.x] = pcs_differ(v, want) ? 1u : 0u;
    return;
  }
  const uint32_t id = (blockIdx.x - n_waves) * 64 + lane;
  if (id >= n_folds) return;
  const uint32_t i = query_proof_of(fj, n, id);
  const QueryShape& sh = shapes[i];
  const uint32_t local = id - fj[i], t = local / sh.n_layers, j = local - t * sh.n_layers;
  const uint32_t* w = blk + sh.base;
  const uint32_t* qb = w + sh.at_queries + (uint64_t)t * sh.qsize;
  const uint32_t* L = blk + sh.o_ltab + PCS_LAYER_WORDS * j;
  const uint32_t idx = blk[sh.o_qs + t] & ((1u << L[PCS_L_DEPTH]) - 1u);
  const E4 got = pcs_fold_lane(qb + L[PCS_L_OFF], L, blk + sh.o_betas + 4 * j, idx);
  const uint32_t* nxt = j + 1 < sh.n_layers ? qb + L[PCS_LAYER_WORDS + PCS_L_OFF] + 4 * (idx >> L[PCS_LAYER_WORDS + PCS_L_DEPTH]) : w + sh.at_fin + 4 * (idx & sh.fin_mask);
  flags_fold[id] = pcs_differ(pcs_load_m(nxt), got) ? 1u : 0u;
}

// ---- the host builder: what a query's layout is for every stage ----

// A matrix opened in a query: its record is `width` words and a path of `depth` levels under the root at word root_at, once (rows = 1: at q mod 2^depth) or twice
// (rows = 2: at q, then at q + 2^(depth - 1)).  rec_off (out): the first record's offset in a query.
struct QueryMat { uint32_t width, depth, root_at, rows, rec_off; };
// where the builder writes the slots: a record's five arrays (QueryShape's, the mixed stage's by-value shape's)
struct QuerySlots { uint32_t *leaf_off, *leaf_words, *depth, *root_at, *idx_add; };

// The slots of a query that holds its index word, the records of mats[] in order and then the FRI layers of the schedule ks[] (from a domain of 2^log_M down to the final
// layer's 4 << b values, layer roots from word at_lroots on), and the layer table (PCS_LAYER_WORDS words a layer, zeroed first).  Answers nullptr, or why the description
// is not a checked proof's: a fold count outside 1 .. 3 or past the domain, a stride that is not qsize, a schedule that does not end on the final layer.
const char* query_layout(uint32_t log_M, uint32_t b, const uint32_t* ks, uint32_t n_layers, uint32_t at_lroots, QueryMat* mats, uint32_t n_mats, uint64_t qsize, const QuerySlots& S,
                         uint32_t* ltab, uint32_t* lay0_off) {
  uint32_t off = 1, sl = 0;                                      // (the index word)
  for (uint32_t m = 0; m < n_mats; m++) {
    QueryMat& M = mats[m];
    M.rec_off = off;
    for (uint32_t s2 = 0; s2 < M.rows; s2++, sl++) {
      S.leaf_off[sl] = off; S.leaf_words[sl] = M.width; S.depth[sl] = M.depth; S.root_at[sl] = M.root_at; S.idx_add[sl] = s2 ? 1u << (M.depth - 1) : 0u;
      off += M.width + 4 * M.depth;
    }
  }
  memset(ltab, 0, (size_t)n_layers * PCS_LAYER_WORDS * 4);
  uint32_t shift = bb::GEN, log_m = log_M;
  for (uint32_t j = 0; j < n_layers; j++, sl++) {
    const uint32_t k = ks[j];
    if (k < 1 || k > 3 || k > log_m) return "a query description is not a checked proof's";
    const uint32_t depth = log_m - k;
    S.leaf_off[sl] = off; S.leaf_words[sl] = 4u << k; S.depth[sl] = depth; S.root_at[sl] = at_lroots + 4 * j; S.idx_add[sl] = 0;
    uint32_t* L = ltab + PCS_LAYER_WORDS * j;
    L[PCS_L_OFF] = off; L[PCS_L_K] = k; L[PCS_L_DEPTH] = depth; L[PCS_L_LOG_M] = log_m;
    if (j == 0) *lay0_off = off;
    for (uint32_t f = 0; f < k; f++) {
      L[PCS_L_INV2SHIFT + f] = bb::to_mont(bb::inv(bb::mul(2, shift))); L[PCS_L_WM + f] = bb::to_mont(bb::root_of_unity((int)log_m));
      shift = bb::mul(shift, shift); log_m--;
    }
    off += (4u << k) + 4 * depth;
  }
  if (off != qsize || log_m != 2 + b) return "the query section is not the header's";
  return nullptr;
}

// ---- the batch runner ----

int query_refuse(const char* who, const char* what, int code = ZKIR_ERR_OTHER) { zkir::set_last_error({code, std::string(who) + ": " + what}); return -code; }

// One proof of a batch.  The stage fills sh (but for base and o_*, which are the runner's), the layer table and what the runner uploads; the runner hands back the flags.
struct QueryJob {
  QueryShape sh;
  uint32_t ltab[zkir::PCS_MAX_LAYERS * PCS_LAYER_WORDS];
  const uint32_t *qs, *gamma_m, *betas_m;                        // borrowed: n_qs samples, n_gamma and sh.n_layers Montgomery E4
  uint32_t n_qs, n_gamma;
  const uint32_t* words; uint64_t n_words;                       // the span of proof words to upload: sh's offsets count from its first word, the n_full queries lie inside it
  uint32_t n_full;                                               // whole queries: the jobs are over these (0: the proof sends nothing and has no jobs)
  const uint32_t *fh, *f0, *ff;                                  // (out) n_full n_slots hash flags, 2 n_full layer-0 flags, n_full n_layers fold flags
};

// Lays out the block, stages and uploads it, launches the pair, downloads the flags and synchronises.  who: the refusal texts' prefix.  times_env (nullable): the switch
// under which the run synchronises after the upload and after the kernels and keeps host clocks of upload | kernels | download in last_ms.  held: the caller holds the
// device state's mutex already; otherwise the run takes it and KEEPS it while it lives — the flags lie in the device state's pinned staging.
struct QueryRun {
  hipStream_t s; bool held; const char* who; const char* times_env; double* last_ms;
  uint64_t hash_jobs = 0, value_jobs = 0, uploaded_words = 0; uint32_t launches = 0;      // what the run launched
  std::unique_lock<std::mutex> lock;
  int run(QueryJob* jobs, uint32_t n) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return query_refuse(who, "no current HIP device", ZKIR_ERR_DEVICE);
    VerifyDevice& V = verify_device(dev);
    if (!held) lock = std::unique_lock<std::mutex>(V.mu);
    V.pin.reset();                                               // (the tape stages are over by the time the queries run: they keep nothing in the staging or the block)
    auto stage = [&](const char* what) { return std::string(who) + ": " + what; };
    // ---- the layout ----
    std::vector<uint32_t> pre(3 * ((size_t)n + 1), 0);
    uint32_t *hj = pre.data(), *cq = hj + n + 1, *fj = cq + n + 1;
    const size_t o_pre = al256((size_t)n * sizeof(QueryShape)), o_tab = o_pre + al256(pre.size() * 4);
    size_t at = o_tab / 4;                                       // (words of the block)
    for (uint32_t i = 0; i < n; i++) {
      QueryJob& J = jobs[i];
      hj[i + 1] = hj[i] + J.n_full * J.sh.n_slots; cq[i + 1] = cq[i] + J.n_full; fj[i + 1] = fj[i] + J.n_full * J.sh.n_layers;
      J.sh.o_qs = (uint32_t)at; at += (J.n_qs + 3) & ~3u;
      J.sh.o_gamma = (uint32_t)at; at += 4 * (size_t)J.n_gamma;
      J.sh.o_betas = (uint32_t)at; at += 4 * (size_t)J.sh.n_layers;
      J.sh.o_ltab = (uint32_t)at; at += (size_t)J.sh.n_layers * PCS_LAYER_WORDS;
      if (at >> 31) return query_refuse(who, "the batch's tables are too large");
    }
    at = al256(at * 4) / 4;
    for (uint32_t i = 0; i < n; i++) { jobs[i].sh.base = at; at += (size_t)((jobs[i].n_words + 3) & ~(uint64_t)3); }
    const uint64_t n_hash = hj[n], n_q = cq[n], n_fold = fj[n];
    if ((n_hash * 16) >> 31) return query_refuse(who, "too many jobs for one batch");
    if (!n_q) return 0;                                          // (no proof has a whole query: nothing is launched)
    const size_t o_flags = al256(at * 4), n_flags = (size_t)(n_hash + 2 * n_q + n_fold), total = o_flags + al256(n_flags * 4);
    // ---- one staged upload ----
    const bool timed = times_env && getenv(times_env) != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t0 = now();
    const int erc = V.ensure(total);
    if (erc) return -erc;
    unsigned char* h = (unsigned char*)V.pin.take(o_flags);
    uint32_t* h_flags = V.pin.take_n<uint32_t>(n_flags);
    if (!h || !h_flags) return query_refuse(who, "no pinned host memory", ZKIR_ERR_DEVICE);
    memcpy(h + o_pre, pre.data(), pre.size() * 4);
    uint32_t* hw = (uint32_t*)h;
    for (uint32_t i = 0; i < n; i++) {
      const QueryJob& J = jobs[i];
      memcpy(h + (size_t)i * sizeof(QueryShape), &J.sh, sizeof(QueryShape));
      memcpy(hw + J.sh.o_qs, J.qs, (size_t)J.n_qs * 4); memcpy(hw + J.sh.o_gamma, J.gamma_m, (size_t)J.n_gamma * 16); memcpy(hw + J.sh.o_betas, J.betas_m, (size_t)J.sh.n_layers * 16);
      memcpy(hw + J.sh.o_ltab, J.ltab, (size_t)J.sh.n_layers * PCS_LAYER_WORDS * 4);
      if (J.n_words) memcpy(hw + J.sh.base, J.words, (size_t)J.n_words * 4);
    }
    if (hipMemcpyAsync(V.d, h, o_flags, hipMemcpyHostToDevice, s) != hipSuccess) { (void)check_launch(stage("upload").c_str()); return -ZKIR_ERR_DEVICE; }
    if (timed && hipStreamSynchronize(s) != hipSuccess) return -ZKIR_ERR_DEVICE;
    const auto t1 = now();
    // ---- two launches ----
    const uint32_t* d_blk = (const uint32_t*)V.d; const QueryShape* d_shapes = (const QueryShape*)V.d;
    const uint32_t *d_hj = (const uint32_t*)(V.d + o_pre), *d_cq = d_hj + n + 1, *d_fj = d_cq + n + 1;
    uint32_t* d_flags = (uint32_t*)(V.d + o_flags);
    uint32_t *d_f0 = d_flags + n_hash, *d_ff = d_f0 + 2 * n_q;
    hipLaunchKernelGGL(query_hash_jobs_kernel, dim3(grid_for(n_hash * 16, NT_MV)), dim3(NT_MV), 0, s, V.d_p2, d_blk, d_shapes, d_hj, n, (uint32_t)n_hash, d_flags);
    hipLaunchKernelGGL(query_value_kernel, dim3((unsigned)(2 * n_q) + grid_for(n_fold, 64)), dim3(64), 0, s, d_blk, d_shapes, d_cq, d_fj, n, (uint32_t)(2 * n_q), (uint32_t)n_fold, d_f0, d_ff);
    hash_jobs = n_hash; value_jobs = 2 * n_q + n_fold; launches = 2; uploaded_words = o_flags / 4;
    if (timed && hipStreamSynchronize(s) != hipSuccess) { (void)check_launch(stage("kernels").c_str()); return -ZKIR_ERR_DEVICE; }
    const auto t2 = now();
    // ---- one download, one synchronisation ----
    if (hipMemcpyAsync(h_flags, d_flags, n_flags * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess || check_launch(stage("query stage").c_str()) != ZKIR_OK) {
      (void)check_launch(stage("query stage").c_str()); return -ZKIR_ERR_DEVICE;
    }
    const auto t3 = now();
    if (timed) { last_ms[0] = ms(t0, t1); last_ms[1] = ms(t1, t2); last_ms[2] = ms(t2, t3); }
    for (uint32_t i = 0; i < n; i++) { jobs[i].fh = h_flags + hj[i]; jobs[i].f0 = h_flags + n_hash + 2 * (size_t)cq[i]; jobs[i].ff = h_flags + n_hash + 2 * n_q + fj[i]; }
    return 0;
  }
};

}  // namespace
