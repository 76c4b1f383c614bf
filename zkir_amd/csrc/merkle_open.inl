// merkle_open.inl — zkir_merkle_open_launch / zkir_merkle_verify_launch (include/zkir_amd.h): open a committed B8 matrix at row indices and check such openings against a root,
// on the device.  Included by stark.hip at file scope, after the Merkle kernels whose trees it reads.
//
// An opening RECORD of a tree with n = 2^d leaves over `width` columns is width + 4 d words: the row's canonical words in column order (the zero padding of a ragged last
// block dropped), then the sibling digest of every level, leaf level first.  In the digest form (ZKIR_OPEN_LEAF_DIGEST: a tree whose leaves are digests, as
// zkir_merkle_cap_launch builds over shard roots) the record is the leaf digest itself, then the path: 4 + 4 d words.  It is the per-position record of a proof's query section
// (verify.cpp: check_query).  Tree layout: level lvl starts at word 4 (2n - (2n >> lvl)), the root is the last four words.
//
// UNTRUSTED INPUT on the verifying side: indices and record words are whatever the caller holds.  An index >= n_leaves reads nothing; a record word >= p is reported before
// any Montgomery product sees it.
namespace {

constexpr uint32_t OPEN_LANES = 16;                              // lanes that share one index in merkle_open_kernel
constexpr int NT_MV = 64;                                        // one wave a workgroup in the verifier: a batch spreads over as many SIMDs as it has waves

// Items of one record: the 16-byte halves of the row's blocks (2 a block), then one 16-byte sibling a level; in the digest form the leaf digest takes the place of the row.
// The OPEN_LANES lanes of an index take the items round-robin: every load is one 16-byte vector (the two halves of a block position by neighbouring lanes: one 32-byte
// sector), every offset 64 bits wide — block b, row j starts at word (b n + j) 8, past 2^32 at 2^25 leaves x 19 blocks.  A record starts at word i (width + 4 d) of `out`,
// 16-byte aligned only when width is a multiple of four: then the stores are 16-byte vectors as well, else four words.
__global__ __launch_bounds__(NT) void merkle_open_kernel(const uint32_t* __restrict__ mat, uint32_t width, uint64_t n, uint32_t depth, const uint32_t* __restrict__ tree, const uint64_t* __restrict__ indices,
                                                         uint64_t n_idx, uint32_t* __restrict__ out) {
  const uint64_t i = ((uint64_t)blockIdx.x * NT + threadIdx.x) / OPEN_LANES;
  const uint32_t l = threadIdx.x % OPEN_LANES;
  if (i >= n_idx) return;
  const bool digest_form = mat == nullptr;
  const uint32_t lead = digest_form ? 4u : width, rec = lead + 4 * depth;
  uint32_t* o = out + i * (uint64_t)rec;
  const uint64_t j = indices[i];
  if (j >= n) {                                                  // nothing is read; the record says so
    for (uint32_t k = l; k < rec; k += OPEN_LANES) o[k] = 0xFFFFFFFFu;
    return;
  }
  const uint4* m4 = reinterpret_cast<const uint4*>(mat);
  const uint4* t4 = reinterpret_cast<const uint4*>(tree);
  const bool vec = (lead & 3) == 0;                              // (rec and lead are then multiples of four, and so is every record's first word)
  const uint32_t n_row = digest_form ? 1u : 2 * ((width + 7) / 8), n_items = n_row + depth;
  for (uint32_t t = l; t < n_items; t += OPEN_LANES) {
    uint4 v; uint32_t at, cnt = 4;
    if (t < n_row) {
      if (digest_form) { v = t4[j]; at = 0; }
      else {
        v = m4[((uint64_t)(t >> 1) * n + j) * 2 + (t & 1)];
        at = 4 * t;                                              // column 8 (t / 2) + 4 (t % 2)
        cnt = width - at < 4 ? width - at : 4;                   // (at < width: t < 2 ceil(width / 8) leaves at most the second half of a ragged block empty — cnt = 0 then)
        if (at >= width) cnt = 0;
      }
    } else {
      const uint32_t lvl = t - n_row;
      v = t4[(2 * n - ((2 * n) >> lvl)) + ((j >> lvl) ^ 1)];
      at = lead + 4 * lvl;
    }
    if (vec && cnt == 4) *reinterpret_cast<uint4*>(o + at) = v;
    else {
      if (cnt > 0) o[at] = v.x;
      if (cnt > 1) o[at + 1] = v.y;
      if (cnt > 2) o[at + 2] = v.z;
      if (cnt > 3) o[at + 3] = v.w;
    }
  }
}

__global__ void merkle_summary_init_kernel(uint32_t* __restrict__ summary) { if (threadIdx.x == 0) { summary[0] = 0; summary[1] = 0xFFFFFFFFu; } }

__device__ __forceinline__ void merkle_verdict_out(uint32_t verdict, uint64_t i, uint32_t* __restrict__ verdicts, uint32_t* __restrict__ summary) {
  verdicts[i] = verdict;
  if (verdict && summary) { atomicAdd(summary, 1u); atomicMin(summary + 1, (uint32_t)i); }
}

// The verifier, one LANE per record (p2::permute_scaled: the fewest instructions a permutation): ceil(width / 8) sponge permutations, then `depth` compressions, one dependent
// chain of ~4250 instructions a link.  Scale factors and the ragged-last-block rule are leaf_hash_kernel's: absorbed words enter with in_scale, words that stay are carried over
// with `carry` — and so is the running node between two compressions, which never takes its canonical form; the last output is brought to canonical words with out_scale and
// compared with the root.  Verdicts: 0 the record hashes to the root, 1 it does not, 2 a word of the record is not canonical (checked over the whole record BEFORE any product:
// mont_mul_lazy's bounds are stated for words below p), 3 the index is not a leaf's.
__global__ __launch_bounds__(NT_MV) void merkle_verify_kernel(const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ root, uint32_t width, uint64_t n, uint32_t depth, const uint64_t* __restrict__ indices,
                                                              uint64_t n_idx, const uint32_t* __restrict__ openings, uint32_t digest_form, uint32_t* __restrict__ verdicts, uint32_t* __restrict__ summary) {
  const uint64_t i = (uint64_t)blockIdx.x * NT_MV + threadIdx.x;
  if (i >= n_idx) return;
  const uint32_t lead = digest_form ? 4u : width, rec = lead + 4 * depth;
  const uint32_t* r = openings + i * (uint64_t)rec;
  const uint64_t j = indices[i];
  if (j >= n) { merkle_verdict_out(3, i, verdicts, summary); return; }
  uint32_t bad = 0;
  for (uint32_t k = 0; k < rec; k++) bad |= r[k] >= bb::P;
  if (bad) { merkle_verdict_out(2, i, verdicts, summary); return; }
  const uint32_t k_in = cp->in_scale, carry = cp->carry, out_scale = cp->out_scale;
  uint32_t s[p2::T], node[4];                                    // node: the running digest as INPUT words (factor F_IN)
  bool ok;
  if (digest_form) {
#pragma unroll
    for (int q = 0; q < 4; q++) node[q] = bb::mont_mul_lazy(r[q], k_in);
    ok = r[0] == root[0] && r[1] == root[1] && r[2] == root[2] && r[3] == root[3];     // (depth 0: the leaf is the root)
  } else {
#pragma unroll
    for (int q = 0; q < p2::T; q++) s[q] = 0;
    for (uint32_t off = 0; off < width; off += p2::RATE) {
#pragma unroll
      for (int q = 0; q < p2::RATE; q++) s[q] = off + q < width ? bb::mont_mul_lazy(r[off + q], k_in) : bb::mont_mul_lazy(s[q], carry);
#pragma unroll
      for (int q = p2::RATE; q < p2::T; q++) s[q] = bb::mont_mul_lazy(s[q], carry);
      p2::permute_scaled(s, *cp);
    }
    if (width == 0) p2::permute_scaled(s, *cp);
    ok = bb::mont_mul(s[0], out_scale) == root[0] && bb::mont_mul(s[1], out_scale) == root[1] && bb::mont_mul(s[2], out_scale) == root[2] && bb::mont_mul(s[3], out_scale) == root[3];
#pragma unroll
    for (int q = 0; q < 4; q++) node[q] = bb::mont_mul_lazy(s[q], carry);
  }
  const uint32_t* path = r + lead;
  for (uint32_t lvl = 0; lvl < depth; lvl++) {
    const bool right = (j >> lvl) & 1;                           // the node is the right child: the sibling goes first
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint32_t sib = bb::mont_mul_lazy(path[4 * lvl + q], k_in);
      s[q] = right ? sib : node[q];
      s[4 + q] = right ? node[q] : sib;
      s[8 + q] = 0;
    }
    p2::permute_scaled(s, *cp);
    if (lvl + 1 == depth) ok = bb::mont_mul(s[0], out_scale) == root[0] && bb::mont_mul(s[1], out_scale) == root[1] && bb::mont_mul(s[2], out_scale) == root[2] && bb::mont_mul(s[3], out_scale) == root[3];
#pragma unroll
    for (int q = 0; q < 4; q++) node[q] = bb::mont_mul_lazy(s[q], carry);
  }
  merkle_verdict_out(ok ? 0u : 1u, i, verdicts, summary);
}

// The same check, one ROW OF 16 LANES per record (p2::permute_row16_scaled: the shortest chain, ~2 us a permutation on a lone wave against ~8): lane l holds state word l, so
// a sponge block is eight lanes' words and a compression puts the node's four words (lanes 0-3 of the previous output) and the sibling's on lanes 0-7.  Sixteen times the lanes
// and about four times the instructions of the lane form: for batches that leave the chip mostly idle.  (One wave a SIMD: the unrolled chain with its constants hoisted takes 256 VGPRs + 28
// AGPRs.  Held to two waves a SIMD — __launch_bounds__(64, 2) — a generation of waves is twice as wide, 224 us instead of 250 at 8192 records, but every chain is slower:
// 133 us instead of 120 for the 50 to 4096 records this form is for.  Not kept.)  All 16 lanes of a row take the same branches (the verdict-2 / 3 decision
// is the row's), which is what the row's DPP sums need.
__global__ __launch_bounds__(NT_MV) void merkle_verify_row16_kernel(const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ root, uint32_t width, uint64_t n, uint32_t depth, const uint64_t* __restrict__ indices,
                                                                    uint64_t n_idx, const uint32_t* __restrict__ openings, uint32_t digest_form, uint32_t* __restrict__ verdicts, uint32_t* __restrict__ summary) {
  const uint64_t i = ((uint64_t)blockIdx.x * NT_MV + threadIdx.x) / 16;
  const uint32_t l = threadIdx.x & 15;
  if (i >= n_idx) return;                                        // (whole rows)
  const uint32_t lead = digest_form ? 4u : width, rec = lead + 4 * depth;
  const uint32_t* r = openings + i * (uint64_t)rec;
  const uint64_t j = indices[i];
  if (j >= n) { if (l == 0) merkle_verdict_out(3, i, verdicts, summary); return; }
  uint32_t bad = 0;
  for (uint32_t k = l; k < rec; k += 16) bad |= r[k] >= bb::P;
  bad |= (uint32_t)__shfl_xor((int)bad, 1, 16); bad |= (uint32_t)__shfl_xor((int)bad, 2, 16); bad |= (uint32_t)__shfl_xor((int)bad, 4, 16); bad |= (uint32_t)__shfl_xor((int)bad, 8, 16);
  if (bad) { if (l == 0) merkle_verdict_out(2, i, verdicts, summary); return; }
  const uint32_t k_in = cp->in_scale, carry = cp->carry, out_scale = cp->out_scale;
  const uint32_t q = l & 3;
  const uint32_t root_q = root[q];
  const uint32_t* path = r + lead;
  // ONE chain, one copy of the (fully unrolled) permutation: link t < n_sponge absorbs block t of the row, link n_sponge + lvl compresses with the sibling of level lvl
  const uint32_t n_sponge = digest_form ? 0u : (width ? (width + p2::RATE - 1) / p2::RATE : 1u), n_links = n_sponge + depth;
  uint32_t s = 0;
  for (uint32_t t = 0; t < n_links; t++) {
    if (t < n_sponge) {
      const uint32_t off = t * p2::RATE;
      s = (l < (uint32_t)p2::RATE && off + l < width) ? bb::mont_mul_lazy(r[off + l], k_in) : bb::mont_mul_lazy(s, carry);
    } else {
      const uint32_t lvl = t - n_sponge, right = (uint32_t)((j >> lvl) & 1);
      const uint32_t from = (uint32_t)__shfl((int)s, (int)q, 16);            // the node's word q (lanes 0-3 of the last output), on every lane
      const uint32_t nd = t == 0 ? bb::mont_mul_lazy(r[q], k_in) : bb::mont_mul_lazy(from, carry);     // (t = 0 here: the digest form's first level — the node is the record's leaf digest)
      const uint32_t sib = bb::mont_mul_lazy(path[4 * lvl + q], k_in);
      s = l >= 8 ? 0u : ((l >> 2) == right ? nd : sib);          // lanes 0-3 = left child, 4-7 = right child
    }
    s = p2::permute_row16_scaled(s, (int)l, *cp);
  }
  uint32_t eq = n_links ? bb::mont_mul(s, out_scale) == root_q : r[q] == root_q;     // "my word of the digest is the root's" (lanes 0-3 count); no link: the digest form at depth 0, the leaf is the root
  eq &= (uint32_t)__shfl_xor((int)eq, 1, 16); eq &= (uint32_t)__shfl_xor((int)eq, 2, 16);     // lanes 0-3: all four words
  if (l == 0) merkle_verdict_out(eq ? 0u : 1u, i, verdicts, summary);
}

// Which form a batch takes: the row form up to MERKLE_VERIFY_ROW16_MAX records, the lane form above.  Measured on one MI355X (profiles/r11_merkle_open.txt,
// scripts/time_merkle_open.py; width 152, 2^21 and 2^23 leaves): the lane form is flat — 323 / 338 us from 50 to 16384 records, one chain of 40 / 42 links, 375 / 391 us at
// 65536 — while the row form takes 120 / 125 us per GENERATION of waves the chip holds at once and falls behind where the next generation starts.
// ZKIR_VERIFY_FORM_LANE / ZKIR_VERIFY_FORM_ROW16 in `flags` override the rule (tests, measurements).
constexpr uint64_t MERKLE_VERIFY_ROW16_MAX = 8192;

}  // namespace

extern "C" {

uint64_t zkir_merkle_opening_words(uint32_t width, uint64_t n_leaves, uint32_t flags) {
  if (n_leaves == 0 || (n_leaves & (n_leaves - 1))) return 0;
  uint32_t d = 0;
  while (((uint64_t)1 << d) < n_leaves) d++;
  return (uint64_t)((flags & ZKIR_OPEN_LEAF_DIGEST) ? 4u : width) + 4ull * d;
}

int zkir_merkle_open_launch(const zkir_stark_ctx* c, const uint32_t* mat, uint32_t width, uint64_t n_leaves, const uint32_t* tree, const uint64_t* indices, uint64_t n_idx, uint32_t* out, void* stream) {
  if (!c || !tree || !indices || !out) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_merkle_open_launch: null context, tree, indices or out"}); return ZKIR_ERR_ARGUMENT; }
  if (n_leaves == 0 || (n_leaves & (n_leaves - 1)) || n_leaves > ((uint64_t)1 << 27)) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_merkle_open_launch: n_leaves must be a power of two, at most 2^27"}); return ZKIR_ERR_ARGUMENT; }
  if (!mat && width != 0) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_merkle_open_launch: mat == NULL selects the digest form, whose width is 0"}); return ZKIR_ERR_ARGUMENT; }
  if (n_idx > ((uint64_t)1 << 31)) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_merkle_open_launch: more than 2^31 indices in one call"}); return ZKIR_ERR_ARGUMENT; }
  if (n_idx == 0) return ZKIR_OK;
  const uint32_t depth = (uint32_t)(zkir_merkle_opening_words(0, n_leaves, 0) / 4);
  hipLaunchKernelGGL(merkle_open_kernel, dim3(grid_for(n_idx * OPEN_LANES)), dim3(NT), 0, (hipStream_t)stream, mat, width, n_leaves, depth, tree, indices, n_idx, out);
  return check_launch("merkle_open");
}

int zkir_merkle_verify_launch(const zkir_stark_ctx* c, const uint32_t* root, uint32_t width, uint64_t n_leaves, const uint64_t* indices, uint64_t n_idx, const uint32_t* openings, uint32_t flags,
                              uint32_t* verdicts, uint32_t* summary, void* stream) {
  if (!c || !root || !indices || !openings || !verdicts) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_merkle_verify_launch: null context, root, indices, openings or verdicts"}); return ZKIR_ERR_ARGUMENT; }
  if (n_leaves == 0 || (n_leaves & (n_leaves - 1)) || n_leaves > ((uint64_t)1 << 27)) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_merkle_verify_launch: n_leaves must be a power of two, at most 2^27"}); return ZKIR_ERR_ARGUMENT; }
  if (flags & ~(uint32_t)(ZKIR_OPEN_LEAF_DIGEST | ZKIR_VERIFY_FORM_LANE | ZKIR_VERIFY_FORM_ROW16) || ((flags & ZKIR_VERIFY_FORM_LANE) && (flags & ZKIR_VERIFY_FORM_ROW16))) {
    zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_merkle_verify_launch: unknown flag bits, or both verifier forms asked for"}); return ZKIR_ERR_ARGUMENT;
  }
  if ((flags & ZKIR_OPEN_LEAF_DIGEST) && width != 0) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_merkle_verify_launch: the digest form has width 0"}); return ZKIR_ERR_ARGUMENT; }
  if (n_idx > ((uint64_t)1 << 31)) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_merkle_verify_launch: more than 2^31 records in one call (summary[1] is a 32-bit position)"}); return ZKIR_ERR_ARGUMENT; }
  hipStream_t s = (hipStream_t)stream;
  if (summary) hipLaunchKernelGGL(merkle_summary_init_kernel, dim3(1), dim3(64), 0, s, summary);
  if (n_idx == 0) return summary ? check_launch("merkle_verify") : ZKIR_OK;
  const uint32_t depth = (uint32_t)(zkir_merkle_opening_words(0, n_leaves, 0) / 4), digest_form = (flags & ZKIR_OPEN_LEAF_DIGEST) ? 1u : 0u;
  const bool row16 = (flags & ZKIR_VERIFY_FORM_ROW16) || (!(flags & ZKIR_VERIFY_FORM_LANE) && n_idx <= MERKLE_VERIFY_ROW16_MAX);
  if (row16) hipLaunchKernelGGL(merkle_verify_row16_kernel, dim3(grid_for(n_idx * 16, NT_MV)), dim3(NT_MV), 0, s, c->d_p2, root, width, n_leaves, depth, indices, n_idx, openings, digest_form, verdicts, summary);
  else hipLaunchKernelGGL(merkle_verify_kernel, dim3(grid_for(n_idx, NT_MV)), dim3(NT_MV), 0, s, c->d_p2, root, width, n_leaves, depth, indices, n_idx, openings, digest_form, verdicts, summary);
  return check_launch("merkle_verify");
}

}  // extern "C"
