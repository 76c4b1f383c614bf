// tape_stage_many.inl — the device form of a mode-4 proof's tape stages over a LIST of proofs (verify_stages.h: TapeManyStage) and the stand-alone entry
// zkir_tape_sections_stage_launch: what zkir_verify_many_tapes_device (stark_verify.inl) and zkir_verify_rate_many_tapes_device (pcs_verify_many.inl) run their fronts with,
// beside the memory list stage.  Included by stark_prove.inl at file scope, behind mem_stage_many.inl: the per-device block, its mutex and pinned staging are
// verify_device.inl's, the record rules are tape_table.inl's, the digests' bodies tape_digest.inl's, the sponge section_hash_kernel's.
//
// As in mem_stage_many.inl, a per-proof RECORD in device memory replaces a launch per proof.  Calls, touched cells and wide records are numbered over the WHOLE batch:
// proof i's calls are [TR_CALL0, TR_CALL0 + TR_NCHECK), its cells start at TR_CELL0, its wide records at TR_WREC0, and ONE concatenated prefix array says before which
// global cell a global call's cells start.  A lane finds its proof by a binary search over the records, so lanes of one wave may belong to different proofs: 64 one-call
// tapes are one wave, not 64 workgroups.
//
// Phase A (prepare: before any front): one staged upload of every located tape and the records, the two check launches and the digest launch, ONE synchronisation; then
// the old-bytes and new-bytes launches are enqueued — over the proofs whose hash check returned 0, which the kernels read from the result words — and NOT waited for: they
// overlap the host fronts, and so do the host threads that hash the calls above TAPE_L_DEV.  Phase B (sides: behind the last front): one upload of the deferred proofs' lookup
// parameters and the patches, one patch launch if any call is long, the two side launches, ONE synchronisation.  The region lies behind the memory stage's batch region.
//
// UNTRUSTED INPUT: no extent is sized by a count word.  The records are placed by tape_section_walk (a record's cell count from its own fields, the walk ends where the
// proof does), the wide records are those the caller has seen inside the proof.  The check and digest kernels run on unchecked words; the byte and side kernels never see a
// record of a tape that failed its check.  Allocation failures and exceptions become a negative return.
#include <thread>

namespace {

constexpr uint32_t TR_OFF = 0, TR_CALL0 = 1, TR_CELL0 = 2, TR_NCHECK = 3, TR_NFULL = 4, TR_NREAL_LO = 5, TR_NREAL_HI = 6, TR_CODE_END = 7, TR_WOFF = 8, TR_WREC0 = 9, TR_NWIDE = 10, TR_NCELLS = 11,
                   TR_WORDS = 16;                               // a proof's record; offsets count words of the block (the wide records start on 16 bytes)
constexpr uint32_t DS_OFF = 0, DS_LEN = 1, DS_CHUNK0 = 2, DS_WORDS = 4;      // a section to digest: where, how many words, its first chunk
constexpr uint32_t TJ_REC = 0, TJ_WG0 = 1, TJ_NWG = 2, TJ_LK = 3, TJ_WORDS = 4;      // a side job: the proof's record, its workgroups (= partial sums), its lk slot (words of the block)
constexpr unsigned TAPE_JOB_BLOCKS = 512;                       // a side job's grid cap

// the record an id belongs to: the largest i < n with recs[i][field] <= id (record 0's is 0, the field rises; a record with an empty range is never found)
__device__ __forceinline__ uint32_t tape_record_of(const uint32_t* __restrict__ recs, uint32_t words, uint32_t field, uint32_t n, uint32_t id) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (recs[words * mid + field] <= id) lo = mid; else hi = mid; }
  return lo;
}
__device__ __forceinline__ const uint32_t* tape_call_at(const uint32_t* __restrict__ blk, const uint32_t* __restrict__ r, const uint32_t* __restrict__ prefix, uint64_t k) {
  return blk + ((uint64_t)r[TR_OFF] + 1 + 8 * k + 5 * (uint64_t)(prefix[(uint64_t)r[TR_CALL0] + k] - r[TR_CELL0]));
}

// hash_tape_check_kernel's rules, one call per LANE over all proofs; call 0 of a proof has no predecessor.  results[i] = min over proof i's failing calls of
// (call << 8 | code) (the caller uploads them: all ones, or what the walk itself found).
__global__ __launch_bounds__(NT) void hash_tapes_check_kernel(const uint32_t* __restrict__ blk, const uint32_t* __restrict__ recs, uint32_t n_sec, const uint32_t* __restrict__ prefix, uint32_t n_check,
                                                               unsigned long long* __restrict__ results) {
  const uint64_t g = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (g >= n_check) return;
  const uint32_t i = tape_record_of(recs, TR_WORDS, TR_CALL0, n_sec, (uint32_t)g);
  const uint32_t* r = recs + TR_WORDS * i;
  const uint64_t k = g - r[TR_CALL0], n_real = (uint64_t)r[TR_NREAL_LO] | ((uint64_t)r[TR_NREAL_HI] << 32), code_end = r[TR_CODE_END];
  const uint32_t* c = tape_call_at(blk, r, prefix, k);
  uint32_t code = 0;
  const uint64_t cycle = c[0], in_ptr = (uint64_t)c[1] | ((uint64_t)c[2] << 20), len = c[3], out_ptr = (uint64_t)c[4] | ((uint64_t)c[5] << 20);
  if (c[1] >= (1u << 20) || c[2] >= (1u << 20) || c[4] >= (1u << 20) || c[5] >= (1u << 20)) code = 56;
  else if (cycle >= n_real || (k && cycle <= tape_call_at(blk, r, prefix, k - 1)[0]) || !hashcall::in_range(in_ptr, len, out_ptr, c[6])) code = 56;
  else if (out_ptr < code_end && out_ptr + 32 > 0x1000) code = 55;
  else {
    const uint64_t n = hashcall::n_cells_of(in_ptr, len, out_ptr);
    if (c[7] != n) code = 56;
    else if (k >= r[TR_NFULL]) code = 4;
    else {
      const uint32_t* q = c + 8;
      for (uint64_t j = 0; j < n && !code; j++, q += 5)
        if (q[1] > 0xFFFF || q[2] > 0xFFFF || q[3] > 0xFFFF || q[4] > 0xFFFF || q[0] > cycle) code = 56;
    }
  }
  if (code) atomicMin(results + i, (unsigned long long)((k << 8) | code));
}

// wide_tape_check_kernel's rules, one record per lane over all proofs; record 0 of a proof has no predecessor.  bad[i] (zeroed by the caller) != 0: a record of proof i fails.
__global__ __launch_bounds__(NT) void wide_tapes_check_kernel(const uint32_t* __restrict__ blk, const uint32_t* __restrict__ recs, uint32_t n_sec, uint32_t n_wide, uint32_t* __restrict__ bad) {
  const uint64_t g = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (g >= n_wide) return;
  const uint32_t i = tape_record_of(recs, TR_WORDS, TR_WREC0, n_sec, (uint32_t)g);
  const uint32_t* r = recs + TR_WORDS * i;
  const uint64_t k = g - r[TR_WREC0], n_real = (uint64_t)r[TR_NREAL_LO] | ((uint64_t)r[TR_NREAL_HI] << 32);
  const uint32_t* c = blk + ((uint64_t)r[TR_WOFF] + 8 * k);
  const bool fails = c[1] >= (1u << 20) || c[2] >= (1u << 20) || c[3] >= (1u << 24) || c[4] >= (1u << 20) || c[5] >= (1u << 20) || c[6] >= (1u << 24) || c[7] < 3 || c[7] > 7 ||
                     c[0] >= n_real || (k && c[0] <= c[-8]) || (c[7] >= 4 && !(c[4] | c[5] | c[6]));
  if (fails) atomicOr(bad + i, 1u);
}

// mem_sections_hash_kernel's quad-per-chunk sponge with the section's word length taken from its record: a ragged last chunk ends at ITS section's end
__global__ __launch_bounds__(64) void tape_sections_hash_kernel(const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ blk, const uint32_t* __restrict__ secs, uint32_t n_sec, uint32_t n_chunks,
                                                                uint32_t* __restrict__ digests) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x, c = t >> 2;
  const int l = (int)(t & 3);
  if (c >= n_chunks) return;                                     // whole quads leave together
  const uint32_t* r = secs + DS_WORDS * tape_record_of(secs, DS_WORDS, DS_CHUNK0, n_sec, c);
  const uint64_t n_words = r[DS_LEN], at = (uint64_t)(c - r[DS_CHUNK0]) * SECTION_CHUNK;
  const uint32_t* w = blk + ((uint64_t)r[DS_OFF] + at);
  const uint64_t len = n_words - at < SECTION_CHUNK ? n_words - at : SECTION_CHUNK;
  uint32_t st[3] = {0, 0, 0};
  const uint32_t k_in = cp->in_scale, carry = cp->carry;
  for (uint64_t off = 0; off < len; off += p2::RATE) {
    st[0] = off + l < len ? bb::mont_mul_lazy(w[off + l], k_in) : bb::mont_mul_lazy(st[0], carry);
    st[1] = off + 4 + l < len ? bb::mont_mul_lazy(w[off + 4 + l], k_in) : bb::mont_mul_lazy(st[1], carry);
    st[2] = bb::mont_mul_lazy(st[2], carry);
    p2::permute_quad_scaled(st, l, *cp);
  }
  digests[4 * c + l] = bb::mont_mul(st[0], cp->out_scale);
}

// the call of proof r that holds the proof's cell h (local): the last call whose prefix <= h
__device__ __forceinline__ uint64_t tape_call_of_cell(const uint32_t* __restrict__ r, const uint32_t* __restrict__ prefix, uint64_t n_calls, uint64_t h) {
  const uint32_t* p = prefix + r[TR_CALL0];
  const uint64_t hg = h + r[TR_CELL0];
  uint64_t lo = 0, hi = n_calls;
  while (lo + 1 < hi) { const uint64_t m = lo + (hi - lo) / 2; if (p[m] <= hg) lo = m; else hi = m; }
  return lo;
}
// hash_tape_old_bytes_kernel over the cells of every proof whose hash check returned 0: side[global cell] = the cell's OLD bytes
__global__ __launch_bounds__(NT) void hash_tapes_old_bytes_kernel(const uint32_t* __restrict__ blk, const uint32_t* __restrict__ recs, uint32_t n_sec, const uint32_t* __restrict__ prefix,
                                                                   const unsigned long long* __restrict__ results, uint64_t n_cells, uint64_t* __restrict__ side) {
  for (uint64_t g = (uint64_t)blockIdx.x * NT + threadIdx.x; g < n_cells; g += (uint64_t)gridDim.x * NT) {
    const uint32_t i = tape_record_of(recs, TR_WORDS, TR_CELL0, n_sec, (uint32_t)g);
    if (results[i] != ~0ull) continue;
    const uint32_t* r = recs + TR_WORDS * i;
    const uint64_t h = g - r[TR_CELL0], lo = tape_call_of_cell(r, prefix, r[TR_NFULL], h);
    side[g] = td_cell(blk + ((uint64_t)r[TR_OFF] + 1 + 8 * (lo + 1) + 5 * h));
  }
}
// hash_tape_new_bytes_kernel's body, one lane per call of at most TAPE_L_DEV bytes of every proof whose hash check returned 0 (every count word of such a proof is
// n_cells_of its record, every field is in range)
__global__ __launch_bounds__(NT) void hash_tapes_new_bytes_kernel(const uint32_t* __restrict__ blk, const uint32_t* __restrict__ recs, uint32_t n_sec, const uint32_t* __restrict__ prefix,
                                                                   const unsigned long long* __restrict__ results, uint32_t n_check, uint64_t* __restrict__ side) {
  const uint64_t g = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (g >= n_check) return;
  const uint32_t i = tape_record_of(recs, TR_WORDS, TR_CALL0, n_sec, (uint32_t)g);
  if (results[i] != ~0ull) return;
  const uint32_t* r = recs + TR_WORDS * i;
  const uint64_t before = prefix[g];
  const uint32_t* c = tape_call_at(blk, r, prefix, g - r[TR_CALL0]);
  const uint64_t in_ptr = (uint64_t)c[1] | ((uint64_t)c[2] << 20), out_ptr = (uint64_t)c[4] | ((uint64_t)c[5] << 20);
  const uint32_t len = c[3], kind = c[6];
  if (len > TAPE_L_DEV) return;                                 // (the host's: long_call_patches)
  TapeMsg m{c + 8, 8 * (uint32_t)(in_ptr & 7), len, 0};
  if (len) { m.q = c + 8 + 5 * hashcall::rank_of(in_ptr, len, out_ptr, in_ptr & ~7ull); m.n_in = (uint32_t)(((in_ptr + len - 1) >> 3) - (in_ptr >> 3)) + 1; }
  uint64_t d[4];
  if (kind == 3) td_sha256(m, d); else if (kind == 5) td_keccak256(m, d); else td_blake3(m, d);
  const uint64_t r_out = hashcall::rank_of(in_ptr, len, out_ptr, out_ptr & ~7ull);
  const uint32_t sh = 8 * (uint32_t)(out_ptr & 7), n_out = sh ? 5 : 4;
  const uint32_t* q = c + 8 + 5 * r_out;
  uint64_t* o = side + before + r_out;
#pragma unroll
  for (int t = 0; t < 5; t++) {
    if ((uint32_t)t >= n_out) break;
    uint64_t val = 0, mask = 0;
    if (t < 4) { val = d[t < 4 ? t : 0] << sh; mask = ~0ull << sh; }
    if (t > 0 && sh) { val |= d[t - 1 >= 0 ? t - 1 : 0] >> (64 - sh); mask |= ~0ull >> (64 - sh); }
    o[t] = (td_cell(q + 5 * t) & ~mask) | val;
  }
}

// hash_table_side_kernel's terms over the deferred proofs: a workgroup belongs to ONE job (uniform lookup), job j has its own lk slot and TJ_NWG workgroups that stride
// over its calls and cells; one partial sum per workgroup at partial[TJ_WG0 ..].  (The HashAux list is the prover's: not written.)
__global__ __launch_bounds__(NT) void hash_tapes_side_kernel(const uint32_t* __restrict__ blk, const uint32_t* __restrict__ recs, const uint32_t* __restrict__ jobs, uint32_t n_jobs,
                                                              const uint32_t* __restrict__ prefix, const uint64_t* __restrict__ side, E4* __restrict__ partial) {
  const uint32_t* jb = jobs + TJ_WORDS * tape_record_of(jobs, TJ_WORDS, TJ_WG0, n_jobs, blockIdx.x);
  const uint32_t* r = recs + TR_WORDS * jb[TJ_REC];
  const uint32_t* lk = blk + jb[TJ_LK];
  const uint64_t n_calls = r[TR_NFULL], n_items = n_calls + r[TR_NCELLS], stride = (uint64_t)jb[TJ_NWG] * NT;
  E4 acc = bb::e_zero();
  for (uint64_t i = (uint64_t)(blockIdx.x - jb[TJ_WG0]) * NT + threadIdx.x; i < n_items; i += stride) {
    if (i < n_calls) {
      const uint32_t* c = tape_call_at(blk, r, prefix, i);
      acc = bb::e_add(acc, bb::e_inv_m(hash_call_den(lk, c[0], (uint64_t)c[1] | ((uint64_t)c[2] << 20), c[3], (uint64_t)c[4] | ((uint64_t)c[5] << 20), c[6])));
    } else {
      const uint64_t h = i - n_calls, lo = tape_call_of_cell(r, prefix, n_calls, h);
      const uint32_t* c = tape_call_at(blk, r, prefix, lo);
      const uint64_t rk = h - (prefix[(uint64_t)r[TR_CALL0] + lo] - r[TR_CELL0]);
      const uint64_t addr = hashcall::cell_at((uint64_t)c[1] | ((uint64_t)c[2] << 20), c[3], (uint64_t)c[4] | ((uint64_t)c[5] << 20), rk);
      const uint32_t* q = c + 8 + 5 * rk;
      const uint64_t old = (uint64_t)q[1] | ((uint64_t)q[2] << 16) | ((uint64_t)q[3] << 32) | ((uint64_t)q[4] << 48);
      const E4 dm = mem_cell_den(lk, addr, q[0], old), dp = mem_cell_den(lk, addr, (uint32_t)(((uint64_t)c[0] + 1) % bb::P), side[(uint64_t)r[TR_CELL0] + h]);
      acc = bb::e_add(acc, bb::e_mul_m(bb::e_sub(dm, dp), bb::e_inv_m(bb::e_mul_m(dp, dm))));      // 1 / d+ - 1 / d-: one inversion for the two terms
    }
  }
  block_sum_to(acc, partial + blockIdx.x);
}
// wide_table_side_kernel's terms over the deferred proofs, jobs as above
__global__ __launch_bounds__(NT) void wide_tapes_side_kernel(const uint32_t* __restrict__ blk, const uint32_t* __restrict__ recs, const uint32_t* __restrict__ jobs, uint32_t n_jobs,
                                                              E4* __restrict__ partial) {
  const uint32_t* jb = jobs + TJ_WORDS * tape_record_of(jobs, TJ_WORDS, TJ_WG0, n_jobs, blockIdx.x);
  const uint32_t* r = recs + TR_WORDS * jb[TJ_REC];
  const uint32_t* lk = blk + jb[TJ_LK];
  const uint4* wr = reinterpret_cast<const uint4*>(blk + r[TR_WOFF]);
  const uint64_t n = r[TR_NWIDE], stride = (uint64_t)jb[TJ_NWG] * NT;
  E4 acc = bb::e_zero();
  for (uint64_t k = (uint64_t)(blockIdx.x - jb[TJ_WG0]) * NT + threadIdx.x; k < n; k += stride) {
    const uint4 r0 = wr[2 * k], r1 = wr[2 * k + 1];
    const uint32_t rec[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    acc = bb::e_add(acc, bb::e_inv_m(wide_record_den(lk, rec)));
  }
  block_sum_to(acc, partial + blockIdx.x);
}

inline unsigned tape_job_grid(uint64_t n_items) { const uint64_t g = (n_items + NT - 1) / NT; return (unsigned)(g < TAPE_JOB_BLOCKS ? g : TAPE_JOB_BLOCKS); }

// The device form of the tape list stage.  It shares the memory list stage's runner (the device state, the mutex held from prepare to done, the stream) and lays its region
// out BEHIND that stage's: [records][digest records][prefix][result words][wide flags][tapes: hash on 256 bytes, wide records on 16][chunk digests][side]; the memory stage's
// phase B and then this stage's ([jobs][lk slots][patches][partial sums]) lie behind it.
struct TapeManyDevice {
  MemManyDevice& md;
  size_t base = 0, o_prefix = 0, o_res = 0, o_side = 0, end_a = 0;
  std::vector<uint32_t> recs;
  std::vector<std::vector<uint64_t>> lprefix;                    // per section the walk's prefix (the long calls' patches are formed from host words)
  std::vector<uint8_t> passed;
  std::vector<const uint32_t*> hash_at;                          // per section its hash words (the caller's list need not outlive the patcher)
  uint64_t n_check = 0, n_cells = 0, n_wide = 0;
  uint32_t launches = 0;
  uint64_t uploaded_words = 0;
  bool ran = false;
  std::thread patcher;                                           // long_call_patches of every passing proof, while the fronts run
  std::vector<uint64_t> pidx, pval;
  bool patch_failed = false;

  explicit TapeManyDevice(MemManyDevice& m) : md(m) {}
  ~TapeManyDevice() { if (patcher.joinable()) patcher.join(); }
  int refuse(const char* what, int code = ZKIR_ERR_OTHER) { return md.refuse(what, code); }
  unsigned char* D() const { return md.V->d; }

  int prepare(const zkir::TapeSection* list, uint32_t n, int* hv, uint64_t* used, int* wv, uint32_t* digests) {
    if (!n) return 0;
    if (const int rc = md.device()) return rc;
    if (!md.lock.owns_lock()) md.lock = std::unique_lock<std::mutex>(md.V->mu);
    VerifyDevice& V = *md.V;
    V.pin.reset();
    base = md.region;
    hipStream_t s = md.s;
    // ---- the walk and the layout ----
    recs.assign((size_t)n * TR_WORDS, 0);
    lprefix.assign(n, {});
    passed.assign(n, 0);
    hash_at.assign(n, nullptr);
    std::vector<uint32_t> drecs;
    std::vector<unsigned long long> res0(n, ~0ull);
    std::vector<size_t> up_words(n, 0);
    size_t at = base + al256((size_t)n * TR_WORDS * 4) + al256((size_t)2 * n * DS_WORDS * 4);
    const size_t o_drecs = base + al256((size_t)n * TR_WORDS * 4);
    uint64_t calls = 0, cells = 0, wides = 0, chunks = 0;
    for (uint32_t i = 0; i < n; i++) {
      const zkir::TapeSection& S = list[i];
      if (!S.hash || S.avail < 1 || (S.code_end >> 32) || (S.wide && S.n_wide > (1u << 28))) return refuse("a tape description is not a located pair's");
      uint32_t* r = recs.data() + (size_t)i * TR_WORDS;
      hash_at[i] = S.hash;
      const uint64_t nh = S.hash[0];
      zkir::TapeExtent x;
      if (nh > S.n_real) res0[i] = 56;                           // (hashcall::parse_section's first check: call 0, code 56; no record is looked at)
      else {
        lprefix[i].resize((size_t)std::min<uint64_t>(nh, S.avail / 8) + 2);
        x = zkir::tape_section_walk(S.hash, S.avail, lprefix[i].data());
        if (!x.whole && !x.header_only) res0[i] = ((unsigned long long)x.n_full << 8) | 4u;      // (the walk left the proof before record n_full's header)
        if (x.whole != S.whole || (x.whole && x.used != S.hash_words)) return refuse("a tape description does not match its words");
        up_words[i] = (size_t)(x.used + (x.header_only ? 8 : 0));
      }
      r[TR_NCHECK] = (uint32_t)(x.n_full + (x.header_only ? 1 : 0)); r[TR_NFULL] = (uint32_t)x.n_full; r[TR_NCELLS] = (uint32_t)x.cells;
      r[TR_CALL0] = (uint32_t)calls; r[TR_CELL0] = (uint32_t)cells; r[TR_WREC0] = (uint32_t)wides;
      r[TR_NREAL_LO] = (uint32_t)S.n_real; r[TR_NREAL_HI] = (uint32_t)(S.n_real >> 32); r[TR_CODE_END] = (uint32_t)S.code_end;
      r[TR_OFF] = (uint32_t)(at / 4); at += al256(up_words[i] * 4);
      if (x.whole && nh <= S.n_real) { drecs.insert(drecs.end(), {r[TR_OFF], (uint32_t)x.used, (uint32_t)chunks, 0u}); chunks += (x.used + 511) / 512; }
      if (S.wide) {
        r[TR_WOFF] = (uint32_t)(at / 4 + 4); r[TR_NWIDE] = (uint32_t)S.n_wide;      // (the count word at + 12 bytes, the records on 16)
        drecs.insert(drecs.end(), {r[TR_WOFF] - 1, (uint32_t)(1 + 8 * S.n_wide), (uint32_t)chunks, 0u}); chunks += (1 + 8 * S.n_wide + 511) / 512;
        at += al256(16 + 32 * (size_t)S.n_wide);
      }
      calls += r[TR_NCHECK]; cells += x.cells; wides += S.wide ? S.n_wide : 0;
      if ((at >> 33) || (calls >> 31) || (cells >> 31) || (wides >> 31) || (chunks >> 29)) return refuse("the batch's tapes are too large for one block");
    }
    const uint32_t n_dsec = (uint32_t)(drecs.size() / DS_WORDS);
    o_prefix = at; at += al256((size_t)calls * 4 + 4);
    o_res = at; at += al256((size_t)n * 8);
    const size_t o_bad = at; at += al256((size_t)n * 4);
    const size_t up_end = at, o_dg = at; at += al256(16 * (size_t)chunks + 16);
    o_side = at; at += al256(8 * (size_t)cells + 8);
    end_a = at;
    if (end_a >> 33) return refuse("the batch's tapes are too large for one block");
    n_check = calls; n_cells = cells; n_wide = wides;
    // ---- one staged upload, three launches, one synchronisation ----
    int rc = V.ensure(end_a, base); if (rc) return -rc;
    unsigned char* h = (unsigned char*)V.pin.take(up_end - base);
    unsigned char* hr = (unsigned char*)V.pin.take(o_dg - o_res);
    uint32_t* hd = V.pin.take_n<uint32_t>(4 * (size_t)chunks + 4);
    if (!h || !hr || !hd) return refuse("no pinned host memory", ZKIR_ERR_DEVICE);
    memcpy(h, recs.data(), recs.size() * 4);
    if (!drecs.empty()) memcpy(h + (o_drecs - base), drecs.data(), drecs.size() * 4);
    uint32_t* hp = (uint32_t*)(h + (o_prefix - base));
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t* r = recs.data() + (size_t)i * TR_WORDS;
      if (up_words[i]) memcpy(h + (4 * (size_t)r[TR_OFF] - base), list[i].hash, up_words[i] * 4);
      if (list[i].wide) memcpy(h + (4 * (size_t)(r[TR_WOFF] - 1) - base), list[i].wide, (1 + 8 * (size_t)list[i].n_wide) * 4);
      for (uint32_t k = 0; k < r[TR_NCHECK]; k++) hp[r[TR_CALL0] + k] = r[TR_CELL0] + (uint32_t)lprefix[i][k];
    }
    memcpy(h + (o_res - base), res0.data(), (size_t)n * 8);
    memset(h + (o_bad - base), 0, (size_t)n * 4);
    if (hipMemcpyAsync(D() + base, h, up_end - base, hipMemcpyHostToDevice, s) != hipSuccess) { (void)check_launch(md.who); return -ZKIR_ERR_DEVICE; }
    uploaded_words += (up_end - base) / 4;
    ran = true;
    const uint32_t* d_blk = (const uint32_t*)D();
    const uint32_t* d_recs = (const uint32_t*)(D() + base);
    const uint32_t* d_prefix = (const uint32_t*)(D() + o_prefix);
    unsigned long long* d_res = (unsigned long long*)(D() + o_res);
    if (calls) { hipLaunchKernelGGL(hash_tapes_check_kernel, dim3(grid_for(calls)), dim3(NT), 0, s, d_blk, d_recs, n, d_prefix, (uint32_t)calls, d_res); launches++; }
    if (wides) { hipLaunchKernelGGL(wide_tapes_check_kernel, dim3(grid_for(wides)), dim3(NT), 0, s, d_blk, d_recs, n, (uint32_t)wides, (uint32_t*)(D() + o_bad)); launches++; }
    if (chunks) {
      hipLaunchKernelGGL(tape_sections_hash_kernel, dim3((unsigned)((4 * chunks + 63) / 64)), dim3(64), 0, s, V.d_p2, d_blk, (const uint32_t*)(D() + o_drecs), n_dsec, (uint32_t)chunks, (uint32_t*)(D() + o_dg));
      launches++;
    }
    if (hipMemcpyAsync(hr, D() + o_res, o_dg - o_res, hipMemcpyDeviceToHost, s) != hipSuccess || (chunks && hipMemcpyAsync(hd, D() + o_dg, 16 * (size_t)chunks, hipMemcpyDeviceToHost, s) != hipSuccess) ||
        hipStreamSynchronize(s) != hipSuccess || check_launch(md.who) != ZKIR_OK) return -ZKIR_ERR_DEVICE;
    // ---- the answers, in the caller's chunk order (a section that is not whole has no digests there and none here) ----
    const unsigned long long* res = (const unsigned long long*)hr;
    const uint32_t* bad = (const uint32_t*)(hr + (o_bad - o_res));
    uint64_t c_in = 0, c_out = 0, pass_calls = 0;
    bool any_long = false;
    for (uint32_t i = 0; i < n; i++) {
      const zkir::TapeSection& S = list[i];
      const uint32_t* r = recs.data() + (size_t)i * TR_WORDS;
      hv[i] = res[i] == ~0ull ? 0 : (int)(res[i] & 0xFF);
      used[i] = hv[i] ? 0 : S.hash_words;
      wv[i] = S.wide && bad[i] ? 57 : 0;
      const uint64_t c0 = zkir::tape_section_chunks(S, 0), c1 = zkir::tape_section_chunks(S, 1), d0 = S.whole && S.hash[0] <= S.n_real ? c0 : 0;
      if (d0) memcpy(digests + 4 * c_out, hd + 4 * c_in, 16 * (size_t)d0);
      if (c1) memcpy(digests + 4 * (c_out + c0), hd + 4 * (c_in + d0), 16 * (size_t)c1);
      c_in += d0 + c1; c_out += c0 + c1;
      passed[i] = !hv[i];
      if (passed[i]) { pass_calls += r[TR_NFULL]; for (uint32_t k = 0; k < r[TR_NFULL] && !any_long; k++) any_long = S.hash[1 + 8 * (size_t)k + 5 * lprefix[i][k] + 3] > TAPE_L_DEV; }
    }
    // ---- what every passing call wrote: enqueued, not waited for ----
    if (pass_calls) {
      hipLaunchKernelGGL(hash_tapes_old_bytes_kernel, dim3(tape_grid(cells)), dim3(NT), 0, s, d_blk, d_recs, n, d_prefix, d_res, cells, (uint64_t*)(D() + o_side));
      hipLaunchKernelGGL(hash_tapes_new_bytes_kernel, dim3(grid_for(calls)), dim3(NT), 0, s, d_blk, d_recs, n, d_prefix, d_res, (uint32_t)calls, (uint64_t*)(D() + o_side));
      launches += 2;
      md.tape_inflight = true;
    }
    if (any_long) patcher = std::thread([this, n] {
      try {
        std::vector<uint64_t> idx, val;
        for (uint32_t i = 0; i < n; i++) if (passed[i]) {
          const uint32_t* r = recs.data() + (size_t)i * TR_WORDS;
          long_call_patches(hash_at[i], lprefix[i].data(), r[TR_NFULL], idx, val);
          for (size_t k = 0; k < idx.size(); k++) { pidx.push_back(idx[k] + r[TR_CELL0]); pval.push_back(val[k]); }
        }
      } catch (...) { patch_failed = true; }
    });
    md.region = end_a;                                           // (the memory stage's phase B lays its data out behind this region)
    return 0;
  }
  int sides(const zkir::TapeSection*, const zkir::TapeSideJob* jobs, uint32_t n_jobs, uint32_t* sums) {
    if (!n_jobs) return 0;
    if (!md.lock.owns_lock() || !ran) return refuse("the table sides were asked for before the tapes went up");
    if (patcher.joinable()) patcher.join();
    if (patch_failed) return refuse("no memory for the long calls' digests");
    VerifyDevice& V = *md.V;
    hipStream_t s = md.s;
    V.pin.reset();
    const uint32_t n_sec = (uint32_t)passed.size();
    std::vector<uint32_t> hj, wj;
    std::vector<int> h_of(n_jobs, -1), w_of(n_jobs, -1);
    uint64_t hwg = 0, wwg = 0;
    const size_t o_wj = end_a + al256((size_t)n_jobs * TJ_WORDS * 4), o_lk = o_wj + al256((size_t)n_jobs * TJ_WORDS * 4), lk_step = al256(air::N_LK * 4);      // [hash jobs][wide jobs][lk slots]
    for (uint32_t j = 0; j < n_jobs; j++) {
      const zkir::TapeSideJob& J = jobs[j];
      if (J.section >= n_sec) return refuse("a table-side job names no tape of the batch");
      const uint32_t* r = recs.data() + (size_t)J.section * TR_WORDS;
      const uint32_t lk = (uint32_t)((o_lk + j * lk_step) / 4);
      if (J.hash && !passed[J.section]) return refuse("a table-side job names a hash tape that failed its check");
      if (J.hash && r[TR_NFULL]) { const uint32_t g = tape_job_grid((uint64_t)r[TR_NFULL] + r[TR_NCELLS]); h_of[j] = (int)(hj.size() / TJ_WORDS); hj.insert(hj.end(), {J.section, (uint32_t)hwg, g, lk}); hwg += g; }
      if (J.wide && r[TR_NWIDE]) { const uint32_t g = tape_job_grid(r[TR_NWIDE]); w_of[j] = (int)(wj.size() / TJ_WORDS); wj.insert(wj.end(), {J.section, (uint32_t)wwg, g, lk}); wwg += g; }
    }
    const size_t o_pidx = o_lk + n_jobs * lk_step, o_pval = o_pidx + al256(pidx.size() * 8 + 8), o_part = o_pval + al256(pval.size() * 8 + 8),
                 total = o_part + al256((size_t)(hwg + wwg) * sizeof(E4) + 16);
    if ((total >> 33) || ((hwg + wwg) >> 31)) return refuse("the batch's table-side jobs are too large for one block");
    if (total > V.cap && md.tape_inflight) { if (hipStreamSynchronize(s) != hipSuccess) return -ZKIR_ERR_DEVICE; md.tape_inflight = false; }      // (a larger block is a copy of this one: nothing may be writing it)
    int rc = V.ensure(total, end_a); if (rc) return -rc;
    unsigned char* h = (unsigned char*)V.pin.take(o_part - end_a);
    E4* hp = V.pin.take_n<E4>((size_t)(hwg + wwg) + 1);
    if (!h || !hp) return refuse("no pinned host memory", ZKIR_ERR_DEVICE);
    if (!hj.empty()) memcpy(h, hj.data(), hj.size() * 4);
    if (!wj.empty()) memcpy(h + (o_wj - end_a), wj.data(), wj.size() * 4);
    for (uint32_t j = 0; j < n_jobs; j++) memcpy(h + (o_lk + j * lk_step - end_a), jobs[j].lk_m, air::N_LK * 4);
    if (!pidx.empty()) { memcpy(h + (o_pidx - end_a), pidx.data(), pidx.size() * 8); memcpy(h + (o_pval - end_a), pval.data(), pval.size() * 8); }
    if (hipMemcpyAsync(D() + end_a, h, o_part - end_a, hipMemcpyHostToDevice, s) != hipSuccess) { (void)check_launch(md.who); return -ZKIR_ERR_DEVICE; }
    uploaded_words += (o_part - end_a) / 4;
    const uint32_t* d_blk = (const uint32_t*)D();
    const uint32_t* d_recs = (const uint32_t*)(D() + base);
    if (!pidx.empty() && hwg) {
      hipLaunchKernelGGL(side_patch_kernel, dim3(grid_for(pidx.size())), dim3(NT), 0, s, (const uint64_t*)(D() + o_pidx), (const uint64_t*)(D() + o_pval), (uint64_t)pidx.size(), (uint64_t*)(D() + o_side));
      launches++;
    }
    if (hwg) {
      hipLaunchKernelGGL(hash_tapes_side_kernel, dim3((unsigned)hwg), dim3(NT), 0, s, d_blk, d_recs, (const uint32_t*)(D() + end_a), (uint32_t)(hj.size() / TJ_WORDS), (const uint32_t*)(D() + o_prefix),
                         (const uint64_t*)(D() + o_side), (E4*)(D() + o_part));
      launches++;
    }
    if (wwg) {
      hipLaunchKernelGGL(wide_tapes_side_kernel, dim3((unsigned)wwg), dim3(NT), 0, s, d_blk, d_recs, (const uint32_t*)(D() + o_wj), (uint32_t)(wj.size() / TJ_WORDS), (E4*)(D() + o_part) + hwg);
      launches++;
    }
    if ((hwg + wwg && hipMemcpyAsync(hp, D() + o_part, (size_t)(hwg + wwg) * sizeof(E4), hipMemcpyDeviceToHost, s) != hipSuccess) || hipStreamSynchronize(s) != hipSuccess || check_launch(md.who) != ZKIR_OK)
      return -ZKIR_ERR_DEVICE;
    md.tape_inflight = false;
    for (uint32_t j = 0; j < n_jobs; j++) {
      E4 th = bb::e_zero(), tw = bb::e_zero();
      if (h_of[j] >= 0) { const uint32_t* r = hj.data() + (size_t)h_of[j] * TJ_WORDS; for (uint32_t b = 0; b < r[TJ_NWG]; b++) th = bb::e_add(th, hp[r[TJ_WG0] + b]); }
      if (w_of[j] >= 0) { const uint32_t* r = wj.data() + (size_t)w_of[j] * TJ_WORDS; for (uint32_t b = 0; b < r[TJ_NWG]; b++) tw = bb::e_add(tw, hp[hwg + r[TJ_WG0] + b]); }
      memcpy(sums + 8 * (size_t)j, th.c, 16); memcpy(sums + 8 * (size_t)j + 4, tw.c, 16);
    }
    return 0;
  }
  void done() {                                                  // nothing of the batch stays in flight: the query stage lays its data out from offset 0
    if (patcher.joinable()) patcher.join();
    if (md.lock.owns_lock()) { if (launches) (void)hipStreamSynchronize(md.s); md.tape_inflight = false; }
    md.done();
  }
  zkir::TapeManyStage stage() {
    return zkir::TapeManyStage{this,
      [](void* p, const zkir::TapeSection* list, uint32_t n, int* hv, uint64_t* used, int* wv, uint32_t* digests) { return guarded([&] { return static_cast<TapeManyDevice*>(p)->prepare(list, n, hv, used, wv, digests); }); },
      [](void* p, const zkir::TapeSection* list, const zkir::TapeSideJob* jobs, uint32_t n_jobs, uint32_t* sums) { return guarded([&] { return static_cast<TapeManyDevice*>(p)->sides(list, jobs, n_jobs, sums); }); },
      [](void* p) { static_cast<TapeManyDevice*>(p)->done(); }};
  }
};

}  // namespace

extern "C" {

int zkir_tape_sections_stage_launch(const uint32_t* const* hash_secs, const uint64_t* hash_words, const uint32_t* const* wide_secs, const uint64_t* wide_words, const uint64_t* n_real,
                                    const uint64_t* code_end, const uint32_t* alphas, const uint32_t* lambdas, uint32_t n, int32_t* hash_verdicts, int32_t* wide_verdicts, uint32_t* digests,
                                    uint32_t* sums, void* stream) {
  MemManyDevice md{(hipStream_t)stream, "zkir_tape_sections_stage_launch"};
  TapeManyDevice td{md};
  const int rc = zkir::tape_sections_stage(md.who, td.stage(), hash_secs, hash_words, wide_secs, wide_words, n_real, code_end, alphas, lambdas, n, hash_verdicts, wide_verdicts, digests, sums);
  zkir::verify_note_tapes(td.n_check + td.n_wide, td.launches, td.uploaded_words);
  return rc;
}

}  // extern "C"
