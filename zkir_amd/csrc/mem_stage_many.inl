// mem_stage_many.inl — the device form of the memory stages over a LIST of proofs (verify_stages.h: MemManyStage) and the stand-alone entry zkir_mem_sections_stage_launch:
// what zkir_verify_many_memory_device (stark_verify.inl) and zkir_verify_rate_many_memory_device (pcs_verify_many.inl) run their fronts with.  Included by stark_prove.inl at
// file scope, behind mem_stage.inl: the per-device block, its mutex and pinned staging are verify_device.inl's, the cell rules and the sponge are mem_stage.inl's and
// section_hash_kernel's.
//
// The answer to "many small shapes" is query_stage.inl's: a per-section RECORD in device memory, one staged upload per phase, a fixed number of launches and one
// synchronisation per phase, however many sections.  Phase A (prepare: before any front) uploads every located section once and runs ONE check launch and ONE digest launch
// over all of them; phase B (side: behind the last front) uploads the deferred proofs' lookup parameters and program images and runs ONE side launch over their cells, which
// are still resident.  Between the phases a mode-4 proof's tape stages lay their data out BEHIND the batch region (DeviceTapes::base; VerifyDevice::ensure keeps the region
// when the block grows), and the stage holds the device state's mutex from prepare to done.
//
// UNTRUSTED INPUT, as in mem_stage.inl: a section comes here only after the host has seen that 1 + 7 n words lie inside its proof (zkir::MemSection), every extent is sized
// by those words, the upload is bounded by the proofs the caller holds, and an image by the blob its proof carries.  The check and digest kernels run on UNCHECKED words
// (phase A precedes the front's word-range scan): air::mem_cell_code and the sponge take any 32-bit word.  The side kernel runs only on sections whose check returned 0 and
// whose front passed the scan.  Allocation failures and exceptions become a negative return.
#include <optional>

namespace {

// A section's record, 8 words of device memory.  Offsets count words of the block; a section starts on 256 bytes.
constexpr uint32_t MS_OFF = 0, MS_N = 1, MS_MODE = 2, MS_CODE = 3, MS_WG0 = 4, MS_CHUNK0 = 5, MS_WORDS = 8;      // phase A: the first workgroup of the check launch, the first chunk
constexpr uint32_t MJ_OFF = 0, MJ_N = 1, MJ_WG0 = 2, MJ_NWG = 3, MJ_IMG = 4, MJ_IMG_LEN = 5, MJ_LK = 6;          // phase B: the first workgroup = the first partial sum; image, lk: words of the block

// the record an id belongs to: the largest i < n with rec[i][field] <= id (record 0's is 0, the field rises; a record with an empty range is never found)
__device__ __forceinline__ uint32_t mem_record_of(const uint32_t* __restrict__ recs, uint32_t field, uint32_t n, uint32_t id) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (recs[MS_WORDS * mid + field] <= id) lo = mid; else hi = mid; }
  return lo;
}

// mem_section_check_kernel over all sections: a workgroup belongs to ONE section (uniform lookup), one cell per lane; cell 0 of a section has no predecessor.
// results[i] = min over section i's failing cells of (cell << 8 | code) (the caller sets them to all ones), one atomic per workgroup.
__global__ __launch_bounds__(NT) void mem_sections_check_kernel(const uint32_t* __restrict__ blk, const uint32_t* __restrict__ recs, uint32_t n_sec, unsigned long long* __restrict__ results) {
  __shared__ unsigned long long smin;
  if (threadIdx.x == 0) smin = ~0ull;
  __syncthreads();
  const uint32_t i = mem_record_of(recs, MS_WG0, n_sec, blockIdx.x);
  const uint32_t* r = recs + MS_WORDS * i;
  const uint32_t* sec = blk + r[MS_OFF];
  const uint64_t n = r[MS_N], k = (uint64_t)(blockIdx.x - r[MS_WG0]) * NT + threadIdx.x;
  if (k < n) {
    const uint32_t* c = sec + 1 + 7 * k;
    const int code = air::mem_cell_code(c, k ? c - 7 : nullptr, (int)r[MS_MODE], (uint64_t)r[MS_CODE]);
    if (code) atomicMin(&smin, (unsigned long long)((k << 8) | (unsigned)code));
  }
  __syncthreads();
  if (threadIdx.x == 0 && smin != ~0ull) atomicMin(results + i, smin);
}

// section_hash_kernel's quad-per-chunk sponge over all sections' chunks: chunk c is chunk c - chunk0 of its section, a section's ragged last chunk ends at that section's
// end, and the digests of section i lie at 4 chunk0 (chunks are numbered section after section).
__global__ __launch_bounds__(64) void mem_sections_hash_kernel(const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ blk, const uint32_t* __restrict__ recs, uint32_t n_sec, uint32_t n_chunks,
                                                               uint32_t* __restrict__ digests) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x, c = t >> 2;
  const int l = (int)(t & 3);
  if (c >= n_chunks) return;                                     // whole quads leave together
  const uint32_t i = mem_record_of(recs, MS_CHUNK0, n_sec, c);
  const uint32_t* r = recs + MS_WORDS * i;
  const uint64_t n_words = 1 + 7 * (uint64_t)r[MS_N], at = (uint64_t)(c - r[MS_CHUNK0]) * SECTION_CHUNK;
  const uint32_t* w = blk + r[MS_OFF] + at;
  const uint64_t len = n_words - at < SECTION_CHUNK ? n_words - at : SECTION_CHUNK;
  uint32_t st[3] = {0, 0, 0};
  const uint32_t k_in = cp->in_scale, carry = cp->carry;
  for (uint64_t off = 0; off < len; off += p2::RATE) {           // (a word the ragged last block does not overwrite stays: so::hash_elems)
    st[0] = off + l < len ? bb::mont_mul_lazy(w[off + l], k_in) : bb::mont_mul_lazy(st[0], carry);
    st[1] = off + 4 + l < len ? bb::mont_mul_lazy(w[off + 4 + l], k_in) : bb::mont_mul_lazy(st[1], carry);
    st[2] = bb::mont_mul_lazy(st[2], carry);
    p2::permute_quad_scaled(st, l, *cp);
  }
  digests[4 * c + l] = bb::mont_mul(st[0], cp->out_scale);
}

// mem_section_side_kernel over the deferred proofs' sections: job j has its own lk, image and MJ_NWG = min(ceil(n / NT), MEM_MAX_BLOCKS) workgroups that stride over its
// cells; one partial sum per workgroup, job j's at partial[MJ_WG0 ..].
__global__ __launch_bounds__(NT) void mem_sections_side_kernel(const uint32_t* __restrict__ blk, const uint32_t* __restrict__ jobs, uint32_t n_jobs, E4* __restrict__ partial) {
  const uint32_t j = mem_record_of(jobs, MJ_WG0, n_jobs, blockIdx.x);
  const uint32_t* r = jobs + MS_WORDS * j;
  const uint32_t* sec = blk + r[MJ_OFF];
  const uint32_t* lk = blk + r[MJ_LK];
  const uint8_t* image = (const uint8_t*)(blk + r[MJ_IMG]);
  const uint64_t n = r[MJ_N], image_len = r[MJ_IMG_LEN], stride = (uint64_t)r[MJ_NWG] * NT;
  E4 acc = bb::e_zero();
  for (uint64_t k = (uint64_t)(blockIdx.x - r[MJ_WG0]) * NT + threadIdx.x; k < n; k += stride) {
    const uint32_t* c = sec + 1 + 7 * k;
    const uint64_t addr = (uint64_t)c[0] | ((uint64_t)c[1] << 20), fin = (uint64_t)c[3] | ((uint64_t)c[4] << 16) | ((uint64_t)c[5] << 32) | ((uint64_t)c[6] << 48);
    uint64_t img = 0;
    for (int b = 0; b < 8; b++) { const uint64_t x = addr + b; if (x >= 0x1000 && x - 0x1000 < image_len) img |= (uint64_t)image[x - 0x1000] << (8 * b); }
    acc = bb::e_add(acc, bb::e_sub(bb::e_inv_m(mem_cell_den(lk, addr, 0, img)), bb::e_inv_m(mem_cell_den(lk, addr, c[2], fin))));
  }
  block_sum_to(acc, partial + blockIdx.x);
}

// The device form of the list stage and of a mode-4 proof's tape stages between its phases (zkir::TapeStagesFor).  The batch region starts the per-device block:
// [records][sections, each on 256 bytes][result words][chunk digests]; phase B's data lies behind it: [job records][images][lk slots][partial sums].
struct MemManyDevice {
  hipStream_t s; const char* who;
  VerifyDevice* V = nullptr;
  std::unique_lock<std::mutex> lock;                             // held from prepare to done
  std::unique_lock<std::mutex> proof_lock;                       // a mode-4 front of a batch that stayed on the host: held for that front, as zkir_verify_rate_many_device does
  size_t region = 0;
  std::vector<uint32_t> sec_off;                                 // where section i lies (words of the block)
  uint32_t launches = 0, tape_stages = 0;
  bool tape_inflight = false;                                    // (tape_stage_many.inl) the tape list stage's byte kernels may still be writing the block
  uint64_t uploaded_words = 0;
  std::optional<DeviceTapes> dt;
  zkir::TapeStages tapes{};

  int refuse(const char* what, int code = ZKIR_ERR_OTHER) { zkir::set_last_error({code, std::string(who) + ": " + what}); return -code; }
  int device() {
    if (V) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return refuse("no current HIP device", ZKIR_ERR_DEVICE);
    V = &verify_device(dev);
    return 0;
  }
  int prepare(const zkir::MemSection* list, uint32_t n, int* verdicts, uint32_t* digests) {
    if (!n) return 0;
    if (const int rc = device()) return rc;
    lock = std::unique_lock<std::mutex>(V->mu);
    V->pin.reset();
    // ---- the layout ----
    std::vector<uint32_t> recs((size_t)n * MS_WORDS, 0);
    sec_off.assign(n, 0);
    size_t at = al256((size_t)n * MS_WORDS * 4);
    uint64_t wg = 0, chunks = 0;
    for (uint32_t i = 0; i < n; i++) {
      const zkir::MemSection& S = list[i];
      if (S.n > (1u << 28) || S.code_words >> 32) return refuse("a section description is not a located section's");
      uint32_t* r = recs.data() + (size_t)i * MS_WORDS;
      sec_off[i] = (uint32_t)(at / 4);
      r[MS_OFF] = sec_off[i]; r[MS_N] = (uint32_t)S.n; r[MS_MODE] = (uint32_t)S.mode; r[MS_CODE] = (uint32_t)S.code_words; r[MS_WG0] = (uint32_t)wg; r[MS_CHUNK0] = (uint32_t)chunks;
      at += al256((1 + 7 * (size_t)S.n) * 4);
      wg += (S.n + NT - 1) / NT; chunks += zkir::mem_section_chunks(S.n);
      if ((at >> 33) || (wg >> 31) || (chunks >> 29)) return refuse("the batch's sections are too large for one block");
    }
    const size_t o_res = at, o_dg = o_res + al256((size_t)n * 8), total = o_dg + al256(16 * (size_t)chunks);
    if (total >> 33) return refuse("the batch's sections are too large for one block");
    // ---- one staged upload, two launches, one download, one synchronisation ----
    int rc = V->ensure(total); if (rc) return -rc;
    unsigned char* h = (unsigned char*)V->pin.take(o_res);
    unsigned char* hr = (unsigned char*)V->pin.take(total - o_res);
    if (!h || !hr) return refuse("no pinned host memory", ZKIR_ERR_DEVICE);
    memcpy(h, recs.data(), recs.size() * 4);
    for (uint32_t i = 0; i < n; i++) memcpy(h + 4 * (size_t)sec_off[i], list[i].sec, (1 + 7 * (size_t)list[i].n) * 4);
    if (hipMemcpyAsync(V->d, h, o_res, hipMemcpyHostToDevice, s) != hipSuccess || hipMemsetAsync(V->d + o_res, 0xFF, (size_t)n * 8, s) != hipSuccess) { (void)check_launch(who); return -ZKIR_ERR_DEVICE; }
    uploaded_words += o_res / 4;
    const uint32_t* d_blk = (const uint32_t*)V->d;
    if (wg) { hipLaunchKernelGGL(mem_sections_check_kernel, dim3((unsigned)wg), dim3(NT), 0, s, d_blk, d_blk, n, (unsigned long long*)(V->d + o_res)); launches++; }
    hipLaunchKernelGGL(mem_sections_hash_kernel, dim3((unsigned)((4 * chunks + 63) / 64)), dim3(64), 0, s, V->d_p2, d_blk, d_blk, n, (uint32_t)chunks, (uint32_t*)(V->d + o_dg));
    launches++;
    if (hipMemcpyAsync(hr, V->d + o_res, total - o_res, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess || check_launch(who) != ZKIR_OK) return -ZKIR_ERR_DEVICE;
    // (the staging is the next stage's from here on: the answers go to the caller's vectors)
    const unsigned long long* res = (const unsigned long long*)hr;
    for (uint32_t i = 0; i < n; i++) verdicts[i] = res[i] == ~0ull ? 0 : (int)(res[i] & 0xFF);
    memcpy(digests, hr + (o_dg - o_res), 16 * (size_t)chunks);
    region = total;
    return 0;
  }
  int side(const zkir::MemSection* list, const zkir::MemSideJob* jobs, uint32_t n_jobs, uint32_t* sums) {
    if (!n_jobs) return 0;
    if (!lock.owns_lock() || !region) return refuse("the table side was asked for before the sections went up");
    V->pin.reset();
    std::vector<uint32_t> recs((size_t)n_jobs * MS_WORDS, 0);
    std::vector<const uint8_t*> images(n_jobs, nullptr);
    size_t at = region + al256((size_t)n_jobs * MS_WORDS * 4);
    uint64_t wg = 0;
    for (uint32_t j = 0; j < n_jobs; j++) {
      const zkir::MemSideJob& J = jobs[j];
      if (J.section >= sec_off.size()) return refuse("a table-side job names no section of the batch");
      uint64_t il = 0;
      images[j] = zkir::mem_image_of(J.blob, J.blob_len, &il);
      uint32_t* r = recs.data() + (size_t)j * MS_WORDS;
      const uint64_t n = list[J.section].n;
      r[MJ_OFF] = sec_off[J.section]; r[MJ_N] = (uint32_t)n; r[MJ_WG0] = (uint32_t)wg; r[MJ_NWG] = mem_grid(n);
      r[MJ_IMG] = (uint32_t)(at / 4); r[MJ_IMG_LEN] = (uint32_t)il; at += al256((size_t)il + 8);
      r[MJ_LK] = (uint32_t)(at / 4); at += al256(air::N_LK * 4);
      wg += r[MJ_NWG];
      if ((il >> 32) || (at >> 33)) return refuse("the batch's program images are too large for one block");
    }
    const size_t o_part = at, total = o_part + al256((size_t)wg * sizeof(E4));
    if (total >> 33) return refuse("the batch's program images are too large for one block");
    if (total > V->cap && tape_inflight) { if (hipStreamSynchronize(s) != hipSuccess) return -ZKIR_ERR_DEVICE; tape_inflight = false; }      // (a larger block is a copy of this one)
    int rc = V->ensure(total, region); if (rc) return -rc;
    unsigned char* h = (unsigned char*)V->pin.take(o_part - region);
    E4* hp = wg ? V->pin.take_n<E4>((size_t)wg) : nullptr;
    if (!h || (wg && !hp)) return refuse("no pinned host memory", ZKIR_ERR_DEVICE);
    memcpy(h, recs.data(), recs.size() * 4);
    for (uint32_t j = 0; j < n_jobs; j++) {
      const uint32_t* r = recs.data() + (size_t)j * MS_WORDS;
      if (r[MJ_IMG_LEN]) memcpy(h + (4 * (size_t)r[MJ_IMG] - region), images[j], r[MJ_IMG_LEN]);
      memcpy(h + (4 * (size_t)r[MJ_LK] - region), jobs[j].lk_m, air::N_LK * 4);
    }
    if (hipMemcpyAsync(V->d + region, h, o_part - region, hipMemcpyHostToDevice, s) != hipSuccess) { (void)check_launch(who); return -ZKIR_ERR_DEVICE; }
    uploaded_words += (o_part - region) / 4;
    if (!wg) { memset(sums, 0, 16 * (size_t)n_jobs); return hipStreamSynchronize(s) == hipSuccess ? 0 : -ZKIR_ERR_DEVICE; }      // (only empty sections: nothing to launch)
    hipLaunchKernelGGL(mem_sections_side_kernel, dim3((unsigned)wg), dim3(NT), 0, s, (const uint32_t*)V->d, (const uint32_t*)(V->d + region), n_jobs, (E4*)(V->d + o_part));
    launches++;
    if (hipMemcpyAsync(hp, V->d + o_part, (size_t)wg * sizeof(E4), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess || check_launch(who) != ZKIR_OK) return -ZKIR_ERR_DEVICE;
    for (uint32_t j = 0; j < n_jobs; j++) {
      const uint32_t* r = recs.data() + (size_t)j * MS_WORDS;
      E4 t = bb::e_zero();
      for (uint32_t b = 0; b < r[MJ_NWG]; b++) t = bb::e_add(t, hp[r[MJ_WG0] + b]);
      memcpy(sums + 4 * (size_t)j, t.c, 16);
    }
    return 0;
  }
  void done() {                                                  // nothing of the batch stays in flight, in the block or in the staging: the query stage lays its data out from offset 0
    if (lock.owns_lock()) { if (launches) (void)hipStreamSynchronize(s); region = 0; lock.unlock(); }
  }
  // a mode-4 proof's tape stages: behind the batch region while the stage holds the mutex, else under the mutex for this front alone
  const zkir::TapeStages* begin(uint32_t) {
    if (device()) return nullptr;
    if (!lock.owns_lock()) proof_lock = std::unique_lock<std::mutex>(V->mu);
    V->pin.reset();
    dt.emplace(*V, s);
    dt->base = lock.owns_lock() ? region : 0;
    tapes = zkir::TapeStages{&*dt, dt_hash_check, dt_wide_check, dt_digests, dt_hash_side, dt_wide_side};
    return &tapes;
  }
  int end(int rc) {
    if (dt) { if (dt->stages_run) (void)hipStreamSynchronize(s); tape_stages += dt->stages_run; dt.reset(); }
    if (proof_lock.owns_lock()) proof_lock.unlock();
    return rc;
  }
  zkir::MemManyStage stage() {
    return zkir::MemManyStage{this,
      [](void* p, const zkir::MemSection* list, uint32_t n, int* verdicts, uint32_t* digests) { return guarded([&] { return static_cast<MemManyDevice*>(p)->prepare(list, n, verdicts, digests); }); },
      [](void* p, const zkir::MemSection* list, const zkir::MemSideJob* jobs, uint32_t n_jobs, uint32_t* sums) { return guarded([&] { return static_cast<MemManyDevice*>(p)->side(list, jobs, n_jobs, sums); }); },
      [](void* p) { static_cast<MemManyDevice*>(p)->done(); }};
  }
  zkir::TapeStagesFor tapes_for() {
    return zkir::TapeStagesFor{this, [](void* p, uint32_t i) { return static_cast<MemManyDevice*>(p)->begin(i); }, [](void* p, int rc) { return static_cast<MemManyDevice*>(p)->end(rc); }};
  }
};

}  // namespace

extern "C" {

int zkir_mem_sections_stage_launch(const uint32_t* const* secs, const uint64_t* n_words, const uint32_t* modes, const uint64_t* code_words, const uint8_t* const* blobs, const size_t* blob_lens,
                                   const uint32_t* alphas, const uint32_t* lambdas, uint32_t n, int32_t* verdicts, uint32_t* digests, uint32_t* sums, void* stream) {
  MemManyDevice md{(hipStream_t)stream, "zkir_mem_sections_stage_launch"};
  return zkir::mem_sections_stage(md.who, md.stage(), secs, n_words, modes, code_words, blobs, blob_lens, alphas, lambdas, n, verdicts, digests, sums);
}

}  // extern "C"
