// mem_stage.inl — the device forms of the verifier's three MEMORY stages (verify_stages.h: MemStages) over the touched-cell section of a mode-3 / mode-4 proof, the
// stand-alone entries zkir_mem_section_check_launch / zkir_mem_table_side_launch, and what zkir_verify_memory_device / zkir_verify_rate_memory_device (stark_verify.inl,
// pcs_verify.inl) run their fronts with.  Included by stark_prove.inl at file scope, behind verify_device.inl: the stages share that file's per-device block, mutex and
// pinned staging, and the section's chunk digests are section_hash_kernel's.
//
// The section is [n] + 7 n words; a record is air::mem_cell_code's: [address limb 0] [limb 1] [time of the last access] [final bytes: four 16-bit pieces].  Records are 28
// bytes apart, so no record is 16-byte aligned: the kernels load words.
//
// UNTRUSTED INPUT, as in verify_device.inl: nothing goes to the device before the host has seen that 1 + 7 n words lie inside the proof behind the section's start, and
// every buffer and extent below is sized by that n.  The image bytes come from the part of the program blob that mem_image_of grants (the blob's own length bounds it).
// Allocation failures and exceptions become a return code.
namespace {

constexpr unsigned MEM_MAX_BLOCKS = 512;                       // the side kernel's grid cap: a thread takes its cells at a stride of the grid, the partial sums fit a fixed buffer
inline unsigned mem_grid(uint64_t n) { const uint64_t g = (n + NT - 1) / NT; return (unsigned)(g < MEM_MAX_BLOCKS ? g : MEM_MAX_BLOCKS); }

// air::mem_cell_code of every record, one cell per lane; *result = min over the failing cells of (cell << 8 | code) (the caller sets it to all ones: no cell fails).  One
// atomic per workgroup, on the codes gathered in LDS, as in hash_tape_check_kernel.
__global__ __launch_bounds__(NT) void mem_section_check_kernel(const uint32_t* __restrict__ sec, uint64_t n, int mode, uint64_t n_code, unsigned long long* __restrict__ result) {
  __shared__ unsigned long long smin;
  if (threadIdx.x == 0) smin = ~0ull;
  __syncthreads();
  const uint64_t k = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (k < n) {
    const uint32_t* c = sec + 1 + 7 * k;
    const int code = air::mem_cell_code(c, k ? c - 7 : nullptr, mode, n_code);
    if (code) atomicMin(&smin, (unsigned long long)((k << 8) | (unsigned)code));
  }
  __syncthreads();
  if (threadIdx.x == 0 && smin != ~0ull) atomicMin(result, smin);
}

// Per cell + 1 / (alpha - fp(cell, 0, image bytes)) - 1 / (alpha - fp(cell, t_last, final bytes)), fp over lk[LK_ALPHA], lk[LK_LAM ..] and TAG_MEM (mem_cell_den): two
// inversions a cell, one partial sum a workgroup.  image: the program's code + data bytes (loaded at 0x1000), image_len of them; a CHECKED section (limbs and pieces in range).
__global__ __launch_bounds__(NT) void mem_section_side_kernel(const uint32_t* __restrict__ sec, uint64_t n, const uint8_t* __restrict__ image, uint64_t image_len, const uint32_t* __restrict__ lk,
                                                               E4* __restrict__ partial) {
  E4 acc = bb::e_zero();
  for (uint64_t k = (uint64_t)blockIdx.x * NT + threadIdx.x; k < n; k += (uint64_t)gridDim.x * NT) {
    const uint32_t* c = sec + 1 + 7 * k;
    const uint64_t addr = (uint64_t)c[0] | ((uint64_t)c[1] << 20), fin = (uint64_t)c[3] | ((uint64_t)c[4] << 16) | ((uint64_t)c[5] << 32) | ((uint64_t)c[6] << 48);
    uint64_t img = 0;
    for (int b = 0; b < 8; b++) { const uint64_t x = addr + b; if (x >= 0x1000 && x - 0x1000 < image_len) img |= (uint64_t)image[x - 0x1000] << (8 * b); }
    acc = bb::e_add(acc, bb::e_sub(bb::e_inv_m(mem_cell_den(lk, addr, 0, img)), bb::e_inv_m(mem_cell_den(lk, addr, c[2], fin))));
  }
  block_sum_to(acc, partial + blockIdx.x);
}

// Sections below MEM_DEVICE_MIN_CELLS cells stay with the host stages: the device route costs a flat ~0.3 ms (an upload, three launches, three synchronisations) where the
// host's cost grows by ~0.7 us a cell, and the two cross between 384 cells (host 1.430 ms, device 1.495 ms) and 512 (1.525 / 1.495) — below that the device route loses by
// up to 0.3 ms, far outside the host form's spread of 0.05 ms (profiles/r24_verify_memory_device.txt, "small sections").  ZKIR_VERIFY_DEVICE_MIN_CELLS (read once per
// call) sets another threshold, 0 included, for measuring the routes against each other.  The count word that routes is the proof's own and unchecked: both routes give
// the same verdict, so it can choose the slower one and nothing else.
// The list entries (mem_stage_many.inl) apply the same threshold to the SUM of a batch's cells: their flat cost is of the same kind with one synchronisation fewer, and
// batches of 64-cell sections cross between 256 cells in all (4 proofs: host 4.159 ms, device 4.290 ms) and 512 (8 proofs: 8.101 / 8.027); from there on the device route
// wins by ~0.7 us a cell (64 proofs, 4096 cells: 64.03 / 61.22 ms) — profiles/r25_verify_many_memory.txt, "the routing crossing".
constexpr uint64_t MEM_DEVICE_MIN_CELLS = 512;
uint64_t verify_device_min_cells() { if (const char* e = getenv("ZKIR_VERIFY_DEVICE_MIN_CELLS")) { const long long v = atoll(e); if (v >= 0) return (uint64_t)v; } return MEM_DEVICE_MIN_CELLS; }

// where the stages' data lies, counted from a 256-byte aligned start: [section][image][lk][partials][check word][chunk digests]
struct MemLayout {
  size_t o_img, o_lk, o_part, o_check, o_dg, total;
  MemLayout(uint64_t n, uint64_t image_len) {
    const size_t words = 1 + 7 * (size_t)n;
    o_img = al256(words * 4); o_lk = o_img + al256((size_t)image_len + 8); o_part = o_lk + al256(air::N_LK * 4); o_check = o_part + al256((size_t)MEM_MAX_BLOCKS * sizeof(E4));
    o_dg = o_check + 256; total = o_dg + al256(16 * ((words + 511) / 512) + 16);
  }
};
// the two launches, on data already in device memory; each leaves its result in pinned staging and is read after the caller's synchronisation
int mem_check_enqueue(const uint32_t* d_sec, uint64_t n, int mode, uint64_t n_code, unsigned long long* d_result, zkir::HostPin& pin, hipStream_t s, const unsigned long long** out) {
  unsigned long long* hr = pin.take_n<unsigned long long>(1);
  if (!hr) HIP_OK(hipErrorOutOfMemory);
  HIP_OK(hipMemsetAsync(d_result, 0xFF, 8, s));
  hipLaunchKernelGGL(mem_section_check_kernel, dim3(grid_for(n)), dim3(NT), 0, s, d_sec, n, mode, n_code, d_result);
  HIP_OK(hipMemcpyAsync(hr, d_result, 8, hipMemcpyDeviceToHost, s));
  *out = hr;
  return ZKIR_OK;
}
int mem_side_enqueue(const uint32_t* d_sec, uint64_t n, const uint8_t* d_image, uint64_t image_len, const uint32_t* d_lk, E4* d_part, zkir::HostPin& pin, hipStream_t s, TapePartials* out) {
  *out = TapePartials{};
  const unsigned g = mem_grid(n);
  E4* hp = pin.take_n<E4>(g);
  if (!hp) HIP_OK(hipErrorOutOfMemory);
  hipLaunchKernelGGL(mem_section_side_kernel, dim3(g), dim3(NT), 0, s, d_sec, n, d_image, image_len, d_lk, d_part);
  HIP_OK(hipMemcpyAsync(hp, d_part, (size_t)g * sizeof(E4), hipMemcpyDeviceToHost, s));
  out->h = hp; out->n = g;
  return ZKIR_OK;
}

// The device forms of the memory stages, at the START of the per-device block: a mode-4 proof's tape stages lay their data out behind this region (DeviceTapes::base), and a
// block that has to grow for them keeps the region's bytes (VerifyDevice::ensure).  An empty section and one below the threshold go to the host stages and touch no device
// memory.
struct DeviceMem {
  VerifyDevice& V; hipStream_t s; DeviceTapes* tapes;
  const uint64_t image_bound;                                   // no image is longer: the byte length of the blob the proof carries (zkir::stark_proof_blob_bytes)
  zkir::HostMem host; zkir::MemStages host_st;
  const uint64_t min_cells = verify_device_min_cells();
  bool dev = false;
  uint32_t stages_run = 0, launches = 0;
  uint64_t n = 0, uploaded_words = 0;
  size_t o_img = 0, o_lk = 0, o_part = 0, o_check = 0, o_dg = 0;
  DeviceMem(VerifyDevice& v, hipStream_t st, DeviceTapes* t, uint64_t bound) : V(v), s(st), tapes(t), image_bound(bound), host_st(zkir::host_mem_stages(&host)) {}

  int upload(size_t off, const void* src, size_t bytes) {
    if (!bytes) return ZKIR_OK;
    void* h = V.pin.take(bytes);
    if (!h) HIP_OK(hipErrorOutOfMemory);
    memcpy(h, src, bytes);
    HIP_OK(hipMemcpyAsync(V.d + off, h, bytes, hipMemcpyHostToDevice, s));
    uploaded_words += (bytes + 3) / 4;
    return ZKIR_OK;
  }
  int check(const uint32_t* sec, size_t avail, int mode, uint64_t code_words, size_t* used) {
    // (4: the host's own answer, before anything is sized by the count word)
    if (avail < 1 || sec[0] == 0 || sec[0] > (1u << 28) || (avail - 1) / 7 < sec[0] || sec[0] < min_cells) return host_st.check(&host, sec, avail, mode, code_words, used);
    n = sec[0];
    const size_t words = 1 + 7 * (size_t)n;
    const MemLayout L(n, image_bound);
    o_img = L.o_img; o_lk = L.o_lk; o_part = L.o_part; o_check = L.o_check; o_dg = L.o_dg;
    int rc = V.ensure(L.total); if (rc) return -rc;
    stages_run++;
    rc = upload(0, sec, words * 4); if (rc) return -rc;
    const unsigned long long* hr = nullptr;
    rc = mem_check_enqueue((const uint32_t*)V.d, n, mode, code_words, (unsigned long long*)(V.d + L.o_check), V.pin, s, &hr); if (rc) return -rc;
    launches++;
    if (hipStreamSynchronize(s) != hipSuccess || check_launch("zkir_verify_memory_device: cell checks") != ZKIR_OK) return -ZKIR_ERR_DEVICE;
    if (*hr != ~0ull) return (int)(*hr & 0xFF);
    dev = true; *used = words;
    if (tapes) tapes->base = L.total;                           // (the section stays where it is: the tape stages lay their data out behind this region)
    return 0;
  }
  int digests(const uint32_t* sec, size_t len, uint32_t* dg) {
    if (!dev) return host_st.digests(&host, sec, len, dg);
    if (len != 1 + 7 * (size_t)n) return -ZKIR_ERR_DEVICE;       // (the checked section, whole)
    stages_run++;
    const size_t n_chunks = (len + 511) / 512;
    uint32_t* h = V.pin.take_n<uint32_t>(4 * n_chunks);
    if (!h) return -ZKIR_ERR_DEVICE;
    uint32_t* d_dg = (uint32_t*)(V.d + o_dg);
    hipLaunchKernelGGL(section_hash_kernel, dim3((unsigned)((4 * n_chunks + 63) / 64)), dim3(64), 0, s, V.d_p2, (const uint32_t*)V.d, (uint64_t)len, d_dg);
    launches++;
    if (hipMemcpyAsync(h, d_dg, 16 * n_chunks, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess || check_launch("zkir_verify_memory_device: section digests") != ZKIR_OK) return -ZKIR_ERR_DEVICE;
    memcpy(dg, h, 16 * n_chunks);
    return 0;
  }
  int side(const uint32_t* lk_m, const uint8_t* blob, size_t blob_len, uint32_t T[4]) {
    if (!dev) return host_st.side(&host, lk_m, blob, blob_len, T);
    stages_run++;
    uint64_t il = 0;
    const uint8_t* image = zkir::mem_image_of(blob, blob_len, &il);
    if (il > image_bound) { zkir::set_last_error({ZKIR_ERR_OTHER, "zkir_verify_memory_device: the program image is larger than the blob the proof's header states"}); return -ZKIR_ERR_OTHER; }
    int rc = upload(o_img, image, (size_t)il); if (rc) return -rc;
    rc = upload(o_lk, lk_m, air::N_LK * 4); if (rc) return -rc;
    TapePartials mp;
    rc = mem_side_enqueue((const uint32_t*)V.d, n, V.d + o_img, il, (const uint32_t*)(V.d + o_lk), (E4*)(V.d + o_part), V.pin, s, &mp); if (rc) return -rc;
    launches++;
    if (hipStreamSynchronize(s) != hipSuccess || check_launch("zkir_verify_memory_device: memory table side") != ZKIR_OK) return -ZKIR_ERR_DEVICE;
    E4 t = bb::e_zero(); mp.add_to(t);
    memcpy(T, t.c, 16);
    return 0;
  }
};
int dm_check(void* p, const uint32_t* sec, size_t avail, int mode, uint64_t code_words, size_t* used) { return guarded([&] { return static_cast<DeviceMem*>(p)->check(sec, avail, mode, code_words, used); }); }
int dm_digests(void* p, const uint32_t* sec, size_t len, uint32_t* dg) { return guarded([&] { return static_cast<DeviceMem*>(p)->digests(sec, len, dg); }); }
int dm_side(void* p, const uint32_t* lk_m, const uint8_t* blob, size_t blob_len, uint32_t T[4]) { return guarded([&] { return static_cast<DeviceMem*>(p)->side(lk_m, blob, blob_len, T); }); }

// The front of a mode-3 / mode-4 verification with the memory stages (and a mode-4 proof's tape stages) on the current device, under the device state's mutex:
// front(tapes or NULL, mem) is the verifier's call.  *stages_run: the stages that ran on the device; the thread's zkir_verify_memory_last record is noted by the caller
// from *cells / *launches / *uploaded (the verifier's own clock resets it when it returns).
struct MemRunNote { uint32_t stages_run = 0, launches = 0; uint64_t cells = 0, uploaded_words = 0; };
template <class F> int with_memory_stages(const uint32_t* proof, uint64_t proof_words, void* stream, const char* who, F&& front, MemRunNote* note) {
  *note = MemRunNote{};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { zkir::set_last_error({ZKIR_ERR_DEVICE, std::string(who) + ": no current HIP device"}); return -ZKIR_ERR_DEVICE; }
  VerifyDevice* Vp = nullptr;
  const int src = guarded([&] { Vp = &verify_device(dev); return 0; });
  if (src) return src;
  VerifyDevice& V = *Vp;
  std::lock_guard<std::mutex> lock(V.mu);
  V.pin.reset();
  DeviceTapes dt(V, (hipStream_t)stream);
  DeviceMem dm(V, (hipStream_t)stream, proof[9] == 4 ? &dt : nullptr, zkir::stark_proof_blob_bytes(proof, proof_words));
  const zkir::TapeStages tapes{&dt, dt_hash_check, dt_wide_check, dt_digests, dt_hash_side, dt_wide_side};
  const zkir::MemStages mem{&dm, dm_check, dm_digests, dm_side};
  const int rc = guarded([&] { return front(proof[9] == 4 ? &tapes : nullptr, &mem); });
  if (dt.stages_run || dm.stages_run) (void)hipStreamSynchronize((hipStream_t)stream);      // (a verdict reached before a stage's own synchronisation: nothing of this call stays in flight)
  note->stages_run = dt.stages_run + dm.stages_run; note->launches = dm.launches; note->uploaded_words = dm.uploaded_words;
  note->cells = dm.stages_run ? dm.n : 0;
  return rc;
}
inline bool has_memory_section(const uint32_t* proof, uint64_t proof_words) { return proof && proof_words >= 10 && (proof[9] == 3 || proof[9] == 4); }

}  // namespace

extern "C" {

int zkir_mem_section_check_launch(const uint32_t* sec, uint64_t n_words, uint32_t mode, uint64_t code_words, int32_t* verdict, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!verdict || (!sec && n_words)) return tape_refuse("zkir_mem_section_check_launch: null argument");
  if (n_words < 1 || sec[0] > (1u << 28) || (n_words - 1) / 7 < sec[0]) { *verdict = 4; return ZKIR_OK; }
  const uint64_t n = sec[0];
  *verdict = 0;
  if (!n) return ZKIR_OK;                                        // (nothing to launch)
  try {
    const MemLayout L(n, 0);
    TapeDevMem dm;
    HIP_OK(hipMalloc(&dm.p, L.total));
    unsigned char* d = (unsigned char*)dm.p;
    zkir::HostPin pin;
    void* h = pin.take((1 + 7 * (size_t)n) * 4);
    if (!h) HIP_OK(hipErrorOutOfMemory);
    memcpy(h, sec, (1 + 7 * (size_t)n) * 4);
    HIP_OK(hipMemcpyAsync(d, h, (1 + 7 * (size_t)n) * 4, hipMemcpyHostToDevice, s));
    const unsigned long long* hr = nullptr;
    const int rc = mem_check_enqueue((const uint32_t*)d, n, (int)mode, code_words, (unsigned long long*)(d + L.o_check), pin, s, &hr);
    if (rc) return rc;
    HIP_OK(hipStreamSynchronize(s));
    if (check_launch("zkir_mem_section_check_launch") != ZKIR_OK) return ZKIR_ERR_DEVICE;
    if (*hr != ~0ull) *verdict = (int32_t)(*hr & 0xFF);
  } catch (const std::exception& e) { zkir::set_last_error({ZKIR_ERR_OTHER, std::string("zkir_mem_section_check_launch: ") + e.what()}); return ZKIR_ERR_OTHER; }
  return ZKIR_OK;
}

int zkir_mem_table_side_launch(const uint32_t* sec, uint64_t n_words, const uint8_t* blob, size_t blob_len, const uint32_t alpha[4], const uint32_t lambda[4], uint32_t sum[4], void* stream) {
  hipStream_t s = (hipStream_t)stream;
  uint32_t lk[air::N_LK];
  uint64_t n = 0;
  if (const char* why = zkir::mem_side_args(sec, n_words, blob, blob_len, alpha, lambda, sum, lk, &n)) return tape_refuse(std::string("zkir_mem_table_side_launch: ") + why);
  if (!n) { sum[0] = sum[1] = sum[2] = sum[3] = 0; return ZKIR_OK; }      // (nothing to launch)
  try {
    uint64_t il = 0;
    const uint8_t* image = zkir::mem_image_of(blob, blob_len, &il);
    const MemLayout L(n, il);
    TapeDevMem dm;
    HIP_OK(hipMalloc(&dm.p, L.total));
    unsigned char* d = (unsigned char*)dm.p;
    zkir::HostPin pin;
    auto up = [&](size_t off, const void* src, size_t bytes) -> hipError_t {
      if (!bytes) return hipSuccess;
      void* h = pin.take(bytes);
      if (!h) return hipErrorOutOfMemory;
      memcpy(h, src, bytes);
      return hipMemcpyAsync(d + off, h, bytes, hipMemcpyHostToDevice, s);
    };
    HIP_OK(up(0, sec, (size_t)n_words * 4)); HIP_OK(up(L.o_img, image, (size_t)il)); HIP_OK(up(L.o_lk, lk, sizeof lk));
    // the records must be what the kernel takes them for (limbs and pieces in range, strictly increasing addresses): check 54, with no code segment
    const unsigned long long* hr = nullptr;
    int rc = mem_check_enqueue((const uint32_t*)d, n, 3, 0, (unsigned long long*)(d + L.o_check), pin, s, &hr);
    if (rc) return rc;
    HIP_OK(hipStreamSynchronize(s));
    if (check_launch("zkir_mem_table_side_launch: cell checks") != ZKIR_OK) return ZKIR_ERR_DEVICE;
    if (*hr != ~0ull) return tape_refuse("zkir_mem_table_side_launch: the section's cells are not in range and strictly increasing");
    TapePartials mp;
    rc = mem_side_enqueue((const uint32_t*)d, n, d + L.o_img, il, (const uint32_t*)(d + L.o_lk), (E4*)(d + L.o_part), pin, s, &mp);
    if (rc) return rc;
    HIP_OK(hipStreamSynchronize(s));
    if (check_launch("zkir_mem_table_side_launch") != ZKIR_OK) return ZKIR_ERR_DEVICE;
    E4 T = bb::e_zero(); mp.add_to(T);
    T = bb::e_from_mont(T);
    memcpy(sum, T.c, 16);
  } catch (const std::exception& e) { zkir::set_last_error({ZKIR_ERR_OTHER, std::string("zkir_mem_table_side_launch: ") + e.what()}); return ZKIR_ERR_OTHER; }
  return ZKIR_OK;
}

}  // extern "C"
