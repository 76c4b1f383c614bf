// verify_device.inl — zkir_hash_tape_new_bytes_{launch,host} and zkir_verify_device (include/zkir_amd.h): the device forms of the verifier's three tape stages
// (verify_stages.h) around the kernels of tape_table.inl / tape_digest.inl and section_hash_kernel.  Included by stark_prove.inl at file scope.
//
// UNTRUSTED INPUT: every buffer and every kernel extent below is sized by how many words the PROOF holds behind the section's start — hash_tape_walk stops at the buffer's
// end and derives each record's cell count from the record's own fields, the wide section's count is checked against the proof's length by verify.cpp before the stage
// runs — never by a count word alone.  Allocation failures and exceptions become a return code.
#include <map>

namespace {

// What zkir_verify_device keeps between calls, ONE PER HIP DEVICE (calls on a device are serialised): its device block, its pinned staging and the Poseidon2
// constants, all allocated while that device is current.  hipMalloc and hipHostMalloc of a 135 MB tape cost more than the stages themselves.  Never destroyed: the HIP
// runtime may be gone when static destructors run.
struct VerifyDevice {
  std::mutex mu;
  unsigned char* d = nullptr; size_t cap = 0;
  p2::Consts* d_p2 = nullptr;
  zkir::HostPin pin;
  // keep: the first `keep` bytes of the block hold data AT REST (the memory stages' region, mem_stage.inl: its last use has been synchronised) that a larger block must still hold
  int ensure(size_t bytes, size_t keep = 0) {
    if (!d_p2) {
      p2::Consts k; p2::generate(k);
      HIP_OK(hipMalloc((void**)&d_p2, sizeof k));
      const hipError_t e = hipMemcpy(d_p2, &k, sizeof k, hipMemcpyHostToDevice);
      if (e != hipSuccess) { (void)hipFree(d_p2); d_p2 = nullptr; HIP_OK(e); }
    }
    if (bytes <= cap) return ZKIR_OK;
    if (d && keep) {
      unsigned char* nd = nullptr;
      HIP_OK(hipMalloc((void**)&nd, bytes));
      hipError_t e = hipMemcpy(nd, d, keep, hipMemcpyDeviceToDevice);
      if (e == hipSuccess) e = hipDeviceSynchronize();
      if (e != hipSuccess) { (void)hipFree(nd); HIP_OK(e); }
      (void)hipFree(d);
      d = nd; cap = bytes;
      return ZKIR_OK;
    }
    if (d) { (void)hipFree(d); d = nullptr; cap = 0; }
    HIP_OK(hipMalloc((void**)&d, bytes));
    cap = bytes;
    return ZKIR_OK;
  }
};
VerifyDevice& verify_device(int dev) {                           // the state of HIP device `dev`: a call made with another device current never touches this one's memory
  static std::mutex mu;
  static std::map<int, VerifyDevice*>* all = new std::map<int, VerifyDevice*>;
  std::lock_guard<std::mutex> lock(mu);
  VerifyDevice*& v = (*all)[dev];
  if (!v) v = new VerifyDevice;
  return *v;
}

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
// Every non-empty tape goes to the device: on a one-call tape (sha256_hello) the device route costs 0.08 ms more than the host's 6.42 ms, inside the host form's own
// spread of 0.19 ms, and from 675 calls on it is the faster one (profiles/r09_verify_device.txt, "routing") — so there is no built-in threshold.  For measuring the
// routes against each other, ZKIR_VERIFY_DEVICE_MIN_RECORDS (read once per call) leaves tapes with fewer records to the host stages.  The count word that routes is the
// proof's own and unchecked: both routes give the same verdict, so it can choose the slower one and nothing else.
uint64_t verify_device_min_records() { if (const char* e = getenv("ZKIR_VERIFY_DEVICE_MIN_RECORDS")) { const long long v = atoll(e); if (v >= 0) return (uint64_t)v; } return 0; }

// The device forms of the tape stages.  Layout of the block: [hash tape][prefix][side][hash list][wide section, its records 16-byte aligned][wide list][lk][partials]
// [check words][chunk digests][patches].
struct DeviceTapes {
  VerifyDevice& V; hipStream_t s;
  zkir::HostTapes host; zkir::TapeStages host_st;
  const uint64_t min_records = verify_device_min_records();
  bool hash_dev = false, wide_dev = false;
  uint32_t stages_run = 0;
  std::vector<uint64_t> prefix;
  const uint32_t* h_hash = nullptr;
  uint64_t n_calls = 0, H = 0, hash_words = 0, n_wide = 0;
  size_t o_prefix = 0, o_side = 0, o_hlist = 0, o_wide = 0, o_wlist = 0, o_lk = 0, o_part = 0, o_check = 0, o_dg = 0, o_patch = 0, patch_cap = 0;
  DeviceTapes(VerifyDevice& v, hipStream_t st) : V(v), s(st), host_st(zkir::host_tape_stages(&host)) {}
  size_t base = 0;                                               // bytes at the block's start that belong to the memory stages (mem_stage.inl; a multiple of 256): the layout starts behind them
  unsigned char* D() const { return V.d + base; }

  int upload(size_t off, const void* src, size_t bytes) {
    if (!bytes) return ZKIR_OK;
    void* h = V.pin.take(bytes);
    if (!h) HIP_OK(hipErrorOutOfMemory);
    constexpr size_t PIECE = (size_t)8 << 20;                   // (a 135 MB tape: the link moves piece k while the host stages piece k + 1)
    for (size_t at = 0; at < bytes; at += PIECE) {
      const size_t n = std::min(PIECE, bytes - at);
      memcpy((unsigned char*)h + at, (const unsigned char*)src + at, n);
      HIP_OK(hipMemcpyAsync(D() + off + at, (unsigned char*)h + at, n, hipMemcpyHostToDevice, s));
    }
    return ZKIR_OK;
  }
  int hash_check(const uint32_t* w, size_t avail, uint64_t n_real, uint64_t code_end, size_t* used) {
    if (avail < 1 || w[0] == 0 || w[0] > n_real || w[0] < min_records) return host_st.hash_check(&host, w, avail, n_real, code_end, used);
    prefix.resize((size_t)std::min<uint64_t>(w[0], avail / 8) + 2);
    const TapeWalk wk = hash_tape_walk(w, avail, prefix.data());
    const uint64_t n_check = wk.n_full + (wk.header_only ? 1 : 0), words = wk.used + (wk.header_only ? 8 : 0);
    unsigned long long best = wk.cut && !wk.header_only ? ((unsigned long long)wk.n_full << 8) | 4u : ~0ull;      // (the walk left the proof before record n_full's header)
    // everything the later stages need, sized by the walk (records that lie in the proof) and by the words behind the section (the wide tape's bound)
    const size_t wide_max = avail - (size_t)wk.used, n_chunks = (size_t)(wk.used + 511) / 512 + (wide_max + 511) / 512;
    o_prefix = al256(words * 4); o_side = o_prefix + al256((n_check + 1) * 8); o_hlist = o_side + al256(wk.cells * 8 + 8); o_wide = o_hlist + al256(n_check * sizeof(HashAux) + 32);
    o_wlist = o_wide + al256(wide_max * 4 + 16); o_lk = o_wlist + al256(wide_max / 8 * sizeof(HashAux) + 32); o_part = o_lk + al256(air::N_LK * 4);
    o_check = o_part + al256(2 * (size_t)TAPE_MAX_BLOCKS * sizeof(E4)); o_dg = o_check + 256; o_patch = o_dg + al256(16 * n_chunks + 16);
    patch_cap = al256((size_t)words / 16 + 64);                 // (a call the host hashes is above 1 KiB: at least 640 words of tape for its 80 bytes of patches)
    if (n_check) {
      int rc = V.ensure(base + o_patch + 2 * patch_cap + 256, base); if (rc) return -rc;
      stages_run++;
      rc = upload(0, w, words * 4); if (rc) return -rc;
      rc = upload(o_prefix, prefix.data(), n_check * 8); if (rc) return -rc;
      int dcode = 0; uint64_t dcall = ~0ull;
      rc = hash_tape_check_run((const uint32_t*)D(), (const uint64_t*)(D() + o_prefix), n_check, wk.n_full, n_real, code_end, (unsigned long long*)(D() + o_check), V.pin, s, &dcode, &dcall);
      if (rc) return -rc;
      if (check_launch("zkir_verify_device: record checks") != ZKIR_OK) return -ZKIR_ERR_DEVICE;
      if (dcode) best = std::min(best, ((unsigned long long)dcall << 8) | (unsigned)dcode);
    }
    if (best != ~0ull) return (int)(best & 0xFF);
    // every record is what the kernels take it for: the full prefix goes up and the new bytes are formed while the host goes on parsing
    hash_dev = true; h_hash = w; n_calls = wk.n_calls; H = wk.cells; hash_words = wk.used; *used = (size_t)wk.used;
    int rc = upload(o_prefix, prefix.data(), (n_calls + 1) * 8); if (rc) return -rc;
    hash_new_bytes_enqueue((const uint32_t*)D(), (const uint64_t*)(D() + o_prefix), n_calls, H, (uint64_t*)(D() + o_side), s);
    return 0;
  }
  int wide_check(const uint32_t* sec, size_t n, uint64_t n_real) {
    if (!n || n < min_records) return host_st.wide_check(&host, sec, n, n_real);
    if (!hash_dev) {                                            // (no hash call went up: the block holds the wide tape alone)
      o_wide = 0; o_wlist = al256((1 + 8 * n) * 4 + 16); o_lk = o_wlist + al256(n * sizeof(HashAux) + 32); o_part = o_lk + al256(air::N_LK * 4);
      o_check = o_part + al256(2 * (size_t)TAPE_MAX_BLOCKS * sizeof(E4)); o_dg = o_check + 256; o_patch = o_dg + al256(16 * ((1 + 8 * n + 511) / 512) + 16);
      const int rc = V.ensure(base + o_patch + 256, base); if (rc) return -rc;
    }
    stages_run++;
    n_wide = n; wide_dev = true;
    int rc = upload(o_wide + 12, sec, (1 + 8 * n) * 4); if (rc) return -rc;      // (the records behind the count word start on 16 bytes: wide_table_side_kernel loads uint4)
    uint32_t* hb = V.pin.take_n<uint32_t>(1);
    if (!hb) return -ZKIR_ERR_DEVICE;
    uint32_t* d_bad = (uint32_t*)(D() + o_check + 64);
    if (hipMemsetAsync(d_bad, 0, 4, s) != hipSuccess) return -ZKIR_ERR_DEVICE;
    hipLaunchKernelGGL(wide_tape_check_kernel, dim3(grid_for(n)), dim3(NT), 0, s, (const uint32_t*)(D() + o_wide + 16), (uint64_t)n, n_real, d_bad);
    if (hipMemcpyAsync(hb, d_bad, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess || check_launch("zkir_verify_device: wide record checks") != ZKIR_OK) return -ZKIR_ERR_DEVICE;
    return *hb ? 57 : 0;
  }
  int digests(int which, const uint32_t* sw, size_t sl, uint32_t* dg) {
    if (!(which ? wide_dev : hash_dev)) return host_st.digests(&host, which, sw, sl, dg);
    stages_run++;
    const size_t n_chunks = (sl + 511) / 512, at = which ? (size_t)(hash_dev ? (hash_words + 511) / 512 : 0) : 0;
    uint32_t* d_dg = (uint32_t*)(D() + o_dg) + 4 * at;
    uint32_t* h = V.pin.take_n<uint32_t>(4 * n_chunks);
    if (!h) return -ZKIR_ERR_DEVICE;
    hipLaunchKernelGGL(section_hash_kernel, dim3((unsigned)((4 * n_chunks + 63) / 64)), dim3(64), 0, s, V.d_p2, (const uint32_t*)(D() + (which ? o_wide + 12 : 0)), (uint64_t)sl, d_dg);
    if (hipMemcpyAsync(h, d_dg, 16 * n_chunks, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess || check_launch("zkir_verify_device: section digests") != ZKIR_OK) return -ZKIR_ERR_DEVICE;
    memcpy(dg, h, 16 * n_chunks);
    return 0;
  }
  int hash_side(const uint32_t* lk_m, uint32_t T[4]) {
    if (!hash_dev) return host_st.hash_side(&host, lk_m, T);
    stages_run++;
    int rc = upload(o_lk, lk_m, air::N_LK * 4); if (rc) return -rc;
    // the calls the lanes left out: hashed here while the device works, their output cells patched in before the table side reads them
    std::vector<uint64_t> idx, val;
    long_call_patches(h_hash, prefix.data(), n_calls, idx, val);
    if (!idx.empty()) {
      if (idx.size() * 8 > patch_cap) { zkir::set_last_error({ZKIR_ERR_OTHER, "zkir_verify_device: more long calls than the tape can hold"}); return -ZKIR_ERR_OTHER; }
      rc = upload(o_patch, idx.data(), idx.size() * 8); if (rc) return -rc;
      rc = upload(o_patch + patch_cap, val.data(), val.size() * 8); if (rc) return -rc;
      hipLaunchKernelGGL(side_patch_kernel, dim3(grid_for(idx.size())), dim3(NT), 0, s, (const uint64_t*)(D() + o_patch), (const uint64_t*)(D() + o_patch + patch_cap), (uint64_t)idx.size(),
                         (uint64_t*)(D() + o_side));
    }
    TapePartials hp;
    rc = hash_table_side_enqueue((const uint32_t*)D(), (const uint64_t*)(D() + o_prefix), (const uint64_t*)(D() + o_side), n_calls, H, (const uint32_t*)(D() + o_lk), (HashAux*)(D() + o_hlist),
                                 (E4*)(D() + o_part), V.pin, s, &hp);
    if (rc) return -rc;
    if (hipStreamSynchronize(s) != hipSuccess || check_launch("zkir_verify_device: hash table side") != ZKIR_OK) return -ZKIR_ERR_DEVICE;
    E4 t = bb::e_zero(); hp.add_to(t);
    memcpy(T, t.c, 16);
    return 0;
  }
  int wide_side(const uint32_t* lk_m, uint32_t T[4]) {
    if (!wide_dev) return host_st.wide_side(&host, lk_m, T);
    stages_run++;
    int rc = upload(o_lk, lk_m, air::N_LK * 4); if (rc) return -rc;
    TapePartials wp;
    rc = wide_table_side_enqueue((const uint32_t*)(D() + o_wide + 16), (uint32_t)n_wide, (const uint32_t*)(D() + o_lk), (HashAux*)(D() + o_wlist), (E4*)(D() + o_part) + TAPE_MAX_BLOCKS, V.pin, s, &wp);
    if (rc) return -rc;
    if (hipStreamSynchronize(s) != hipSuccess || check_launch("zkir_verify_device: wide table side") != ZKIR_OK) return -ZKIR_ERR_DEVICE;
    E4 t = bb::e_zero(); wp.add_to(t);
    memcpy(T, t.c, 16);
    return 0;
  }
};
template <class F> int guarded(F&& f) {                          // an exception (no memory for a host vector) is a code, not an abort
  try { return f(); } catch (const std::exception& e) { zkir::set_last_error({ZKIR_ERR_OTHER, std::string("zkir_verify_device: ") + e.what()}); return -ZKIR_ERR_OTHER; }
}
int dt_hash_check(void* p, const uint32_t* w, size_t avail, uint64_t n_real, uint64_t code_end, size_t* used) { return guarded([&] { return static_cast<DeviceTapes*>(p)->hash_check(w, avail, n_real, code_end, used); }); }
int dt_wide_check(void* p, const uint32_t* sec, size_t n, uint64_t n_real) { return guarded([&] { return static_cast<DeviceTapes*>(p)->wide_check(sec, n, n_real); }); }
int dt_digests(void* p, int which, const uint32_t* sw, size_t sl, uint32_t* dg) { return guarded([&] { return static_cast<DeviceTapes*>(p)->digests(which, sw, sl, dg); }); }
int dt_hash_side(void* p, const uint32_t* lk_m, uint32_t T[4]) { return guarded([&] { return static_cast<DeviceTapes*>(p)->hash_side(lk_m, T); }); }
int dt_wide_side(void* p, const uint32_t* lk_m, uint32_t T[4]) { return guarded([&] { return static_cast<DeviceTapes*>(p)->wide_side(lk_m, T); }); }

// zkir_verify_device's body.  queries == nullptr: the whole verification (zkir_verify's verdict).  Else the verification up to check 11 with *queries filled where it
// returns 0 (zkir::stark_verify_collect): the query stage and check 30 are the caller's (stark_verify.inl).  *stages_run: the tape stages that ran on the device.
int verify_device_part(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, void* stream, zkir::StarkQueries* queries, uint32_t* stages_run) {
  *stages_run = 0;
  // modes 0-3 have no tapes, and a proof too short to name its mode has no verdict that depends on them: zkir_verify itself, no HIP call
  if (!proof || proof_words < 10 || proof[9] != 4) return guarded([&] { return zkir::stark_verify_collect(proof, proof_words, expect, true, nullptr, queries); });
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_verify_device: no current HIP device"}); return -ZKIR_ERR_DEVICE; }
  VerifyDevice* Vp = nullptr;
  const int src = guarded([&] { Vp = &verify_device(dev); return 0; });
  if (src) return src;
  VerifyDevice& V = *Vp;
  std::lock_guard<std::mutex> lock(V.mu);
  V.pin.reset();
  DeviceTapes dt(V, (hipStream_t)stream);
  const zkir::TapeStages st{&dt, dt_hash_check, dt_wide_check, dt_digests, dt_hash_side, dt_wide_side};
  const int rc = guarded([&] { return zkir::stark_verify_collect(proof, proof_words, expect, true, &st, queries); });
  if (dt.stages_run) (void)hipStreamSynchronize((hipStream_t)stream);      // (a verdict reached before a stage's own synchronisation: nothing of this call stays in flight)
  *stages_run = dt.stages_run;
  return rc;
}

}  // namespace

extern "C" {

int zkir_hash_tape_new_bytes_host(const uint32_t* hash_words, uint64_t n_hash_words, uint64_t* new_bytes) {
  if (!hash_words || !n_hash_words) { hash_words = tape_no_calls; n_hash_words = 1; }
  try {
    std::vector<hashcall::Call> calls;
    size_t used = 0;
    const int hrc = hashcall::parse_section(hash_words, (size_t)n_hash_words, ~0ull, 0, calls, &used);
    if (hrc || used != n_hash_words) { char m[160]; snprintf(m, sizeof m, "zkir_hash_tape_new_bytes_host: the hash section is malformed (check %d)", hrc ? hrc : 4); return tape_refuse(m); }
    std::vector<uint64_t> off(calls.size() + 1, 0);
    for (size_t k = 0; k < calls.size(); k++) off[k + 1] = off[k] + calls[k].cells.size();
    if (off.back() && !new_bytes) return tape_refuse("zkir_hash_tape_new_bytes_host: new_bytes must not be null where the section has calls");
    std::atomic<bool> failed{false};                            // (a worker thread must not let an exception out)
    hashcall::for_calls(calls.size(), hashcall::parts_for(calls.size()), [&](unsigned, size_t lo, size_t hi) {
      try {
        std::vector<uint64_t> nb;
        for (size_t k = lo; k < hi; k++) { hashcall::new_bytes(calls[k], nb); memcpy(new_bytes + off[k], nb.data(), nb.size() * 8); }
      } catch (...) { failed = true; }
    });
    if (failed) throw std::bad_alloc();
  } catch (const std::exception& e) { zkir::set_last_error({ZKIR_ERR_OTHER, std::string("zkir_hash_tape_new_bytes_host: ") + e.what()}); return ZKIR_ERR_OTHER; }
  return ZKIR_OK;
}

int zkir_hash_tape_new_bytes_launch(const uint32_t* hash_words, uint64_t n_hash_words, uint64_t* new_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!hash_words || !n_hash_words) { hash_words = tape_no_calls; n_hash_words = 1; }
  try {
    std::vector<uint64_t> prefix((size_t)std::min<uint64_t>(hash_words[0], n_hash_words / 8) + 2);
    const TapeWalk wk = hash_tape_walk(hash_words, n_hash_words, prefix.data());
    if (wk.cut || wk.used != n_hash_words) {
      // (a record the walk could not place: its own fields may still be what fails first — the host parser names the check)
      std::vector<hashcall::Call> calls; size_t used = 0;
      const int hrc = hashcall::parse_section(hash_words, (size_t)n_hash_words, ~0ull, 0, calls, &used);
      char m[160]; snprintf(m, sizeof m, "zkir_hash_tape_new_bytes_launch: the hash section is malformed (check %d)", hrc ? hrc : 4); return tape_refuse(m);
    }
    const uint64_t n_calls = wk.n_calls, H = wk.cells;
    if (!n_calls) return ZKIR_OK;
    if (!new_bytes) return tape_refuse("zkir_hash_tape_new_bytes_launch: new_bytes must not be null where the section has calls");
    const size_t o_prefix = al256(n_hash_words * 4), o_side = o_prefix + al256((n_calls + 1) * 8), o_check = o_side + al256(H * 8), total = o_check + 256;
    TapeDevMem dm;
    HIP_OK(hipMalloc(&dm.p, total));
    unsigned char* d = (unsigned char*)dm.p;
    zkir::HostPin pin;
    void* ht = pin.take(n_hash_words * 4); void* hp = pin.take((n_calls + 1) * 8); uint64_t* hs = pin.take_n<uint64_t>(H);
    if (!ht || !hp || !hs) HIP_OK(hipErrorOutOfMemory);
    memcpy(ht, hash_words, n_hash_words * 4); memcpy(hp, prefix.data(), (n_calls + 1) * 8);
    HIP_OK(hipMemcpyAsync(d, ht, n_hash_words * 4, hipMemcpyHostToDevice, s)); HIP_OK(hipMemcpyAsync(d + o_prefix, hp, (n_calls + 1) * 8, hipMemcpyHostToDevice, s));
    // the records must be what the kernel takes them for: hashcall::parse_section's checks, with no row bound and no code segment
    int code = 0;
    const int rc = hash_tape_check_run((const uint32_t*)d, (const uint64_t*)(d + o_prefix), n_calls, n_calls, ~0ull, 0, (unsigned long long*)(d + o_check), pin, s, &code);
    if (rc) return rc;
    if (code) { char m[160]; snprintf(m, sizeof m, "zkir_hash_tape_new_bytes_launch: the hash section is malformed (check %d)", code); return tape_refuse(m); }
    hash_new_bytes_enqueue((const uint32_t*)d, (const uint64_t*)(d + o_prefix), n_calls, H, (uint64_t*)(d + o_side), s);
    HIP_OK(hipMemcpyAsync(hs, d + o_side, H * 8, hipMemcpyDeviceToHost, s));
    std::vector<uint64_t> idx, val;
    long_call_patches(hash_words, prefix.data(), n_calls, idx, val);      // (host threads, while the kernels run)
    HIP_OK(hipStreamSynchronize(s));
    if (check_launch("zkir_hash_tape_new_bytes_launch") != ZKIR_OK) return ZKIR_ERR_DEVICE;
    memcpy(new_bytes, hs, H * 8);
    for (size_t i = 0; i < idx.size(); i++) new_bytes[idx[i]] = val[i];
  } catch (const std::exception& e) { zkir::set_last_error({ZKIR_ERR_OTHER, std::string("zkir_hash_tape_new_bytes_launch: ") + e.what()}); return ZKIR_ERR_OTHER; }
  return ZKIR_OK;
}

int zkir_verify_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, void* stream) {
  uint32_t stages_run = 0;
  const int rc = verify_device_part(proof, proof_words, expect, stream, nullptr, &stages_run);
  zkir::verify_note_device_stages(stages_run);
  return rc;
}

}  // extern "C"
