// tape_digest.inl — (AIR mode 4) what every hash call of a tape WROTE, recomputed on the device: hashcall::new_bytes for a section that has passed the record checks
// (included by stark_prove.inl behind tape_table.inl, inside its unnamed namespace).
//
// The prover takes a call's 32 output bytes from the interpreter's records; a verifier has only the tape.  Per call it rebuilds the message from the OLD bytes of the cells
// under [in, in + len) (reads come before writes, crypto.rs:232-235: an output that overlaps its own input does not change the message), hashes it — SHA-256 (kind 3),
// Keccak-256 with the original padding byte 0x01 (kind 5), BLAKE3 (kind 6) — and lays the 32 bytes over the old bytes of the cells under [out, out + 32).  side[h] = cell h's
// bytes after its call, in the section's cell order: what hash_table_side_kernel reads.
//
// Two kernels.  hash_tape_old_bytes_kernel copies every touched cell's old bytes (a thread per cell).  hash_tape_new_bytes_kernel then gives every call a LANE: the lane
// reads its message eight bytes at a time straight from the record's cell words (msg64: two cells, shifted by in & 7 — no per-lane byte buffer), hashes, and rewrites the
// four or five cells of its output.  Nothing in it is a dynamically indexed private array: the SHA-256 schedule window, the Keccak state and the BLAKE3 block are indexed by
// unrolled loop counters only, and a call of at most TAPE_L_DEV = 1024 bytes is ONE BLAKE3 chunk, so the lanes need no chaining-value stack.
// Calls longer than TAPE_L_DEV (up to hashcall::MAX_LEN = 1 MiB) are left out by the lanes — one such lane would hold its wave for thousands of compressions — and hashed
// with hashcall::output_bytes on host threads while the kernels run (long_call_patches); their output cells are patched in afterwards (DESIGN 8.10 b''').
// The SHA-256 rounds of witness.hip build the chip's witness columns from a padded block in another translation unit: not shared.

constexpr uint32_t TAPE_L_DEV = 1024;                           // a lane hashes calls of at most this many bytes: one full BLAKE3 chunk

__device__ const uint32_t TD_K256[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
    0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
    0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
__device__ const uint64_t TD_KRC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
                                        0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
                                        0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
                                        0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

__device__ __forceinline__ uint32_t td_ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
__device__ __forceinline__ uint64_t td_rol64(uint64_t x, int n) { return (x << n) | (x >> (64 - n)); }
__device__ __forceinline__ uint32_t td_bswap(uint32_t x) { return __builtin_bswap32(x); }
// a cell's bytes out of its record (time, four 16-bit pieces)
__device__ __forceinline__ uint64_t td_cell(const uint32_t* __restrict__ q) { return (uint64_t)q[1] | ((uint64_t)q[2] << 16) | ((uint64_t)q[3] << 32) | ((uint64_t)q[4] << 48); }

// A call's message where it lies: q = the record of the first cell under the input (the input's cells are consecutive records: hashcall::spans_of), sh = 8 (in & 7),
// n_in = how many cells lie under the input.  get(i) = message bytes 8 i .. 8 i + 7, little-endian, zero beyond len.
struct TapeMsg {
  const uint32_t* q; uint32_t sh, len, n_in;
  __device__ __forceinline__ uint64_t get(uint32_t i) const {
    if (8 * i >= len) return 0;                                 // (so i < n_in below: byte 8 i lies in cell i of the input)
    uint64_t v = td_cell(q + 5 * i) >> sh;
    if (sh && i + 1 < n_in) v |= td_cell(q + 5 * (i + 1)) << (64 - sh);
    const uint32_t rem = len - 8 * i;
    if (rem < 8) v &= (1ull << (8 * rem)) - 1;
    return v;
  }
  // .. with the padding's first byte (0x80 / 0x01) behind the message's last
  __device__ __forceinline__ uint64_t get_padded(uint32_t i, uint64_t pad) const { uint64_t v = get(i); if ((len >> 3) == i) v |= pad << (8 * (len & 7)); return v; }
};

// d = the 32 bytes the call writes at out, as four little-endian words (hashcall::output_bytes)
__device__ void td_sha256(const TapeMsg& m, uint64_t d[4]) {
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  const uint32_t n_blk = (m.len + 9 + 63) >> 6;
  for (uint32_t b = 0; b < n_blk; b++) {
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 8; j++) { const uint64_t v = m.get_padded(8 * b + j, 0x80); w[2 * j] = td_bswap((uint32_t)v); w[2 * j + 1] = td_bswap((uint32_t)(v >> 32)); }
    if (b + 1 == n_blk) { w[14] = 0; w[15] = m.len * 8; }     // (len <= TAPE_L_DEV: the bit count fits the low word)
    uint32_t s0 = h[0], s1 = h[1], s2 = h[2], s3 = h[3], s4 = h[4], s5 = h[5], s6 = h[6], s7 = h[7];
    for (int t0 = 0; t0 < 64; t0 += 16) {
#pragma unroll
      for (int j = 0; j < 16; j++) {
        if (t0) {                                                // rolling 16-word schedule window
          const uint32_t w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
          w[j] += (td_ror(w15, 7) ^ td_ror(w15, 18) ^ (w15 >> 3)) + w[(j + 9) & 15] + (td_ror(w2, 17) ^ td_ror(w2, 19) ^ (w2 >> 10));
        }
        const uint32_t t1 = s7 + (td_ror(s4, 6) ^ td_ror(s4, 11) ^ td_ror(s4, 25)) + ((s4 & s5) ^ (~s4 & s6)) + TD_K256[t0 + j] + w[j];
        const uint32_t t2 = (td_ror(s0, 2) ^ td_ror(s0, 13) ^ td_ror(s0, 22)) + ((s0 & s1) ^ (s0 & s2) ^ (s1 & s2));
        s7 = s6; s6 = s5; s5 = s4; s4 = s3 + t1; s3 = s2; s2 = s1; s1 = s0; s0 = t1 + t2;
      }
    }
    h[0] += s0; h[1] += s1; h[2] += s2; h[3] += s3; h[4] += s4; h[5] += s5; h[6] += s6; h[7] += s7;
  }
  // the eight big-endian-parsed words, each stored little-endian (crypto.rs:251-254)
#pragma unroll
  for (int j = 0; j < 4; j++) d[j] = (uint64_t)h[2 * j] | ((uint64_t)h[2 * j + 1] << 32);
}

__device__ __forceinline__ void td_keccakf(uint64_t (&st)[25]) {
  constexpr int ROT[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
  constexpr int PIL[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
  for (int round = 0; round < 24; round++) {
    uint64_t bc[5];
#pragma unroll
    for (int i = 0; i < 5; i++) bc[i] = st[i] ^ st[i + 5] ^ st[i + 10] ^ st[i + 15] ^ st[i + 20];
#pragma unroll
    for (int i = 0; i < 5; i++) {
      const uint64_t t = bc[(i + 4) % 5] ^ td_rol64(bc[(i + 1) % 5], 1);
#pragma unroll
      for (int j = 0; j < 25; j += 5) st[j + i] ^= t;
    }
    uint64_t t = st[1];
#pragma unroll
    for (int i = 0; i < 24; i++) { const uint64_t b = st[PIL[i]]; st[PIL[i]] = td_rol64(t, ROT[i]); t = b; }
#pragma unroll
    for (int j = 0; j < 25; j += 5) {
#pragma unroll
      for (int i = 0; i < 5; i++) bc[i] = st[j + i];
#pragma unroll
      for (int i = 0; i < 5; i++) st[j + i] ^= (~bc[(i + 1) % 5]) & bc[(i + 2) % 5];
    }
    st[0] ^= TD_KRC[round];
  }
}
__device__ void td_keccak256(const TapeMsg& m, uint64_t d[4]) {
  uint64_t st[25];
#pragma unroll
  for (int i = 0; i < 25; i++) st[i] = 0;
  const uint32_t n_blk = m.len / 136 + 1;                       // rate 136 bytes = 17 lanes; the padding always fits the last block
  for (uint32_t b = 0; b < n_blk; b++) {
#pragma unroll
    for (int i = 0; i < 17; i++) st[i] ^= m.get_padded(17 * b + i, 0x01);
    if (b + 1 == n_blk) st[16] ^= 0x80ull << 56;
    td_keccakf(st);
  }
#pragma unroll
  for (int j = 0; j < 4; j++) d[j] = st[j];
}

// one chunk (len <= 1024): up to 16 blocks chained, the last one CHUNK_END | ROOT
__device__ void td_blake3(const TapeMsg& m, uint64_t d[4]) {
  constexpr int PERM[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
  const uint32_t IV0 = 0x6A09E667, IV1 = 0xBB67AE85, IV2 = 0x3C6EF372, IV3 = 0xA54FF53A;
  uint32_t cv[8] = {IV0, IV1, IV2, IV3, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19};
  const uint32_t n_blk = m.len == 0 ? 1 : (m.len + 63) >> 6;
  for (uint32_t b = 0; b < n_blk; b++) {
    uint32_t mw[16];
#pragma unroll
    for (int j = 0; j < 8; j++) { const uint64_t v = m.get(8 * b + j); mw[2 * j] = (uint32_t)v; mw[2 * j + 1] = (uint32_t)(v >> 32); }
    const uint32_t bl = b + 1 == n_blk ? m.len - 64 * b : 64, flags = (b == 0 ? 1u : 0u) | (b + 1 == n_blk ? 2u | 8u : 0u);      // CHUNK_START 1, CHUNK_END 2, ROOT 8
    uint32_t v[16] = {cv[0], cv[1], cv[2], cv[3], cv[4], cv[5], cv[6], cv[7], IV0, IV1, IV2, IV3, 0u, 0u, bl, flags};          // (chunk counter 0)
#define TD_G(a, b_, c, d_, x, y)                              \
  v[a] += v[b_] + (x); v[d_] = td_ror(v[d_] ^ v[a], 16);      \
  v[c] += v[d_];       v[b_] = td_ror(v[b_] ^ v[c], 12);      \
  v[a] += v[b_] + (y); v[d_] = td_ror(v[d_] ^ v[a], 8);       \
  v[c] += v[d_];       v[b_] = td_ror(v[b_] ^ v[c], 7);
    for (int r = 0; r < 7; r++) {
      TD_G(0, 4, 8, 12, mw[0], mw[1]) TD_G(1, 5, 9, 13, mw[2], mw[3]) TD_G(2, 6, 10, 14, mw[4], mw[5]) TD_G(3, 7, 11, 15, mw[6], mw[7])
      TD_G(0, 5, 10, 15, mw[8], mw[9]) TD_G(1, 6, 11, 12, mw[10], mw[11]) TD_G(2, 7, 8, 13, mw[12], mw[13]) TD_G(3, 4, 9, 14, mw[14], mw[15])
      uint32_t t[16];                                            // the fixed permutation of the message words between rounds
#pragma unroll
      for (int i = 0; i < 16; i++) t[i] = mw[PERM[i]];
#pragma unroll
      for (int i = 0; i < 16; i++) mw[i] = t[i];
    }
#undef TD_G
#pragma unroll
    for (int i = 0; i < 8; i++) cv[i] = v[i] ^ v[i + 8];
  }
#pragma unroll
  for (int j = 0; j < 4; j++) d[j] = (uint64_t)cv[2 * j] | ((uint64_t)cv[2 * j + 1] << 32);
}

// side[h] = cell h's OLD bytes; a cell finds its call by the search hash_table_side_kernel does
__global__ __launch_bounds__(NT) void hash_tape_old_bytes_kernel(const uint32_t* __restrict__ tape, const uint64_t* __restrict__ prefix, uint64_t n_calls, uint64_t H, uint64_t* __restrict__ side) {
  for (uint64_t h = (uint64_t)blockIdx.x * NT + threadIdx.x; h < H; h += (uint64_t)gridDim.x * NT) {
    uint64_t lo = 0, hi = n_calls;
    while (lo + 1 < hi) { const uint64_t m = lo + (hi - lo) / 2; if (prefix[m] <= h) lo = m; else hi = m; }
    side[h] = td_cell(tape + (1 + 8 * (lo + 1) + 5 * h));       // (the cells before h and the headers of calls 0 .. lo lie before it)
  }
}
// One lane per call of at most TAPE_L_DEV bytes: the digest over the call's output cells (side already holds every cell's old bytes).  The records have passed
// hash_tape_check_kernel: every count word is n_cells_of its record, prefix is their running sum, every field is in range.
__global__ __launch_bounds__(NT) void hash_tape_new_bytes_kernel(const uint32_t* __restrict__ tape, const uint64_t* __restrict__ prefix, uint64_t n_calls, uint64_t* __restrict__ side) {
  const uint64_t k = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (k >= n_calls) return;
  const uint64_t before = prefix[k];
  const uint32_t* c = tape + (1 + 8 * k + 5 * before);
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
// side[idx[i]] = val[i]: the output cells of the calls the host hashed
__global__ __launch_bounds__(NT) void side_patch_kernel(const uint64_t* __restrict__ idx, const uint64_t* __restrict__ val, uint64_t n, uint64_t* __restrict__ side) {
  const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (i < n) side[idx[i]] = val[i];
}
// the wide tape's record checks (verify.cpp: 57), one record per thread; *bad (zeroed by the caller) != 0: some record fails
__global__ __launch_bounds__(NT) void wide_tape_check_kernel(const uint32_t* __restrict__ recs, uint64_t n, uint64_t n_real, uint32_t* __restrict__ bad) {
  const uint64_t k = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (k >= n) return;
  const uint32_t* c = recs + 8 * k;
  const bool fails = c[1] >= (1u << 20) || c[2] >= (1u << 20) || c[3] >= (1u << 24) || c[4] >= (1u << 20) || c[5] >= (1u << 20) || c[6] >= (1u << 24) || c[7] < 3 || c[7] > 7 ||
                     c[0] >= n_real || (k && c[0] <= c[-8]) || (c[7] >= 4 && !(c[4] | c[5] | c[6]));
  if (fails) atomicOr(bad, 1u);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------------------------------------
// The calls of a CHECKED section (host words, the walk's prefix) that are longer than TAPE_L_DEV, hashed with hashcall::new_bytes on host threads: five (cell index in
// the section's order, new bytes) pairs per such call — its output cells, the last pair repeated when the output lies on four.
void long_call_patches(const uint32_t* w, const uint64_t* prefix, uint64_t n_calls, std::vector<uint64_t>& idx, std::vector<uint64_t>& val) {
  std::vector<uint64_t> which;
  for (uint64_t k = 0; k < n_calls; k++) if (w[1 + 8 * k + 5 * prefix[k] + 3] > TAPE_L_DEV) which.push_back(k);
  idx.assign(5 * which.size(), 0); val.assign(5 * which.size(), 0);
  if (which.empty()) return;
  std::atomic<bool> failed{false};                              // (a worker thread must not let an exception out: it would end the process)
  hashcall::for_calls(which.size(), hashcall::parts_for(which.size() * 512), [&](unsigned, size_t lo, size_t hi) {      // (a call here is worth a thread's start by itself)
   try {
    hashcall::Call hc; std::vector<uint64_t> nb;
    for (size_t i = lo; i < hi; i++) {
      const uint64_t k = which[i];
      const uint32_t* c = w + (1 + 8 * k + 5 * prefix[k]);
      hc.cycle = c[0]; hc.in_ptr = (uint64_t)c[1] | ((uint64_t)c[2] << 20); hc.len = c[3]; hc.out_ptr = (uint64_t)c[4] | ((uint64_t)c[5] << 20); hc.kind = c[6];
      const uint64_t n = hashcall::n_cells_of(hc.in_ptr, hc.len, hc.out_ptr);
      hc.cells.resize((size_t)n);
      for (uint64_t r = 0; r < n; r++) {
        const uint32_t* q = c + 8 + 5 * r;
        hc.cells[(size_t)r] = hashcall::Cell{hashcall::cell_at(hc.in_ptr, hc.len, hc.out_ptr, r), (uint64_t)q[1] | ((uint64_t)q[2] << 16) | ((uint64_t)q[3] << 32) | ((uint64_t)q[4] << 48), q[0]};
      }
      hashcall::new_bytes(hc, nb);
      const uint64_t r_out = hashcall::rank_of(hc.in_ptr, hc.len, hc.out_ptr, hc.out_ptr & ~7ull), n_out = (hc.out_ptr & 7) ? 5 : 4;
      for (uint64_t t = 0; t < 5; t++) { const uint64_t r = r_out + (t < n_out ? t : n_out - 1); idx[5 * i + t] = prefix[k] + r; val[5 * i + t] = nb[(size_t)r]; }
    }
   } catch (...) { failed = true; }
  });
  if (failed) throw std::bad_alloc();                           // (the message of a long call is up to 1 MiB of host memory; the caller turns this into a code)
}
// enqueues the two kernels: d_side = every touched cell's bytes after its call, but for the output cells of the calls above TAPE_L_DEV (long_call_patches)
void hash_new_bytes_enqueue(const uint32_t* d_tape, const uint64_t* d_prefix, uint64_t n_calls, uint64_t H, uint64_t* d_side, hipStream_t s) {
  if (!n_calls) return;
  hipLaunchKernelGGL(hash_tape_old_bytes_kernel, dim3(tape_grid(H)), dim3(NT), 0, s, d_tape, d_prefix, n_calls, H, d_side);
  hipLaunchKernelGGL(hash_tape_new_bytes_kernel, dim3(grid_for(n_calls)), dim3(NT), 0, s, d_tape, d_prefix, n_calls, d_side);
}
