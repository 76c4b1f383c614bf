// tape_table.inl — (AIR mode 4) the hash tape's and the wide tape's share of the lookup argument's table side, and the hash tape's record checks, on the device
// (included by stark_prove.inl, inside its unnamed namespace, behind HashAux / hash_aux_kernel).
//
// What the verifier forms from the proof's sections (verify.cpp; oracle: so::hash_table_sum / so::wide_table_sum):
//   per hash call      + 1 / (alpha - fp(call))                                   — also the call's row's helper HH
//   per touched cell   - 1 / (alpha - fp(cell, told, old bytes)) + 1 / (alpha - fp(cell, cycle + 1, new bytes))
//   per wide record    + 1 / (alpha - fp(cycle, rs1, rs2, the reference's result, opcode))   — also the row's helper WW
// with fp = tag lambda^11 + sum_{j < 11} e_j lambda^j.  Field addition is exact and commutative: the sums do not depend on the order of their terms, so a proof made from
// them is the proof the host sums give, byte for byte.  Every item (a call, a touched cell, a record) is one loop turn of one thread; a workgroup leaves ONE partial sum and
// the host adds the partials.  The helpers go into a dense list of HashAux (row, 1 / d) in item order: the running-sum increment of a row needs T / N, which needs every
// term first — hash_aux_kernel scatters the list into the aux trace once T is known (zkir_prove), the stand-alone entries copy it back.
//
// The host functions below (hash_table_side_host / wide_table_side_host) are what the prover ran before these kernels: they remain the reference the tests hold the
// kernels to, and what a proof from a caller's host witness runs for its hash calls (there the new bytes come from a digest per call).

constexpr unsigned TAPE_MAX_BLOCKS = 2048;                     // grid cap: a thread takes its items at a stride of the grid, the partial sums fit a fixed buffer

// alpha - fp(e; tag), Montgomery.  lk: the proof's lookup parameters (air.h LK_*), Montgomery words; e: canonical words (any 32-bit value is taken modulo p)
BB_HD E4 tape_den(const uint32_t* __restrict__ lk, const uint32_t (&e)[air::N_TUPLE], uint32_t tag) {
  uint32_t em[air::N_TUPLE];
  for (int j = 0; j < air::N_TUPLE; j++) em[j] = bb::to_mont(e[j]);
  const uint32_t tm = bb::to_mont(tag);
  E4 d;
  for (int c4 = 0; c4 < 4; c4++) {
    uint32_t f = bb::mont_mul(lk[air::LK_LAM + 4 * air::N_TUPLE + c4], tm);
    for (int j = 0; j < air::N_TUPLE; j++) f = bb::add(f, bb::mont_mul(lk[air::LK_LAM + 4 * j + c4], em[j]));
    d.c[c4] = bb::sub(lk[air::LK_ALPHA + c4], f);
  }
  return d;
}
BB_HD E4 hash_call_den(const uint32_t* __restrict__ lk, uint64_t cycle, uint64_t in_ptr, uint64_t len, uint64_t out_ptr, uint32_t kind) {
  const uint32_t e[air::N_TUPLE] = {(uint32_t)(cycle % bb::P), (uint32_t)(in_ptr & 0xFFFFF), (uint32_t)((in_ptr >> 20) & 0xFFFFF), (uint32_t)(in_ptr >> 40), (uint32_t)(len & 0xFFFFF),
                                    (uint32_t)((len >> 20) & 0xFFFFF), (uint32_t)(len >> 40), (uint32_t)(out_ptr & 0xFFFFF), (uint32_t)((out_ptr >> 20) & 0xFFFFF), (uint32_t)(out_ptr >> 40), kind};
  return tape_den(lk, e, (uint32_t)air::TAG_HASH);
}
BB_HD E4 mem_cell_den(const uint32_t* __restrict__ lk, uint64_t addr, uint32_t t, uint64_t bytes) {
  const uint32_t e[air::N_TUPLE] = {(uint32_t)(addr & 0xFFFFF), (uint32_t)((addr >> 20) & 0xFFFFF), t, (uint32_t)(bytes & 0xFF), (uint32_t)((bytes >> 8) & 0xFF), (uint32_t)((bytes >> 16) & 0xFF),
                                    (uint32_t)((bytes >> 24) & 0xFF), (uint32_t)((bytes >> 32) & 0xFF), (uint32_t)((bytes >> 40) & 0xFF), (uint32_t)((bytes >> 48) & 0xFF), (uint32_t)(bytes >> 56)};
  return tape_den(lk, e, (uint32_t)air::TAG_MEM);
}
BB_HD E4 wide_record_den(const uint32_t* __restrict__ lk, const uint32_t* __restrict__ r) {      // r: (cycle, rs1's three limbs, rs2's three limbs, opcode)
  const uint64_t a = (uint64_t)r[1] | ((uint64_t)r[2] << 20) | ((uint64_t)r[3] << 40), b = (uint64_t)r[4] | ((uint64_t)r[5] << 20) | ((uint64_t)r[6] << 40);
  const uint64_t y = air::wide_result(r[7], a, b);
  const uint32_t e[air::N_TUPLE] = {r[0] % bb::P, r[1], r[2], r[3], r[4], r[5], r[6], (uint32_t)(y & 0xFFFFF), (uint32_t)((y >> 20) & 0xFFFFF), (uint32_t)(y >> 40), r[7]};
  return tape_den(lk, e, (uint32_t)air::TAG_WIDE);
}

// one partial sum per workgroup: a shuffle tree inside each wave, the waves' sums through LDS
__device__ __forceinline__ void block_sum_to(E4 v, E4* __restrict__ out) {
  __shared__ E4 wave_sum[NT / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    E4 o;
#pragma unroll
    for (int k = 0; k < 4; k++) o.c[k] = (uint32_t)__shfl_down((int)v.c[k], off, 64);
    v = bb::e_add(v, o);
  }
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    E4 t = wave_sum[0];
#pragma unroll
    for (uint32_t w = 1; w < NT / 64; w++) t = bb::e_add(t, wave_sum[w]);
    *out = t;
  }
}

// Items [0, n_calls): the calls; [n_calls, n_calls + H): the touched cells of all calls in tape order.  tape: the hash section ([n] then the records); prefix[k]: how
// many cells the calls before call k touch (prefix[n_calls] = H), so call k's record starts at word 1 + 8 k + 5 prefix[k]; side[h]: cell h's bytes AFTER its call.
// A cell finds its call by the search the witness's expand step does (memcheck.hip: hcells_kernel).  list[k] = (call k's row, 1 / d_k).
__global__ __launch_bounds__(NT) void hash_table_side_kernel(const uint32_t* __restrict__ tape, const uint64_t* __restrict__ prefix, const uint64_t* __restrict__ side, uint64_t n_calls, uint64_t H,
                                                              const uint32_t* __restrict__ lk, HashAux* __restrict__ list, E4* __restrict__ partial) {
  E4 acc = bb::e_zero();
  const uint64_t n_items = n_calls + H;
  for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n_items; i += (uint64_t)gridDim.x * NT) {
    if (i < n_calls) {
      const uint32_t* c = tape + (1 + 8 * i + 5 * prefix[i]);
      const E4 h = bb::e_inv_m(hash_call_den(lk, c[0], (uint64_t)c[1] | ((uint64_t)c[2] << 20), c[3], (uint64_t)c[4] | ((uint64_t)c[5] << 20), c[6]));
      acc = bb::e_add(acc, h);
      HashAux x; x.row = c[0]; x.pad[0] = x.pad[1] = x.pad[2] = 0; x.h = h;
      list[i] = x;
    } else {
      const uint64_t h = i - n_calls;
      uint64_t lo = 0, hi = n_calls;                              // the last call whose prefix <= h (every call touches at least the four cells of its output)
      while (lo + 1 < hi) { const uint64_t m = lo + (hi - lo) / 2; if (prefix[m] <= h) lo = m; else hi = m; }
      const uint64_t before = prefix[lo], r = h - before;
      const uint32_t* c = tape + (1 + 8 * lo + 5 * before);
      const uint64_t addr = hashcall::cell_at((uint64_t)c[1] | ((uint64_t)c[2] << 20), c[3], (uint64_t)c[4] | ((uint64_t)c[5] << 20), r);
      const uint32_t* q = c + 8 + 5 * r;
      const uint64_t old = (uint64_t)q[1] | ((uint64_t)q[2] << 16) | ((uint64_t)q[3] << 32) | ((uint64_t)q[4] << 48);
      const E4 dm = mem_cell_den(lk, addr, q[0], old), dp = mem_cell_den(lk, addr, (uint32_t)(((uint64_t)c[0] + 1) % bb::P), side[h]);
      // 1 / d+ - 1 / d- = (d- - d+) / (d+ d-): one inversion for the two terms
      acc = bb::e_add(acc, bb::e_mul_m(bb::e_sub(dm, dp), bb::e_inv_m(bb::e_mul_m(dp, dm))));
    }
  }
  block_sum_to(acc, partial + blockIdx.x);
}

// One record per loop turn, in whatever order lookup_index_kernel appended them.  list[k] = (record k's row, 1 / d_k).  (Small and on its own: DESIGN 8.10a'.)
__global__ __launch_bounds__(NT) void wide_table_side_kernel(const uint32_t* __restrict__ recs, uint32_t n, const uint32_t* __restrict__ lk, HashAux* __restrict__ list, E4* __restrict__ partial) {
  E4 acc = bb::e_zero();
  for (uint32_t k = blockIdx.x * NT + threadIdx.x; k < n; k += gridDim.x * NT) {
    const uint4 r0 = reinterpret_cast<const uint4*>(recs)[2 * (uint64_t)k], r1 = reinterpret_cast<const uint4*>(recs)[2 * (uint64_t)k + 1];
    const uint32_t r[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    const E4 h = bb::e_inv_m(wide_record_den(lk, r));
    acc = bb::e_add(acc, h);
    HashAux x; x.row = r[0]; x.pad[0] = x.pad[1] = x.pad[2] = 0; x.h = h;
    list[k] = x;
  }
  block_sum_to(acc, partial + blockIdx.x);
}

// hashcall::parse_section's checks on a tape in device memory, one call per thread, in that function's order within a record; *result = min over the failing calls of
// (call << 8 | code) (the caller sets it to all ones: no call fails).  Calls [0, n_full) lie in the buffer whole; of call n_full (n_check = n_full + 1) only the eight
// header words do: it fails with its header's code if it has one, else with 4 (truncated).  One atomic per workgroup, on the flags gathered in LDS.
__global__ __launch_bounds__(NT) void hash_tape_check_kernel(const uint32_t* __restrict__ tape, const uint64_t* __restrict__ prefix, uint64_t n_check, uint64_t n_full, uint64_t n_real, uint64_t code_end,
                                                              unsigned long long* __restrict__ result) {
  __shared__ unsigned long long smin;
  if (threadIdx.x == 0) smin = ~0ull;
  __syncthreads();
  const uint64_t k = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (k < n_check) {
    const uint32_t* c = tape + (1 + 8 * k + 5 * prefix[k]);
    uint32_t code = 0;
    const uint64_t cycle = c[0], in_ptr = (uint64_t)c[1] | ((uint64_t)c[2] << 20), len = c[3], out_ptr = (uint64_t)c[4] | ((uint64_t)c[5] << 20);
    if (c[1] >= (1u << 20) || c[2] >= (1u << 20) || c[4] >= (1u << 20) || c[5] >= (1u << 20)) code = 56;
    else if (cycle >= n_real || (k && cycle <= tape[1 + 8 * (k - 1) + 5 * prefix[k - 1]]) || !hashcall::in_range(in_ptr, len, out_ptr, c[6])) code = 56;
    else if (out_ptr < code_end && out_ptr + 32 > 0x1000) code = 55;
    else {
      const uint64_t n = hashcall::n_cells_of(in_ptr, len, out_ptr);
      if (c[7] != n) code = 56;
      else if (k >= n_full) code = 4;
      else {
        const uint32_t* q = c + 8;
        for (uint64_t j = 0; j < n && !code; j++, q += 5)
          if (q[1] > 0xFFFF || q[2] > 0xFFFF || q[3] > 0xFFFF || q[4] > 0xFFFF || q[0] > cycle) code = 56;
      }
    }
    if (code) atomicMin(&smin, (unsigned long long)((k << 8) | code));
  }
  __syncthreads();
  if (threadIdx.x == 0 && smin != ~0ull) atomicMin(result, smin);
}

// ---- the host forms (the reference) ----------------------------------------------------------------------------------------------------------------------------------
// The hash calls' share: returns the sum (Montgomery) and fills aux[k] = (call k's row, 1 / d_k).  side: per touched cell, in the section's order, the bytes after its
// call; nullptr: they are made from a digest per call (hashcall::new_bytes).  Host threads, one batch inversion each.
E4 hash_table_side_host(const std::vector<hashcall::Call>& calls, const uint64_t* side, const uint32_t* lk, std::vector<HashAux>& aux, unsigned* parts_used = nullptr) {
  aux.resize(calls.size());
  std::vector<uint64_t> side_off;                                // where a call's cells start in the side array
  if (side) { side_off.resize(calls.size()); uint64_t o = 0; for (size_t ci = 0; ci < calls.size(); ci++) { side_off[ci] = o; o += calls[ci].cells.size(); } }
  const unsigned parts = hashcall::parts_for(calls.size());
  if (parts_used) *parts_used = parts;
  std::vector<E4> Tpart(parts, bb::e_zero());
  hashcall::for_calls(calls.size(), parts, [&](unsigned part, size_t lo, size_t hi) {        // (host threads: 175 k calls at 2^20 rows of the SHA chain are ~1 s on one core)
    std::vector<E4> d; std::vector<int8_t> sign; std::vector<uint64_t> nb;
    for (size_t ci = lo; ci < hi; ci++) {
      const hashcall::Call& hc = calls[ci];
      d.push_back(hash_call_den(lk, hc.cycle, hc.in_ptr, hc.len, hc.out_ptr, hc.kind)); sign.push_back(2);      // (2: a call's own entry — its inverse is also the row's HH)
      const uint64_t* nbp;
      if (side) nbp = side + side_off[ci]; else { hashcall::new_bytes(hc, nb); nbp = nb.data(); }
      for (size_t k = 0; k < hc.cells.size(); k++) {
        d.push_back(mem_cell_den(lk, hc.cells[k].addr, hc.cells[k].t, hc.cells[k].bytes)); sign.push_back(-1);
        d.push_back(mem_cell_den(lk, hc.cells[k].addr, (uint32_t)((hc.cycle + 1) % bb::P), nbp[k])); sign.push_back(1);
      }
    }
    std::vector<E4> pre(d.size());
    E4 acc = bb::e_one_m();
    for (size_t i = 0; i < d.size(); i++) { pre[i] = acc; acc = bb::e_mul_m(acc, d[i]); }
    E4 inv = bb::e_inv_m(acc), Tp = bb::e_zero();
    size_t call = hi;
    for (size_t i = d.size(); i-- > 0;) {
      const E4 di = bb::e_mul_m(inv, pre[i]);
      inv = bb::e_mul_m(inv, d[i]);
      if (sign[i] < 0) Tp = bb::e_sub(Tp, di); else Tp = bb::e_add(Tp, di);
      if (sign[i] == 2) { call--; aux[call].row = (uint32_t)calls[call].cycle; aux[call].pad[0] = aux[call].pad[1] = aux[call].pad[2] = 0; aux[call].h = di; }
    }
    Tpart[part] = Tp;
  });
  E4 T = bb::e_zero();
  for (const E4& tp : Tpart) T = bb::e_add(T, tp);
  return T;
}
// The wide tape's share: recs = n records of eight words; the result is computed HERE (air::wide_result).  aux[k] = (record k's row, 1 / d_k).
E4 wide_table_side_host(const uint32_t* recs, size_t n, const uint32_t* lk, std::vector<HashAux>& aux) {
  aux.resize(n);
  const unsigned parts = hashcall::parts_for(n / 4);
  std::vector<E4> Tpart(parts, bb::e_zero());
  hashcall::for_calls(n, parts, [&](unsigned part, size_t lo, size_t hi) {        // (host threads: a run with 2^18 tape rows is ~50 ms on one core)
    std::vector<E4> d(hi - lo), pre(hi - lo);
    for (size_t k = lo; k < hi; k++) d[k - lo] = wide_record_den(lk, recs + 8 * k);
    E4 acc = bb::e_one_m(), Tp = bb::e_zero();
    for (size_t k = 0; k < d.size(); k++) { pre[k] = acc; acc = bb::e_mul_m(acc, d[k]); }
    E4 inv = bb::e_inv_m(acc);
    for (size_t k = d.size(); k-- > 0;) {
      const E4 dk = bb::e_mul_m(inv, pre[k]);
      inv = bb::e_mul_m(inv, d[k]);
      Tp = bb::e_add(Tp, dk);
      HashAux& x = aux[lo + k];
      x.row = recs[8 * (lo + k)]; x.pad[0] = x.pad[1] = x.pad[2] = 0; x.h = dk;
    }
    Tpart[part] = Tp;
  });
  E4 T = bb::e_zero();
  for (const E4& tp : Tpart) T = bb::e_add(T, tp);
  return T;
}

// ---- the device forms: what zkir_prove and the stand-alone entries both run -------------------------------------------------------------------------------------------
// Each enqueues its kernel and the copy of its partial sums into pinned staging on the stream; the caller synchronises the stream, then reads (add_to).
struct TapePartials {
  const E4* h = nullptr; unsigned n = 0;
  void add_to(E4& T) const { for (unsigned k = 0; k < n; k++) T = bb::e_add(T, h[k]); }
};
inline unsigned tape_grid(uint64_t n_items) { const uint64_t g = (n_items + NT - 1) / NT; return (unsigned)(g < TAPE_MAX_BLOCKS ? g : TAPE_MAX_BLOCKS); }
// d_list: n_calls entries; d_part: TAPE_MAX_BLOCKS entries (device)
int hash_table_side_enqueue(const uint32_t* d_tape, const uint64_t* d_prefix, const uint64_t* d_side, uint64_t n_calls, uint64_t H, const uint32_t* d_lk, HashAux* d_list, E4* d_part,
                            zkir::HostPin& pin, hipStream_t s, TapePartials* out) {
  *out = TapePartials{};
  if (!n_calls) return ZKIR_OK;
  const unsigned g = tape_grid(n_calls + H);
  E4* hp = pin.take_n<E4>(g);
  if (!hp) HIP_OK(hipErrorOutOfMemory);
  hipLaunchKernelGGL(hash_table_side_kernel, dim3(g), dim3(NT), 0, s, d_tape, d_prefix, d_side, n_calls, H, d_lk, d_list, d_part);
  HIP_OK(hipMemcpyAsync(hp, d_part, (size_t)g * sizeof(E4), hipMemcpyDeviceToHost, s));
  out->h = hp; out->n = g;
  return ZKIR_OK;
}
int wide_table_side_enqueue(const uint32_t* d_recs, uint32_t n, const uint32_t* d_lk, HashAux* d_list, E4* d_part, zkir::HostPin& pin, hipStream_t s, TapePartials* out) {
  *out = TapePartials{};
  if (!n) return ZKIR_OK;
  const unsigned g = tape_grid(n);
  E4* hp = pin.take_n<E4>(g);
  if (!hp) HIP_OK(hipErrorOutOfMemory);
  hipLaunchKernelGGL(wide_table_side_kernel, dim3(g), dim3(NT), 0, s, d_recs, n, d_lk, d_list, d_part);
  HIP_OK(hipMemcpyAsync(hp, d_part, (size_t)g * sizeof(E4), hipMemcpyDeviceToHost, s));
  out->h = hp; out->n = g;
  return ZKIR_OK;
}
// The record checks; synchronises the stream.  *code = parse_section's code of the lowest failing call among the n_check given, 0 if none fails.  d_result: one device word.
int hash_tape_check_run(const uint32_t* d_tape, const uint64_t* d_prefix, uint64_t n_check, uint64_t n_full, uint64_t n_real, uint64_t code_end, unsigned long long* d_result, zkir::HostPin& pin,
                        hipStream_t s, int* code, uint64_t* call = nullptr) {
  *code = 0;
  if (call) *call = ~0ull;
  if (!n_check) return ZKIR_OK;
  unsigned long long* hr = pin.take_n<unsigned long long>(1);
  if (!hr) HIP_OK(hipErrorOutOfMemory);
  HIP_OK(hipMemsetAsync(d_result, 0xFF, 8, s));
  hipLaunchKernelGGL(hash_tape_check_kernel, dim3(grid_for(n_check)), dim3(NT), 0, s, d_tape, d_prefix, n_check, n_full, n_real, code_end, d_result);
  HIP_OK(hipMemcpyAsync(hr, d_result, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (*hr != ~0ull) { *code = (int)(*hr & 0xFF); if (call) *call = *hr >> 8; }
  return ZKIR_OK;
}

// The allocation-free walk over a hash section in HOST memory that the stand-alone entries place the records with (zkir_prove has the witness's prefix): prefix[k] from
// hashcall::n_cells_of of the record's own fields — never its count word.  n_full: the records that lie in the buffer whole; header_only: record n_full's eight header
// words do, its cells do not; cut: the walk left the buffer (at record n_full).  used: the words of the n_full records and the count word.
struct TapeWalk { uint64_t n_calls = 0, n_full = 0, cells = 0, used = 1; bool header_only = false, cut = false; };
TapeWalk hash_tape_walk(const uint32_t* w, uint64_t avail, uint64_t* prefix /* min(w[0], avail / 8) + 1 entries */) {
  TapeWalk t;
  t.n_calls = w[0];
  uint64_t q = 1;
  for (uint64_t k = 0; k < t.n_calls; k++) {
    if (q + 8 > avail) { t.cut = true; break; }
    const uint32_t* c = w + q;
    prefix[k] = t.cells;
    const uint64_t n = hashcall::n_cells_of((uint64_t)c[1] | ((uint64_t)c[2] << 20), c[3], (uint64_t)c[4] | ((uint64_t)c[5] << 20));
    if (q + 8 + 5 * n > avail) { t.cut = t.header_only = true; break; }
    q += 8 + 5 * n; t.cells += n; t.n_full++;
  }
  if (!t.cut) prefix[t.n_calls] = t.cells;
  t.used = q;
  return t;
}
