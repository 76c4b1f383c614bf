// memcheck.hip — the memory witness of AIR mode 3 ON THE DEVICE: for every load / store row the bytes of its aligned 8-byte cell before the access and
// the time of the cell's previous access, and the touched cells with their final bytes and times.
//
// What a load returns depends on every earlier store to its cell: a chain per CELL, not per run.  The host replay (verify.cpp: zkir_memcheck_witness_of) walks the run once;
// here the accesses are put in ADDRESS-MAJOR order — the key order VERDICT r3 asked for, (cell, time) — and each cell's chain becomes a segment of a scan:
//   1. memkey_kernel     one key per row: (cell index << 26) | row for a load / store (rs1 + sext(imm17), registers read from the trace columns), all-ones otherwise;
//   2. radix sort        rocPRIM, on the whole key: (cell, row) order, each cell's accesses in time order.  (Sorting on the cell bits alone — begin_bit = 26, relying on
//                        stability — comes out UNSORTED from rocPRIM 7.2's merge-sort path, 2^17 < n <= 2^21 keys: scripts/dbg/sort_test.hip reproduces it; begin_bit = 0 is right at every size);
//   3. memelem_kernel    per sorted access: (byte mask, bytes placed at their offset) of a store, nothing for a load; head = first access of its cell;
//   4. segmented scan    an inclusive scan with the "later store overwrites" operator (associative, not commutative), restarting at heads; it also counts the heads.
//                        Three kernels of this file — tile aggregates, their spine, the tiles again with their prefix — 2 reads + 1 write of 16 B per access;
//   5. memout_kernel     old bytes = the program image's (code at 0x1000, data behind it, zero elsewhere: vm.rs:153-170) overlaid with the scan value of the PREVIOUS access of
//                        the cell, old time = that access's row + 1 (0 at a head) -> scattered to the row; the last access of a cell emits the cell's final bytes and time.
// rocPRIM supplies the radix sort — AMD's own device-wide primitive for gfx950; every other kernel is this file's.  (Round 4 used rocprim::inclusive_scan as well: each of its
// calls, the size query included, runs hipGetDeviceProperties on the host — 3 to 6 ms a call in a process that is not the first on its box, 13-22 ms per proof; ZKIR_PROVE_TIMES
// showed it.  The radix sort asks for the architecture once per process and caches it.)
// Refused: an address of 2^40 or more, an executed hash syscall (their memory effect is not stated by the AIR).
// MODE 4, a run WITH hash syscalls (memcheck_device_hash, further down): the same pipeline with 0, 1 or many accesses per row — a count pass and a scan of the counts first (the
// access count is not bounded by the row count), one key per touched cell of every call, the written bytes from the interpreter's zkir_hash_out records — which also builds the
// proof's hash section in place and every touched cell's bytes after its call.
#include <hip/hip_runtime.h>

#include <cstring>
// (only the primitive used: the umbrella header drags in iterators that do not compile here)
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/zkir_amd.h"
#include "hashcall.h"
#include "host.h"

namespace {

constexpr int NT = 256, ROW_BITS = 26;
constexpr uint64_t ROW_MASK = (1ull << ROW_BITS) - 1, NO_KEY = ~0ull;
inline unsigned grid_for(uint64_t n) { return (unsigned)((n + NT - 1) / NT); }

struct MemElem { uint64_t data; uint32_t count; uint8_t mask, head, pad[2]; };      // 16 bytes
static_assert(sizeof(MemElem) == 16, "scan element");
__host__ __device__ __forceinline__ uint64_t expand_mask(uint32_t m) { uint64_t r = 0; for (int k = 0; k < 8; k++) if (m & (1u << k)) r |= 0xFFull << (8 * k); return r; }
struct OverlayOp {       // (a then b): b's bytes over a's; a head restarts the segment; the head count runs through
  __host__ __device__ MemElem operator()(const MemElem& a, const MemElem& b) const {
    MemElem r;
    r.count = a.count + b.count;
    if (b.head) { r.data = b.data; r.mask = b.mask; r.head = 1; }
    else { r.data = (a.data & ~expand_mask(b.mask)) | b.data; r.mask = a.mask | b.mask; r.head = a.head; }
    r.pad[0] = r.pad[1] = 0;
    return r;
  }
};

struct Access { uint64_t ea; uint32_t op, fb; bool mem; };
__device__ __forceinline__ Access access_of(const zkir_trace_columns& t, uint64_t i) {
  const uint32_t w = t.instruction[i], op = w & 0x7F, fa = (w >> 7) & 0xF, fb = (w >> 11) & 0xF;
  const bool load = op >= 0x30 && op <= 0x35, store = op >= 0x38 && op <= 0x3B;
  Access a{0, op, fb, load || store};
  if (a.mem) a.ea = t.registers[(uint64_t)(load ? fb : fa) * t.reg_stride + i] + (uint64_t)((int64_t)(int32_t)(w & 0xFFFF8000u) >> 15);   // rs1 + sext(imm17), wrapping (execute.rs:477-575)
  return a;
}
__device__ __forceinline__ int width_of(uint32_t op) { return op >= 0x38 ? 1 << (op - 0x38) : op <= 0x31 ? 1 : op <= 0x33 ? 2 : op == 0x34 ? 4 : 8; }

__global__ __launch_bounds__(NT) void memkey_kernel(zkir_trace_columns t, uint64_t n_real, uint64_t* __restrict__ keys, uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n_real) return;
  uint64_t key = NO_KEY;
  if (i + 1 < n_real) {                                        // the halt row executes nothing the AIR describes
    const Access a = access_of(t, i);
    if (a.mem) { if (a.ea >> 40) atomicOr(bad, 1u); else key = ((a.ea >> 3) << ROW_BITS) | i; }
    else if (a.op == 0x50) { const uint64_t num = t.registers[(uint64_t)10 * t.reg_stride + i]; if (num >= 3 && num <= 6) atomicOr(bad, 2u); }
  }
  keys[i] = key;
}
__global__ __launch_bounds__(NT) void memelem_kernel(zkir_trace_columns t, uint64_t n, const uint64_t* __restrict__ keys, MemElem* __restrict__ el) {
  const uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (j >= n) return;
  const uint64_t key = keys[j];
  MemElem e{0, 0, 0, 1, {0, 0}};
  if (key != NO_KEY) {
    const uint64_t row = key & ROW_MASK;
    e.head = j == 0 || (keys[j - 1] >> ROW_BITS) != (key >> ROW_BITS);
    e.count = e.head;
    const Access a = access_of(t, row);
    if (a.op >= 0x38) {                                        // a store: the low `width` bytes of rs2, placed at the access's offset in the cell
      const int w = width_of(a.op), off = (int)(a.ea & 7);
      const uint64_t mask = w == 8 ? ~0ull : ((1ull << (8 * w)) - 1);
      e.mask = (uint8_t)(((1u << w) - 1) << off);
      e.data = (t.registers[(uint64_t)a.fb * t.reg_stride + row] & mask) << (8 * off);
    }
  }
  el[j] = e;
}
// ---- the segmented scan: tiles of NT * SCAN_IPT consecutive elements, one block each ------------------------------------------------
constexpr int SCAN_IPT = 8, SCAN_TILE = NT * SCAN_IPT;
__device__ __forceinline__ MemElem elem_identity() { return MemElem{0, 0, 0, 0, {0, 0}}; }        // op(id, b) = b, op(a, id) = a
__device__ __forceinline__ MemElem elem_load(const MemElem* __restrict__ p) { const uint4 v = *reinterpret_cast<const uint4*>(p); MemElem e; memcpy(&e, &v, 16); return e; }
__device__ __forceinline__ void elem_store(MemElem* __restrict__ p, const MemElem& e) { uint4 v; memcpy(&v, &e, 16); *reinterpret_cast<uint4*>(p) = v; }
__device__ __forceinline__ MemElem elem_shfl_up(const MemElem& e, int d) {
  uint32_t w[4]; memcpy(w, &e, 16);
  for (int k = 0; k < 4; k++) w[k] = __shfl_up(w[k], d, 64);
  MemElem r; memcpy(&r, w, 16); return r;
}
// every thread brings the aggregate of its own (consecutive) elements: returns the aggregate of all the threads BEFORE it, and the block's in *total
__device__ __forceinline__ MemElem block_exclusive(const MemElem& agg, MemElem* total) {
  __shared__ MemElem wave_tot[NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const OverlayOp op;
  MemElem inc = agg;
  for (int d = 1; d < 64; d <<= 1) { const MemElem o = elem_shfl_up(inc, d); if (lane >= d) inc = op(o, inc); }
  __syncthreads();                                             // (a second call in one kernel: the readers of the first are done)
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  MemElem exc = elem_shfl_up(inc, 1);
  if (lane == 0) exc = elem_identity();
  MemElem before = elem_identity(), all = elem_identity();
  for (int w = 0; w < NT / 64; w++) { if (w == wave) before = all; all = op(all, wave_tot[w]); }
  *total = all;
  return op(before, exc);
}
__global__ __launch_bounds__(NT) void scan_tiles_kernel(const MemElem* __restrict__ el, uint64_t n, MemElem* __restrict__ part) {
  const uint64_t j0 = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_IPT;
  const OverlayOp op;
  MemElem agg = elem_identity();
  for (int k = 0; k < SCAN_IPT; k++) if (j0 + k < n) agg = op(agg, elem_load(el + j0 + k));
  MemElem tot;
  (void)block_exclusive(agg, &tot);
  if (threadIdx.x == 0) elem_store(part + blockIdx.x, tot);
}
__global__ __launch_bounds__(NT) void scan_spine_kernel(MemElem* __restrict__ part, uint32_t n_tiles) {      // ONE block: part[i] <- the aggregate of the tiles before i
  const uint32_t per = (n_tiles + NT - 1) / NT, i0 = threadIdx.x * per;
  const OverlayOp op;
  MemElem agg = elem_identity();
  for (uint32_t k = 0; k < per; k++) if (i0 + k < n_tiles) agg = op(agg, elem_load(part + i0 + k));
  MemElem tot;
  MemElem run = block_exclusive(agg, &tot);
  for (uint32_t k = 0; k < per; k++) if (i0 + k < n_tiles) { const MemElem e = elem_load(part + i0 + k); elem_store(part + i0 + k, run); run = op(run, e); }
}
__global__ __launch_bounds__(NT) void scan_apply_kernel(const MemElem* __restrict__ el, uint64_t n, const MemElem* __restrict__ part, MemElem* __restrict__ out) {
  const uint64_t j0 = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_IPT;
  const OverlayOp op;
  MemElem e[SCAN_IPT], agg = elem_identity();
  for (int k = 0; k < SCAN_IPT; k++) { e[k] = j0 + k < n ? elem_load(el + j0 + k) : elem_identity(); agg = op(agg, e[k]); }
  MemElem tot;
  MemElem run = op(elem_load(part + blockIdx.x), block_exclusive(agg, &tot));
  for (int k = 0; k < SCAN_IPT; k++) { run = op(run, e[k]); if (j0 + k < n) elem_store(out + j0 + k, run); }
}
inline uint32_t scan_tiles_of(uint64_t n) { return (uint32_t)((n + SCAN_TILE - 1) / SCAN_TILE); }

__device__ __forceinline__ uint64_t image_cell(const uint8_t* __restrict__ image, uint64_t image_len, uint64_t addr) {
  uint64_t v = 0;
  if (addr + 8 <= 0x1000 || addr - 0x1000 >= image_len) return 0;
  for (int k = 0; k < 8; k++) { const uint64_t a = addr + k; if (a >= 0x1000 && a - 0x1000 < image_len) v |= (uint64_t)image[a - 0x1000] << (8 * k); }
  return v;
}
__global__ __launch_bounds__(NT) void memout_kernel(uint64_t n, const uint64_t* __restrict__ keys, const MemElem* __restrict__ sc, const uint8_t* __restrict__ image, uint64_t image_len,
                                                     uint64_t* __restrict__ mem_old, uint32_t* __restrict__ mem_told, uint64_t* __restrict__ cell_addr, uint64_t* __restrict__ cell_bytes,
                                                     uint32_t* __restrict__ cell_time, uint32_t* __restrict__ n_cells) {
  const uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (j >= n) return;
  const uint64_t key = keys[j];
  if (key == NO_KEY) return;
  const uint64_t row = key & ROW_MASK, cell = (key >> ROW_BITS) << 3;
  const uint64_t img = image_cell(image, image_len, cell);
  const bool head = j == 0 || (keys[j - 1] >> ROW_BITS) != (key >> ROW_BITS);
  uint64_t ob = img; uint32_t told = 0;
  if (!head) { const MemElem p = sc[j - 1]; ob = (img & ~expand_mask(p.mask)) | p.data; told = (uint32_t)(keys[j - 1] & ROW_MASK) + 1; }
  mem_old[row] = ob; mem_told[row] = told;
  const uint64_t nk = j + 1 < n ? keys[j + 1] : NO_KEY;
  if (nk == NO_KEY || (nk >> ROW_BITS) != (key >> ROW_BITS)) {  // the cell's last access: its final bytes and time
    const MemElem c = sc[j];
    const uint32_t idx = c.count - 1;
    cell_addr[idx] = cell; cell_bytes[idx] = (img & ~expand_mask(c.mask)) | c.data; cell_time[idx] = (uint32_t)row + 1;
    if (nk == NO_KEY) *n_cells = c.count;
  }
}

// ---- (mode 4) a run WITH hash syscalls: a row has 0, 1 or many accesses -------------------------------------------------------------------------------------------------
//   1. hcount_kernel        per row: 1 access for a load / store, for a hash ECALL (R10 in 3 / 5 / 6, not the halt row) the number of distinct cells under [R11, R11 + R12) and
//                           [R13, R13 + 32) (hashcall::n_cells_of, a closed form); hashcall::in_range is applied here.  Tile totals of (accesses, hash cells, calls);
//   2. hcount_spine_kernel  their exclusive prefix and the run's totals, which the host reads back ONCE: everything behind is sized by them;
//   3. hrows_kernel         the rows again with their prefix: a load / store writes its key at its offset, a hash row its call descriptor (where its keys, its cells' new
//                           bytes and its tape record start) and is held against the interpreter's record of what it wrote;
//   4. hcells_kernel        one thread per HASH ACCESS (a call may touch 131 078 cells while its neighbours touch 8): a binary search over the calls' offsets finds the call,
//                           hashcall::cell_at the cell.  A call lists each cell once: keys stay unique;
//   5. the radix sort, helem_kernel (a hash access writes the part of the call's 32 output bytes that falls into the cell), the segmented scan above, hout_kernel: a load /
//      store row as memout_kernel; a hash access writes [time][four 16-bit pieces of the old bytes] into the call's tape record (hashcall::put_section's layout, built in
//      place; the access of the call's first cell also writes the record's eight header words) and the cell's NEW bytes to a side array in tape order.
struct HCnt { uint64_t acc, hcells; uint32_t calls, pad; };
struct HashCallD { uint64_t in_ptr, len, out_ptr, acc_off, hoff; uint32_t row, kind, n_cells, pad; };      // hoff: hash cells before the call; its record starts at word 1 + 8 * index + 5 * hoff
__device__ __forceinline__ HCnt cnt_add(const HCnt& a, const HCnt& b) { return HCnt{a.acc + b.acc, a.hcells + b.hcells, a.calls + b.calls, 0}; }
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) { const uint32_t lo = __shfl_up((uint32_t)v, d, 64), hi = __shfl_up((uint32_t)(v >> 32), d, 64); return ((uint64_t)hi << 32) | lo; }
__device__ __forceinline__ HCnt cnt_shfl_up(const HCnt& c, int d) { return HCnt{shfl_up64(c.acc, d), shfl_up64(c.hcells, d), __shfl_up(c.calls, d, 64), 0}; }
__device__ __forceinline__ HCnt cnt_block_exclusive(const HCnt& v, HCnt* total) {
  __shared__ HCnt wave_tot[NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  HCnt inc = v;
  for (int d = 1; d < 64; d <<= 1) { const HCnt o = cnt_shfl_up(inc, d); if (lane >= d) inc = cnt_add(o, inc); }
  __syncthreads();
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  HCnt exc = cnt_shfl_up(inc, 1);
  if (lane == 0) exc = HCnt{0, 0, 0, 0};
  HCnt before{0, 0, 0, 0}, all{0, 0, 0, 0};
  for (int w = 0; w < NT / 64; w++) { if (w == wave) before = all; all = cnt_add(all, wave_tot[w]); }
  *total = all;
  return cnt_add(before, exc);
}
struct RowKind { HCnt c; uint64_t a, len, out; uint32_t kind, type; };      // type: 0 no access, 1 load / store (a = the address), 2 hash call (a = the input pointer)
__device__ __forceinline__ RowKind row_kind(const zkir_trace_columns& t, uint64_t i, uint64_t n_real, uint32_t& bad) {
  RowKind r{{0, 0, 0, 0}, 0, 0, 0, 0, 0};
  if (i + 1 >= n_real) return r;                               // the halt row (and the threads past it) executes nothing the AIR describes
  const Access a = access_of(t, i);
  if (a.mem) { if (a.ea >> 40) bad |= 1u; else { r.type = 1; r.a = a.ea; r.c.acc = 1; } }
  else if (a.op == 0x50) {
    const uint64_t num = t.registers[(uint64_t)10 * t.reg_stride + i];
    if (num >= 3 && num <= 6) {
      r.a = t.registers[(uint64_t)11 * t.reg_stride + i]; r.len = t.registers[(uint64_t)12 * t.reg_stride + i]; r.out = t.registers[(uint64_t)13 * t.reg_stride + i]; r.kind = (uint32_t)num;
      if (!hashcall::in_range(r.a, r.len, r.out, r.kind)) bad |= 4u;
      else { r.type = 2; const uint64_t n = hashcall::n_cells_of(r.a, r.len, r.out); r.c = HCnt{n, n, 1, 0}; }
    }
  }
  return r;
}
__global__ __launch_bounds__(NT) void hcount_kernel(zkir_trace_columns t, uint64_t n_real, HCnt* __restrict__ part, uint32_t* __restrict__ bad) {
  __shared__ uint32_t sbad;                                     // the refusal flags of a block: one global atomic per block that has any
  if (threadIdx.x == 0) sbad = 0;
  __syncthreads();
  uint32_t b = 0;
  const RowKind r = row_kind(t, (uint64_t)blockIdx.x * NT + threadIdx.x, n_real, b);
  if (b) atomicOr(&sbad, b);
  HCnt tot;
  (void)cnt_block_exclusive(r.c, &tot);                         // (its barriers order sbad too)
  if (threadIdx.x == 0) { part[blockIdx.x] = tot; if (sbad) atomicOr(bad, sbad); }
}
__global__ __launch_bounds__(NT) void hcount_spine_kernel(HCnt* __restrict__ part, uint32_t n_tiles, HCnt* __restrict__ total) {      // ONE block
  const uint32_t per = (n_tiles + NT - 1) / NT, i0 = threadIdx.x * per;
  HCnt agg{0, 0, 0, 0};
  for (uint32_t k = 0; k < per; k++) if (i0 + k < n_tiles) agg = cnt_add(agg, part[i0 + k]);
  HCnt tot;
  HCnt run = cnt_block_exclusive(agg, &tot);
  for (uint32_t k = 0; k < per; k++) if (i0 + k < n_tiles) { const HCnt e = part[i0 + k]; part[i0 + k] = run; run = cnt_add(run, e); }
  if (threadIdx.x == 0) *total = tot;
}
__global__ __launch_bounds__(NT) void hrows_kernel(zkir_trace_columns t, uint64_t n_real, const HCnt* __restrict__ part, const zkir_hash_out* __restrict__ outs, uint64_t* __restrict__ keys,
                                                    HashCallD* __restrict__ calls, uint32_t* __restrict__ rowcall, uint64_t* __restrict__ mem_old, uint32_t* __restrict__ mem_told,
                                                    uint32_t* __restrict__ bad) {
  __shared__ uint32_t sbad;
  if (threadIdx.x == 0) sbad = 0;
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
  uint32_t b = 0;
  const RowKind r = row_kind(t, i, n_real, b);
  HCnt tot;
  const HCnt at = cnt_add(part[blockIdx.x], cnt_block_exclusive(r.c, &tot));
  if (r.type == 1) keys[at.acc] = ((r.a >> 3) << ROW_BITS) | i;
  else if (r.type == 2) {                                       // (the host has checked that the run has as many calls as records: at.calls indexes both)
    calls[at.calls] = HashCallD{r.a, r.len, r.out, at.acc, at.hcells, (uint32_t)i, r.kind, (uint32_t)r.c.hcells, 0};
    rowcall[i] = at.calls;
    if (outs[at.calls].row != (uint32_t)i) atomicOr(&sbad, 8u);
    mem_old[i] = 0; mem_told[i] = 0;                            // a hash row's own entries stay 0, as in the host replay
  }
  __syncthreads();
  if (threadIdx.x == 0 && sbad) atomicOr(bad, sbad);
}
__global__ __launch_bounds__(NT) void hcells_kernel(const HashCallD* __restrict__ calls, uint32_t n_calls, uint64_t n_hcells, uint64_t* __restrict__ keys) {
  const uint64_t h = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (h >= n_hcells) return;
  uint32_t lo = 0, hi = n_calls;                                // the last call whose hoff <= h
  while (lo + 1 < hi) { const uint32_t m = lo + (hi - lo) / 2; if (calls[m].hoff <= h) lo = m; else hi = m; }
  const HashCallD d = calls[lo];
  const uint64_t r = h - d.hoff;                                // < d.n_cells: the next call's hoff is d.hoff + d.n_cells
  keys[d.acc_off + r] = ((hashcall::cell_at(d.in_ptr, d.len, d.out_ptr, r) >> 3) << ROW_BITS) | d.row;
}
// the calls' cell-offset prefix, kept for the readers of the tape behind the witness (the record checks, the lookup table side): prefix[n_calls] = the total
__global__ __launch_bounds__(NT) void hprefix_kernel(const HashCallD* __restrict__ calls, uint32_t n_calls, uint64_t n_hcells, uint64_t* __restrict__ prefix) {
  const uint32_t k = blockIdx.x * NT + threadIdx.x;
  if (k <= n_calls) prefix[k] = k < n_calls ? calls[k].hoff : n_hcells;
}
__global__ __launch_bounds__(NT) void helem_kernel(zkir_trace_columns t, uint64_t n, const uint64_t* __restrict__ keys, const HashCallD* __restrict__ calls, const uint32_t* __restrict__ rowcall,
                                                    const zkir_hash_out* __restrict__ outs, MemElem* __restrict__ el) {
  const uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (j >= n) return;
  const uint64_t key = keys[j], row = key & ROW_MASK, cell = (key >> ROW_BITS) << 3;
  MemElem e{0, 0, 0, 0, {0, 0}};
  e.head = j == 0 || (keys[j - 1] >> ROW_BITS) != (key >> ROW_BITS);
  e.count = e.head;
  const Access a = access_of(t, row);
  if (a.mem) {
    if (a.op >= 0x38) {
      const int w = width_of(a.op), off = (int)(a.ea & 7);
      const uint64_t mask = w == 8 ? ~0ull : ((1ull << (8 * w)) - 1);
      e.mask = (uint8_t)(((1u << w) - 1) << off);
      e.data = (t.registers[(uint64_t)a.fb * t.reg_stride + row] & mask) << (8 * off);
    }
  } else {                                                      // a hash access: the part of the call's 32 output bytes that falls into this cell (nothing when it is input only)
    const uint32_t ci = rowcall[row];
    const uint64_t out = calls[ci].out_ptr;
    for (int k = 0; k < 8; k++) { const uint64_t o = cell + k - out; if (o < 32) { e.mask |= (uint8_t)(1u << k); e.data |= (uint64_t)outs[ci].bytes[o] << (8 * k); } }
  }
  elem_store(el + j, e);
}
__global__ __launch_bounds__(NT) void hout_kernel(zkir_trace_columns t, uint64_t n, const uint64_t* __restrict__ keys, const MemElem* __restrict__ sc, const uint8_t* __restrict__ image,
                                                   uint64_t image_len, const HashCallD* __restrict__ calls, uint32_t n_calls, const uint32_t* __restrict__ rowcall, uint64_t* __restrict__ mem_old,
                                                   uint32_t* __restrict__ mem_told, uint32_t* __restrict__ tape, uint64_t* __restrict__ side, uint64_t* __restrict__ cell_addr,
                                                   uint64_t* __restrict__ cell_bytes, uint32_t* __restrict__ cell_time, uint32_t* __restrict__ n_cells) {
  const uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (j >= n) return;
  if (j == 0) tape[0] = n_calls;
  const uint64_t key = keys[j], row = key & ROW_MASK, cell = (key >> ROW_BITS) << 3;
  const uint64_t img = image_cell(image, image_len, cell);
  const bool head = j == 0 || (keys[j - 1] >> ROW_BITS) != (key >> ROW_BITS);
  uint64_t ob = img; uint32_t told = 0;
  if (!head) { const MemElem p = elem_load(sc + j - 1); ob = (img & ~expand_mask(p.mask)) | p.data; told = (uint32_t)(keys[j - 1] & ROW_MASK) + 1; }
  const MemElem c = elem_load(sc + j);
  const uint64_t nb = (img & ~expand_mask(c.mask)) | c.data;    // the cell's bytes after this access
  const uint32_t w = t.instruction[row], op = w & 0x7F;
  if (op != 0x50) { mem_old[row] = ob; mem_told[row] = told; }
  else {
    const uint32_t ci = rowcall[row];
    const HashCallD d = calls[ci];
    const uint64_t r = hashcall::rank_of(d.in_ptr, d.len, d.out_ptr, cell);       // < d.n_cells: the key was made by cell_at
    uint32_t* rec = tape + (1 + 8 * (uint64_t)ci + 5 * d.hoff);
    if (r == 0) {
      rec[0] = d.row; rec[1] = (uint32_t)(d.in_ptr & 0xFFFFF); rec[2] = (uint32_t)(d.in_ptr >> 20); rec[3] = (uint32_t)d.len;
      rec[4] = (uint32_t)(d.out_ptr & 0xFFFFF); rec[5] = (uint32_t)(d.out_ptr >> 20); rec[6] = d.kind; rec[7] = d.n_cells;
    }
    uint32_t* q = rec + 8 + 5 * r;
    q[0] = told; for (int k = 0; k < 4; k++) q[1 + k] = (uint32_t)((ob >> (16 * k)) & 0xFFFF);
    side[d.hoff + r] = nb;
  }
  if (j + 1 == n || (keys[j + 1] >> ROW_BITS) != (key >> ROW_BITS)) {       // the cell's last access: its final bytes and time
    const uint32_t idx = c.count - 1;
    cell_addr[idx] = cell; cell_bytes[idx] = nb; cell_time[idx] = (uint32_t)row + 1;
    if (j + 1 == n) *n_cells = c.count;
  }
}

int dev_fail(const char* what, hipError_t e) { zkir::set_last_error({ZKIR_ERR_DEVICE, std::string("memcheck: ") + what + ": " + hipGetErrorString(e)}); return ZKIR_ERR_DEVICE; }
#define MC_OK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return dev_fail(#x, e_); } while (0)
size_t sort_tmp_bytes(uint64_t n) { size_t t = 0; (void)rocprim::radix_sort_keys(nullptr, t, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)n, 0, 64, (hipStream_t)0); return t; }

}  // namespace

namespace zkir {

HostPin::~HostPin() { for (auto& b : blocks) (void)hipHostFree(b.first); }
void* HostPin::take(size_t bytes) {
  const size_t need = (bytes + 255) & ~(size_t)255;
  for (; cur < blocks.size(); cur++, off = 0)
    if (off + need <= blocks[cur].second) { void* p = blocks[cur].first + off; off += need; return p; }
  size_t total = 0;
  for (auto& b : blocks) total += b.second;
  const size_t sz = std::max(need, std::max(total, (size_t)4 << 20));     // geometric: a context settles on a handful of blocks
  void* p = nullptr;
  if (hipHostMalloc(&p, sz, hipHostMallocDefault) != hipSuccess || !p) { (void)hipGetLastError(); return nullptr; }
  blocks.push_back({(unsigned char*)p, sz});
  cur = blocks.size() - 1; off = need;
  return p;
}

// scratch: device memory, at least memcheck_scratch_bytes(n_real) bytes, 256-byte aligned.  mem_old / mem_told: device [n_real] (rows that are no load / store are left
// untouched).  cells: host vectors, by increasing address.  pin: staging of the copies (host.h).  Synchronises the stream.
size_t memcheck_scratch_bytes(uint64_t n_real, uint64_t image_len) {
  const size_t tmp = sort_tmp_bytes(n_real) + 256;
  return tmp + (size_t)scan_tiles_of(n_real) * 16 + 256 + (size_t)n_real * (8 + 8 + 16 + 16 + 8 + 8 + 4) + ((image_len + 255) & ~(size_t)255) + 4096;
}
int memcheck_device(const zkir_trace_columns* trace, uint64_t n_real, const uint8_t* blob, size_t blob_len, void* scratch, size_t scratch_bytes, uint64_t* mem_old, uint32_t* mem_told,
                    std::vector<uint64_t>& cell_addr, std::vector<uint64_t>& cell_bytes, std::vector<uint32_t>& cell_time, HostPin& pin, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const bool dbg_t = getenv("ZKIR_PROVE_TIMES") != nullptr;      // diagnostics: host wall time of the phases on stderr
  const auto t0_ = std::chrono::steady_clock::now();
  const bool dbg_sync = dbg_t && getenv("ZKIR_PROVE_TIMES")[0] == '2';   // (= 2: a synchronisation at every lap: which phase waits)
  auto lap = [&](const char* what) { if (dbg_sync) (void)hipStreamSynchronize(s); if (dbg_t) fprintf(stderr, "  memcheck %s: %.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count()); };
  if (!trace || !blob || blob_len < 32 || !scratch || !mem_old || !mem_told || n_real == 0 || n_real > (1ull << ROW_BITS)) { set_last_error({ZKIR_ERR_ARGUMENT, "memcheck_device: bad argument"}); return ZKIR_ERR_ARGUMENT; }
  uint32_t code_size, data_size; memcpy(&code_size, blob + 16, 4); memcpy(&data_size, blob + 20, 4);
  uint64_t image_len = (uint64_t)code_size + data_size;
  if (32 + image_len > blob_len) image_len = 0;
  if (scratch_bytes < memcheck_scratch_bytes(n_real, image_len)) { set_last_error({ZKIR_ERR_ARGUMENT, "memcheck_device: scratch too small"}); return ZKIR_ERR_ARGUMENT; }
  lap("entry");
  const size_t tmp_bytes = (sort_tmp_bytes(n_real) + 255) & ~(size_t)255;
  const uint32_t n_tiles = scan_tiles_of(n_real);
  lap("size query");
  unsigned char* p = (unsigned char*)scratch;
  auto take = [&](size_t bytes) { unsigned char* q = p; p += (bytes + 255) & ~(size_t)255; return q; };
  void* tmp = take(tmp_bytes); MemElem* part = (MemElem*)take((size_t)n_tiles * 16);
  uint64_t* keys = (uint64_t*)take(n_real * 8); uint64_t* skeys = (uint64_t*)take(n_real * 8);
  MemElem* el = (MemElem*)take(n_real * 16); MemElem* sc = (MemElem*)take(n_real * 16);
  uint64_t* d_ca = (uint64_t*)take(n_real * 8); uint64_t* d_cb = (uint64_t*)take(n_real * 8); uint32_t* d_ct = (uint32_t*)take(n_real * 4);
  uint8_t* d_img = (uint8_t*)take(image_len + 1); uint32_t* d_flags = (uint32_t*)take(256);      // [0] = refusal flags, [1] = the cell count
  MC_OK(hipMemsetAsync(d_flags, 0, 8, s));
  if (image_len) {
    void* h = pin.take(image_len);
    if (!h) return dev_fail("pinned staging", hipErrorOutOfMemory);
    memcpy(h, blob + 32, image_len);
    MC_OK(hipMemcpyAsync(d_img, h, image_len, hipMemcpyHostToDevice, s));
  }
  lap("image H2D");
  hipLaunchKernelGGL(memkey_kernel, dim3(grid_for(n_real)), dim3(NT), 0, s, *trace, n_real, keys, d_flags);
  size_t tb = tmp_bytes;
  lap("keys");
  MC_OK(rocprim::radix_sort_keys(tmp, tb, keys, skeys, (size_t)n_real, 0, 63, s));      // the keys are 37 + 26 = 63 bits; the all-ones keys of the rows that are no load / store are the largest on those bits too (one digit pass fewer)
  lap("sort");
  hipLaunchKernelGGL(memelem_kernel, dim3(grid_for(n_real)), dim3(NT), 0, s, *trace, n_real, skeys, el);
  lap("elems");
  hipLaunchKernelGGL(scan_tiles_kernel, dim3(n_tiles), dim3(NT), 0, s, el, n_real, part);
  hipLaunchKernelGGL(scan_spine_kernel, dim3(1), dim3(NT), 0, s, part, n_tiles);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(n_tiles), dim3(NT), 0, s, el, n_real, part, sc);
  lap("scan");
  hipLaunchKernelGGL(memout_kernel, dim3(grid_for(n_real)), dim3(NT), 0, s, n_real, skeys, sc, d_img, image_len, mem_old, mem_told, d_ca, d_cb, d_ct, d_flags + 1);
  uint32_t flags[2] = {0, 0};
  MC_OK(hipMemcpyAsync(flags, d_flags, 8, hipMemcpyDeviceToHost, s));
  MC_OK(hipStreamSynchronize(s));
  lap("out, synchronised");
  MC_OK(hipGetLastError());
  if (flags[0] & 1) { set_last_error({ZKIR_ERR_ARGUMENT, "zkir_prove (mode 3): the run accesses an address of 2^40 or more: it has no proof in this AIR (addr_limbs = 2, config.rs:30)"}); return ZKIR_ERR_ARGUMENT; }
  if (flags[0] & 2) { set_last_error({ZKIR_ERR_ARGUMENT, "zkir_prove (mode 3): the run executes a hash syscall: its memory effect is not stated by the AIR"}); return ZKIR_ERR_ARGUMENT; }
  const size_t nc = flags[1];
  cell_addr.resize(nc); cell_bytes.resize(nc); cell_time.resize(nc);
  if (nc) {
    uint64_t* ha = pin.take_n<uint64_t>(nc); uint64_t* hb = pin.take_n<uint64_t>(nc); uint32_t* ht = pin.take_n<uint32_t>(nc);
    if (!ha || !hb || !ht) return dev_fail("pinned staging", hipErrorOutOfMemory);
    MC_OK(hipMemcpyAsync(ha, d_ca, nc * 8, hipMemcpyDeviceToHost, s));
    MC_OK(hipMemcpyAsync(hb, d_cb, nc * 8, hipMemcpyDeviceToHost, s));
    MC_OK(hipMemcpyAsync(ht, d_ct, nc * 4, hipMemcpyDeviceToHost, s));
    MC_OK(hipStreamSynchronize(s));
    memcpy(cell_addr.data(), ha, nc * 8); memcpy(cell_bytes.data(), hb, nc * 8); memcpy(cell_time.data(), ht, nc * 4);
  }
  lap("cells copied");
  return ZKIR_OK;
}

HashWitness::~HashWitness() { if (d_block) (void)hipFree(d_block); }

namespace { struct DevBuf { void* p = nullptr; ~DevBuf() { if (p) (void)hipFree(p); } }; }
int memcheck_device_hash(const zkir_trace_columns* trace, uint64_t n_real, const uint8_t* blob, size_t blob_len, const zkir_hash_out* outs, uint64_t n_outs, uint64_t* mem_old,
                         uint32_t* mem_told, std::vector<uint64_t>& cell_addr, std::vector<uint64_t>& cell_bytes, std::vector<uint32_t>& cell_time, HashWitness& hw, HostPin& pin,
                         void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const bool dbg_t = getenv("ZKIR_PROVE_TIMES") != nullptr;
  const auto t0_ = std::chrono::steady_clock::now();
  const bool dbg_sync = dbg_t && getenv("ZKIR_PROVE_TIMES")[0] == '2';
  auto lap = [&](const char* what) { if (dbg_sync) (void)hipStreamSynchronize(s); if (dbg_t) fprintf(stderr, "  memcheck (hash) %s: %.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count()); };
  auto refuse = [](const std::string& m) { set_last_error({ZKIR_ERR_ARGUMENT, m}); return ZKIR_ERR_ARGUMENT; };
  if (!trace || !blob || blob_len < 32 || !mem_old || !mem_told || (!outs && n_outs) || n_real == 0 || n_real > (1ull << ROW_BITS)) return refuse("memcheck_device_hash: bad argument");
  uint32_t code_size, data_size; memcpy(&code_size, blob + 16, 4); memcpy(&data_size, blob + 20, 4);
  uint64_t image_len = (uint64_t)code_size + data_size;
  if (32 + image_len > blob_len) image_len = 0;
  // the records: in row order, one per executed call; the halt row executes nothing the AIR describes, a record the log holds for it is ignored
  uint64_t n_use = n_outs;
  if (n_use && (uint64_t)outs[n_use - 1].row + 1 >= n_real) n_use--;
  for (uint64_t k = 0; k < n_use; k++)
    if ((uint64_t)outs[k].row + 1 >= n_real || (k && outs[k].row <= outs[k - 1].row)) return refuse("zkir_prove (mode 4): the hash-output records of the public inputs (hash_outs) are not in strictly increasing row order below the halt row");
  // ---- the count pass: everything behind it is sized by its totals ----
  const uint32_t n_rt = grid_for(n_real);
  DevBuf small;
  MC_OK(hipMalloc(&small.p, (size_t)n_rt * sizeof(HCnt) + 512));
  HCnt* d_part = (HCnt*)small.p; HCnt* d_tot = (HCnt*)((unsigned char*)small.p + (((size_t)n_rt * sizeof(HCnt) + 255) & ~(size_t)255)); uint32_t* d_flags = (uint32_t*)((unsigned char*)d_tot + 128);   // [0] refusal flags, [1] the cell count
  MC_OK(hipMemsetAsync(d_flags, 0, 8, s));
  hipLaunchKernelGGL(hcount_kernel, dim3(n_rt), dim3(NT), 0, s, *trace, n_real, d_part, d_flags);
  hipLaunchKernelGGL(hcount_spine_kernel, dim3(1), dim3(NT), 0, s, d_part, n_rt, d_tot);
  struct { HCnt tot; uint32_t flags[2]; }* hb = (decltype(hb))pin.take(sizeof *hb);
  if (!hb) return dev_fail("pinned staging", hipErrorOutOfMemory);
  MC_OK(hipMemcpyAsync(&hb->tot, d_tot, sizeof(HCnt), hipMemcpyDeviceToHost, s));
  MC_OK(hipMemcpyAsync(hb->flags, d_flags, 8, hipMemcpyDeviceToHost, s));
  MC_OK(hipStreamSynchronize(s));
  MC_OK(hipGetLastError());
  lap("count, read back");
  if (hb->flags[0] & 1) return refuse("zkir_prove (mode 3): the run accesses an address of 2^40 or more: it has no proof in this AIR (addr_limbs = 2, config.rs:30)");
  if (hb->flags[0] & 4) return refuse("zkir_prove (mode 4): a hash syscall of the run is outside what a proof states (kind 3 / 5 / 6, at most 1 MiB of input, buffers below 2^40, a SHA-256 output at a multiple of 4)");
  const uint64_t A = hb->tot.acc, H = hb->tot.hcells, n_calls = hb->tot.calls;
  if (n_calls != n_use) {
    char m[256]; snprintf(m, sizeof m, "zkir_prove (mode 4): the run makes %llu hash syscalls before its halt row and the public inputs' hash_outs record %llu: they must be the run's own (zkir_public_inputs_of)",
                          (unsigned long long)n_calls, (unsigned long long)n_use);
    return refuse(m);
  }
  const uint64_t n_words = 1 + 8 * n_calls + 5 * H;
  hw.n_words = n_words; hw.n_hcells = H; hw.n_calls = n_calls;
  const char* oom = "zkir_prove (mode 4): out of device memory for the memory witness of a run with hash syscalls (its size follows the cells the calls touch)";
  if (A >> 32) { set_last_error({ZKIR_ERR_DEVICE, oom}); return ZKIR_ERR_DEVICE; }
  if (hipMalloc(&hw.d_block, H * 8 + (n_calls + 1) * 8 + n_words * 4 + 256) != hipSuccess) { (void)hipGetLastError(); hw.d_block = nullptr; set_last_error({ZKIR_ERR_DEVICE, oom}); return ZKIR_ERR_DEVICE; }
  uint64_t* d_side = (uint64_t*)hw.d_block; uint64_t* d_prefix = d_side + H; uint32_t* d_tape = (uint32_t*)(d_prefix + n_calls + 1);
  hw.d_tape = d_tape; hw.d_side = d_side; hw.d_prefix = d_prefix;
  MC_OK(hipMemsetAsync(d_tape, 0, 4, s));                      // (a run whose only hash call sits on the halt row: an empty tape)
  MC_OK(hipMemsetAsync(d_prefix, 0, 8, s));
  cell_addr.clear(); cell_bytes.clear(); cell_time.clear();
  if (A) {
    const size_t tmp_bytes = (sort_tmp_bytes(A) + 255) & ~(size_t)255;
    const uint32_t n_tiles = scan_tiles_of(A);
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t total = tmp_bytes + al((size_t)n_tiles * 16) + 2 * al(A * 8) + 2 * al(A * 16) + 2 * al(A * 8) + al(A * 4) + al(image_len + 1) + al((n_calls + 1) * sizeof(HashCallD)) +
                         al((n_use + 1) * sizeof(zkir_hash_out)) + al(n_real * 4);
    DevBuf big;
    if (hipMalloc(&big.p, total) != hipSuccess) { (void)hipGetLastError(); big.p = nullptr; set_last_error({ZKIR_ERR_DEVICE, oom}); return ZKIR_ERR_DEVICE; }
    unsigned char* p = (unsigned char*)big.p;
    auto take = [&](size_t bytes) { unsigned char* q = p; p += al(bytes); return q; };
    void* tmp = take(tmp_bytes); MemElem* part = (MemElem*)take((size_t)n_tiles * 16);
    uint64_t* keys = (uint64_t*)take(A * 8); uint64_t* skeys = (uint64_t*)take(A * 8);
    MemElem* el = (MemElem*)take(A * 16); MemElem* sc = (MemElem*)take(A * 16);
    uint64_t* d_ca = (uint64_t*)take(A * 8); uint64_t* d_cb = (uint64_t*)take(A * 8); uint32_t* d_ct = (uint32_t*)take(A * 4);
    uint8_t* d_img = (uint8_t*)take(image_len + 1); HashCallD* d_calls = (HashCallD*)take((n_calls + 1) * sizeof(HashCallD));
    zkir_hash_out* d_outs = (zkir_hash_out*)take((n_use + 1) * sizeof(zkir_hash_out)); uint32_t* d_rowcall = (uint32_t*)take(n_real * 4);
    if (image_len) {
      void* h = pin.take(image_len);
      if (!h) return dev_fail("pinned staging", hipErrorOutOfMemory);
      memcpy(h, blob + 32, image_len);
      MC_OK(hipMemcpyAsync(d_img, h, image_len, hipMemcpyHostToDevice, s));
    }
    if (n_use) {
      void* h = pin.take(n_use * sizeof(zkir_hash_out));
      if (!h) return dev_fail("pinned staging", hipErrorOutOfMemory);
      memcpy(h, outs, n_use * sizeof(zkir_hash_out));
      MC_OK(hipMemcpyAsync(d_outs, h, n_use * sizeof(zkir_hash_out), hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(hrows_kernel, dim3(n_rt), dim3(NT), 0, s, *trace, n_real, d_part, d_outs, keys, d_calls, d_rowcall, mem_old, mem_told, d_flags);
    if (H) hipLaunchKernelGGL(hcells_kernel, dim3(grid_for(H)), dim3(NT), 0, s, d_calls, (uint32_t)n_calls, H, keys);
    if (n_calls) hipLaunchKernelGGL(hprefix_kernel, dim3(grid_for(n_calls + 1)), dim3(NT), 0, s, d_calls, (uint32_t)n_calls, H, d_prefix);
    lap("keys");
    size_t tb = tmp_bytes;
    MC_OK(rocprim::radix_sort_keys(tmp, tb, keys, skeys, (size_t)A, 0, 63, s));
    lap("sort");
    hipLaunchKernelGGL(helem_kernel, dim3(grid_for(A)), dim3(NT), 0, s, *trace, A, skeys, d_calls, d_rowcall, d_outs, el);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(n_tiles), dim3(NT), 0, s, el, A, part);
    hipLaunchKernelGGL(scan_spine_kernel, dim3(1), dim3(NT), 0, s, part, n_tiles);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(n_tiles), dim3(NT), 0, s, el, A, part, sc);
    lap("elems, scan");
    hipLaunchKernelGGL(hout_kernel, dim3(grid_for(A)), dim3(NT), 0, s, *trace, A, skeys, sc, d_img, image_len, d_calls, (uint32_t)n_calls, d_rowcall, mem_old, mem_told, d_tape, d_side, d_ca, d_cb,
                       d_ct, d_flags + 1);
    MC_OK(hipMemcpyAsync(hb->flags, d_flags, 8, hipMemcpyDeviceToHost, s));
    MC_OK(hipStreamSynchronize(s));
    MC_OK(hipGetLastError());
    lap("out, synchronised");
    if (hb->flags[0] & 8) return refuse("zkir_prove (mode 4): the hash-output records of the public inputs (hash_outs) are not those of the run's hash rows, row for row");
    const size_t nc = hb->flags[1];
    cell_addr.resize(nc); cell_bytes.resize(nc); cell_time.resize(nc);
    if (nc) {
      uint64_t* ha = pin.take_n<uint64_t>(nc); uint64_t* hbv = pin.take_n<uint64_t>(nc); uint32_t* ht = pin.take_n<uint32_t>(nc);
      if (!ha || !hbv || !ht) return dev_fail("pinned staging", hipErrorOutOfMemory);
      MC_OK(hipMemcpyAsync(ha, d_ca, nc * 8, hipMemcpyDeviceToHost, s));
      MC_OK(hipMemcpyAsync(hbv, d_cb, nc * 8, hipMemcpyDeviceToHost, s));
      MC_OK(hipMemcpyAsync(ht, d_ct, nc * 4, hipMemcpyDeviceToHost, s));
      MC_OK(hipStreamSynchronize(s));
      memcpy(cell_addr.data(), ha, nc * 8); memcpy(cell_bytes.data(), hbv, nc * 8); memcpy(cell_time.data(), ht, nc * 4);
    }
  }
  // the tape: copied to the host ONCE (the proof carries it); the cells' new bytes stay on the device, where the table side reads them
  uint32_t* ht_ = pin.take_n<uint32_t>(n_words);
  if (!ht_) return dev_fail("pinned staging", hipErrorOutOfMemory);
  MC_OK(hipMemcpyAsync(ht_, d_tape, n_words * 4, hipMemcpyDeviceToHost, s));
  MC_OK(hipStreamSynchronize(s));
  hw.h_tape = ht_;
  lap("tape copied");
  return ZKIR_OK;
}

}  // namespace zkir

// The device witness on its own (tests: compared entry for entry with zkir_memcheck_witness_of's host replay).  trace = DEVICE columns of a whole run; mem_old / mem_told: HOST
// arrays of n_real entries (zero where the row is no load / store); cells: HOST arrays of capacity `cap`; *n_cells receives the count (ZKIR_ERR_ARGUMENT if it exceeds cap).
extern "C" int zkir_memcheck_witness_device(const zkir_trace_columns* trace, uint64_t n_real, const uint8_t* blob, size_t blob_len, uint64_t* mem_old, uint32_t* mem_told, uint64_t* cell_addr,
                                            uint64_t* cell_bytes, uint32_t* cell_time, uint64_t cap, uint64_t* n_cells, void* stream) {
  if (!trace || !blob || !mem_old || !mem_told || !n_cells || n_real == 0) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_memcheck_witness_device: null argument"}); return ZKIR_ERR_ARGUMENT; }
  const size_t sb = zkir::memcheck_scratch_bytes(n_real, blob_len);
  void* scratch = nullptr; uint64_t* d_old = nullptr; uint32_t* d_told = nullptr;
  if (hipMalloc(&scratch, sb) != hipSuccess || hipMalloc((void**)&d_old, n_real * 8) != hipSuccess || hipMalloc((void**)&d_told, n_real * 4) != hipSuccess) {
    (void)hipFree(scratch); (void)hipFree(d_old); (void)hipFree(d_told);
    zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_memcheck_witness_device: out of device memory"}); return ZKIR_ERR_DEVICE;
  }
  if (hipMemsetAsync(d_old, 0, n_real * 8, (hipStream_t)stream) != hipSuccess || hipMemsetAsync(d_told, 0, n_real * 4, (hipStream_t)stream) != hipSuccess) {
    (void)hipFree(scratch); (void)hipFree(d_old); (void)hipFree(d_told); return dev_fail("clearing the witness columns", hipGetLastError());
  }
  std::vector<uint64_t> ca, cb; std::vector<uint32_t> ct;
  zkir::HostPin pin;
  int rc = zkir::memcheck_device(trace, n_real, blob, blob_len, scratch, sb, d_old, d_told, ca, cb, ct, pin, stream);
  if (rc == ZKIR_OK) {
    uint64_t* ho = pin.take_n<uint64_t>(n_real); uint32_t* ht = pin.take_n<uint32_t>(n_real);
    if (!ho || !ht) { (void)hipFree(scratch); (void)hipFree(d_old); (void)hipFree(d_told); return dev_fail("pinned staging", hipErrorOutOfMemory); }
    const hipError_t e1 = hipMemcpy(ho, d_old, n_real * 8, hipMemcpyDeviceToHost), e2 = hipMemcpy(ht, d_told, n_real * 4, hipMemcpyDeviceToHost);
    if (e1 != hipSuccess || e2 != hipSuccess) { (void)hipFree(scratch); (void)hipFree(d_old); (void)hipFree(d_told); return dev_fail("copying the witness back", e1 != hipSuccess ? e1 : e2); }
    memcpy(mem_old, ho, n_real * 8); memcpy(mem_told, ht, n_real * 4);
    *n_cells = ca.size();
    if (ca.size() > cap) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_memcheck_witness_device: more cells than the caller's buffers hold"}); rc = ZKIR_ERR_ARGUMENT; }
    else if (!ca.empty()) { memcpy(cell_addr, ca.data(), ca.size() * 8); memcpy(cell_bytes, cb.data(), cb.size() * 8); memcpy(cell_time, ct.data(), ct.size() * 4); }
  }
  (void)hipFree(scratch); (void)hipFree(d_old); (void)hipFree(d_told);
  return rc;
}

extern "C" int zkir_memcheck_witness_device_mode(const zkir_trace_columns* trace, uint64_t n_real, const uint8_t* blob, size_t blob_len, uint32_t mode, const zkir_hash_out* hash_outs,
                                                 uint64_t n_hash_outs, uint64_t* mem_old, uint32_t* mem_told, uint64_t* cell_addr, uint64_t* cell_bytes, uint32_t* cell_time, uint64_t cap,
                                                 uint64_t* n_cells, uint32_t* hash_words, uint64_t hash_cap_words, uint64_t* n_hash_words, void* stream) {
  if (mode == 3) return zkir_memcheck_witness_device(trace, n_real, blob, blob_len, mem_old, mem_told, cell_addr, cell_bytes, cell_time, cap, n_cells, stream);
  if (mode != 4 || !trace || !blob || !mem_old || !mem_told || !n_cells || !n_hash_words || n_real == 0) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_memcheck_witness_device_mode: mode must be 3 or 4, and no argument null"}); return ZKIR_ERR_ARGUMENT; }
  uint64_t* d_old = nullptr; uint32_t* d_told = nullptr;
  if (hipMalloc((void**)&d_old, n_real * 8) != hipSuccess || hipMalloc((void**)&d_told, n_real * 4) != hipSuccess) {
    (void)hipFree(d_old); (void)hipFree(d_told);
    zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_memcheck_witness_device_mode: out of device memory"}); return ZKIR_ERR_DEVICE;
  }
  std::vector<uint64_t> ca, cb; std::vector<uint32_t> ct;
  zkir::HostPin pin;
  zkir::HashWitness hw;
  int rc = ZKIR_OK;
  if (hipMemsetAsync(d_old, 0, n_real * 8, (hipStream_t)stream) != hipSuccess || hipMemsetAsync(d_told, 0, n_real * 4, (hipStream_t)stream) != hipSuccess) rc = dev_fail("clearing the witness columns", hipGetLastError());
  if (rc == ZKIR_OK) rc = zkir::memcheck_device_hash(trace, n_real, blob, blob_len, hash_outs, n_hash_outs, d_old, d_told, ca, cb, ct, hw, pin, stream);
  if (rc == ZKIR_OK) {
    const hipError_t e1 = hipMemcpy(mem_old, d_old, n_real * 8, hipMemcpyDeviceToHost), e2 = hipMemcpy(mem_told, d_told, n_real * 4, hipMemcpyDeviceToHost);
    if (e1 != hipSuccess || e2 != hipSuccess) rc = dev_fail("copying the witness back", e1 != hipSuccess ? e1 : e2);
  }
  if (rc == ZKIR_OK) {
    *n_cells = ca.size(); *n_hash_words = hw.n_words;
    if (ca.size() > cap || hw.n_words > hash_cap_words || (hw.n_words && !hash_words)) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_memcheck_witness_device_mode: more cells / hash-section words than the caller's buffers hold"}); rc = ZKIR_ERR_ARGUMENT; }
    else {
      if (!ca.empty()) { memcpy(cell_addr, ca.data(), ca.size() * 8); memcpy(cell_bytes, cb.data(), cb.size() * 8); memcpy(cell_time, ct.data(), ct.size() * 4); }
      memcpy(hash_words, hw.h_tape, hw.n_words * 4);
    }
  }
  (void)hipFree(d_old); (void)hipFree(d_told);
  return rc;
}
