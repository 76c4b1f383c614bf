// verify.cpp — the product's verifier of ZKIR-STARK proofs (format v10: whole runs, segments of a run, chains of segments) and the
// public-input helpers; host only, no device.
//
// Self-defined stages (the reference has no prover or verifier: SURVEY.md F1 / a17, N4).  Independent of oracle/: Montgomery
// arithmetic (babybear.h), the product's Poseidon2 (poseidon2.h) and the product's constraint list (air.h, the same template the
// quotient kernel instantiates); tests/ compare its verdicts with the oracle's so::verify on valid, tampered and cheating proofs.
// Transcript and proof layout: see zkir_prove (stark_prove.inl) and DESIGN.md §8.8.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <atomic>
#include <thread>
#include <vector>

#include "../../include/zkir_amd.h"
#include "air.h"
#include "babybear.h"
#include "fri_shape.h"
#include "host.h"
#include "hashcall.h"
#include "poseidon2.h"
#include "verify_stages.h"

namespace {

using bb::E4;
constexpr int LOG_FINAL = air::LOG_FINAL, NS = air::N_STATE, HEADER_WORDS = 21 + 2 * NS;   // (queries / grinding bits: the proof's own, air.h; the version: the mode's)
constexpr uint32_t PROOF_MAGIC = 0x46504B5Au;

const p2::Consts& consts() { static const p2::Consts c = [] { p2::Consts k; p2::generate(k); return k; }(); return c; }

// The permutation on a state of Montgomery words (R v, canonical range) in the hash kernels' formulation (p2::permute_scaled: a quarter fewer host instructions than
// p2::permute; the same function — tests/test_stark_oracle.py compares both with the oracle's textbook permutation)
inline void permute_m(uint32_t* st) {
  const p2::Consts& c = consts();
  const uint32_t k_in = bb::from_mont(c.in_scale), ko_m = bb::to_mont(c.out_scale);
  uint32_t s[p2::T];
  for (int i = 0; i < p2::T; i++) s[i] = bb::mont_mul_lazy(st[i], k_in);
  p2::permute_scaled(s, c);
  for (int i = 0; i < p2::T; i++) st[i] = bb::mont_mul(s[i], ko_m);
}

// canonical digests / compressions on top of the Montgomery permutation
void hash_elems(const uint32_t* in, size_t n, uint32_t out[4]) {          // overwrite-mode sponge, rate 8 (so::hash_elems)
  uint32_t s[p2::T] = {0};
  for (size_t off = 0; off < n; off += p2::RATE) {
    const size_t len = n - off < (size_t)p2::RATE ? n - off : (size_t)p2::RATE;
    for (size_t i = 0; i < len; i++) s[i] = bb::to_mont(in[off + i]);
    permute_m(s);
  }
  if (n == 0) permute_m(s);
  for (int i = 0; i < 4; i++) out[i] = bb::from_mont(s[i]);
}
void compress(const uint32_t* l, const uint32_t* r, uint32_t out[4]) {
  uint32_t s[p2::T] = {0};
  for (int i = 0; i < 4; i++) { s[i] = bb::to_mont(l[i]); s[4 + i] = bb::to_mont(r[i]); }
  permute_m(s);
  for (int i = 0; i < 4; i++) out[i] = bb::from_mont(s[i]);
}
bool check_path(const uint32_t* leaf, size_t idx, const uint32_t* path, int depth, const uint32_t* root) {
  uint32_t node[4]; memcpy(node, leaf, 16);
  for (int d = 0; d < depth; d++) { uint32_t nx[4]; if (idx & 1) compress(path + 4 * d, node, nx); else compress(node, path + 4 * d, nx); memcpy(node, nx, 16); idx >>= 1; }
  return !memcmp(node, root, 16);
}

struct Challenger {                                                        // duplex sponge, Montgomery state, canonical in / out
  uint32_t st[p2::T] = {0};
  std::vector<uint32_t> in, out;
  void duplex() { for (size_t i = 0; i < in.size(); i++) st[i] = bb::to_mont(in[i]); in.clear(); permute_m(st); out.clear(); for (int i = 0; i < p2::RATE; i++) out.push_back(bb::from_mont(st[i])); }
  void observe(uint32_t x) { out.clear(); in.push_back(x); if ((int)in.size() == p2::RATE) duplex(); }
  void observe_n(const uint32_t* x, size_t n) { for (size_t i = 0; i < n; i++) observe(x[i]); }
  uint32_t sample() { if (!in.empty() || out.empty()) duplex(); const uint32_t v = out.back(); out.pop_back(); return v; }
  E4 sample_ext() { E4 e; for (int i = 0; i < 4; i++) e.c[i] = sample(); return e; }
  uint32_t sample_bits(int b) { return sample() & ((1u << b) - 1); }
  bool check_pow(uint32_t nonce, int pow_bits) { if (!in.empty()) duplex(); out.clear(); observe(nonce); return (sample() & ((1u << pow_bits) - 1)) == 0; }
};

// E4 helpers on MONTGOMERY values
inline E4 m_base(uint32_t xm) { return E4{{xm, 0, 0, 0}}; }
inline E4 m_pow(E4 a, uint64_t e) { E4 r = bb::e_one_m(); while (e) { if (e & 1) r = bb::e_mul_m(r, a); a = bb::e_mul_m(a, a); e >>= 1; } return r; }
inline bool e_eq(const E4& a, const E4& b) { return !memcmp(a.c, b.c, 16); }

struct VerifierOps {                                                       // air::eval on the openings at zeta (E4, Montgomery): plain arithmetic, nothing lazy
  using V = E4;
  using AccP = E4;
  using AccL = E4;
  const E4* l; const E4* n; const E4* al; const E4* an; const uint32_t* lk_m; const E4* ap; E4 acc; int deferred;   // deferred: the MODE (0, 1, 2)
  E4 is_first, is_last, is_trans;
  V aloc(int k) const { return al[k]; }
  V anxt(int k) const { return an[k]; }
  V par(int i) const { return m_base(lk_m[i]); }
  V add(const V& a, const V& b) const { return bb::e_add(a, b); }
  V sub(const V& a, const V& b) const { return bb::e_sub(a, b); }
  V mul(const V& a, const V& b) const { return bb::e_mul_m(a, b); }
  V mulc(const V& a, uint32_t cm) const { return bb::e_mul_fm(a, cm); }
  V cst(uint32_t cm) const { return m_base(cm); }
  V lsub(const V& a, const V& b) const { return bb::e_sub(a, b); }
  V ladd(const V& a, const V& b) const { return bb::e_add(a, b); }
  V lmul(const V& a, const V& b) const { return bb::e_mul_m(a, b); }
  AccP accp() const { return bb::e_zero(); }
  void acc_mul(AccP& a, const V& x, const V& y) const { a = bb::e_add(a, bb::e_mul_m(x, y)); }
  V acc_val(const AccP& a) const { return a; }
  AccL accl() const { return bb::e_zero(); }
  void acc_lin(AccL& a, const V& x, uint32_t k) const { a = bb::e_add(a, bb::e_mul_fm(x, bb::to_mont(k))); }
  V accl_val(const AccL& a) const { return a; }
  // logical column k of the AIR: the constant 0 if it is not committed (air.h: is_virtual), else the opening of its committed position
  V loc(int k) const { return air::is_virtual(k, deferred) ? bb::e_zero() : l[air::phys_col(k, deferred)]; }
  V nxt(int k) const { return air::is_virtual(k, deferred) ? bb::e_zero() : n[air::phys_col(k, deferred)]; }
  V loc_r(int k) const { return loc(k); }
  V nxt_r(int k) const { return nxt(k); }
  void end_boundary() {}
  void end_trans() {}
  void push(int idx, const V& v) { acc = bb::e_add(acc, bb::e_mul_m(ap[idx], v)); }
  void push_t(int idx, const V& v) { push(idx, bb::e_mul_m(v, is_trans)); }
  void push_fc(int idx, const V& v, uint32_t cm) { push(idx, bb::e_mul_m(bb::e_sub(v, m_base(cm)), is_first)); }
  void push_lc(int idx, const V& v, uint32_t cm) { push(idx, bb::e_mul_m(bb::e_sub(v, m_base(cm)), is_last)); }
  void push_fc0(int idx, uint32_t cm) { push_fc(idx, bb::e_zero(), cm); }
  void push_lc0(int idx, uint32_t cm) { push_lc(idx, bb::e_zero(), cm); }
};

// binary fold of one pair, Montgomery: (a + b)/2 + beta (a - b) / (2x)
inline E4 fold_pair(const E4& a, const E4& b, uint32_t x_m, const E4& beta) {
  const uint32_t half_m = bb::to_mont((bb::P + 1) / 2), two_m = bb::to_mont(2);
  uint32_t inv = bb::R1, base = bb::mont_mul(two_m, x_m), e = bb::P - 2;
  while (e) { if (e & 1) inv = bb::mont_mul(inv, base); base = bb::mont_mul(base, base); e >>= 1; }
  return bb::e_add(bb::e_mul_fm(bb::e_add(a, b), half_m), bb::e_mul_m(beta, bb::e_mul_fm(bb::e_sub(a, b), inv)));
}

// ---- the FRI verifier core: what verify_impl (a STARK proof: b = 1) and fri_part_verify / host_query_run (the commitment layer's proofs: any b) share.  Each caller keeps
//      its own order of checks and its own codes: the oracle and the Python specifications fix them. ----

// The final layer (fri_final_size(b) Montgomery values) has degree < 4: coefficients 4 .. n_fin - 1 of its interpolant vanish.  A plain inverse DFT decides: the coset shift
// scales coefficient k by shift^-k and cannot make a non-zero one vanish.
bool fri_final_degree_ok(const std::vector<E4>& fin, int b) {
  const size_t n_fin = fin.size();
  const uint32_t winv_m = bb::to_mont(bb::inv(bb::root_of_unity(2 + b)));
  for (size_t k = 4; k < n_fin; k++) {
    E4 c = bb::e_zero();
    uint32_t tw = bb::R1, step = bb::R1;
    for (size_t t = 0; t < k; t++) step = bb::mont_mul(step, winv_m);       // w^-k
    for (size_t i = 0; i < n_fin; i++) { c = bb::e_add(c, bb::e_mul_fm(fin[i], tw)); tw = bb::mont_mul(tw, step); }
    if (c.c[0] | c.c[1] | c.c[2] | c.c[3]) return false;
  }
  return true;
}

// The transcript after gamma: per layer root -> beta (Montgomery), the final layer's words, the grinding check.  The caller samples its queries next.
bool fri_transcript(Challenger& ch, const uint32_t* lroots, int n_layers, const uint32_t* fin_words, size_t n_fin, uint32_t nonce, int pow_bits, std::vector<E4>& betas) {
  betas.resize(n_layers);
  for (int j = 0; j < n_layers; j++) { ch.observe_n(lroots + 4 * j, 4); betas[j] = bb::e_to_mont(ch.sample_ext()); }
  ch.observe_n(fin_words, 4 * n_fin);
  return ch.check_pow(nonce, pow_bits);
}

// A query's walk down the layers: where it stands before a layer, and what one layer shows of it
struct FriWalk {
  uint32_t shift; int log_m; E4 carried; size_t carried_idx;
  FriWalk(int log_M, size_t q) : shift(bb::GEN), log_m(log_M), carried(bb::e_zero()), carried_idx(q) {}
};
struct FriLayerSeen {
  E4 v0, v1;          // the leaf's first two values (layer 0: the codeword at q and q + M/2)
  bool leaf_ok;       // the leaf hashes up its path to the layer's root
  bool carried_ok;    // v[slot] is the value carried from the layer before (meaningless at layer 0, which carries nothing)
};
// One layer: `words` are its 4 * 2^k value words and 4 * (log_m - k) path words, all present (the caller has checked the length).  Folds k times with beta, beta^2, ..
// and the squared shift, and carries the result to the next layer.
FriLayerSeen fri_walk_step(FriWalk& s, const uint32_t* words, int k, const uint32_t* root, E4 beta) {
  const int depth = s.log_m - k;
  const size_t nv = (size_t)1 << k, g = (size_t)1 << depth, idx = s.carried_idx & (g - 1), slot = s.carried_idx >> depth;
  std::vector<E4> v(nv);
  for (size_t t = 0; t < nv; t++) v[t] = bb::e_to_mont(E4{{words[4 * t], words[4 * t + 1], words[4 * t + 2], words[4 * t + 3]}});
  uint32_t dg[4]; hash_elems(words, 4 * nv, dg);
  const FriLayerSeen seen{v[0], v[1], check_path(dg, idx, words + 4 * nv, depth, root), e_eq(v[slot], s.carried)};
  for (int f = 0; f < k; f++) {
    const size_t half = nv >> (f + 1);
    const uint32_t wm = bb::root_of_unity(s.log_m);
    for (size_t t = 0; t < half; t++) v[t] = fold_pair(v[t], v[t + half], bb::to_mont(bb::mul(s.shift, bb::pow(wm, idx + t * g))), beta);
    s.shift = bb::mul(s.shift, s.shift); s.log_m--; beta = bb::e_mul_m(beta, beta);
  }
  s.carried = v[0]; s.carried_idx = idx;
  return seen;
}

// the VM's initial state at `entry` (VMState::new, state.rs:55-71) as a state vector: cycle 0, pc limbs, zero registers, Normalized
void initial_state(uint64_t entry, uint32_t st[NS]) {
  memset(st, 0, NS * sizeof(uint32_t));
  st[1] = (uint32_t)(entry & 0xFFFFF); st[2] = (uint32_t)((entry >> 20) & 0xFFFFF); st[3] = (uint32_t)(entry >> 40);
}

// A proof at the context's own rate ('ZKSR', zkir_prove_rate): the sections of a zkir_prove proof through the quotient root under its own header, then ONE embedded 'ZKBE'
// evaluation proof in place of the openings, the FRI part and the queries.  verify_impl's front (header, program, I/O section, table side, challenges up to zeta) is the
// same code for both formats — modes 3 and 4 included: the touched cells, the tapes, their digests and the table side all lie before zeta; `rate` != NULL selects the
// header's checks and, after zeta, the tail (rate_tail below).
constexpr uint32_t RATE_MAGIC = 0x52534B5Au, RATE_VERSION = 1, BATCH_EVAL_MAGIC = 0x45424B5Au;      // 'ZKSR'; 'ZKBE'
struct RateCheck { uint32_t min_queries, min_pow_bits; const zkir::QueryStage* stage; };
int verify_impl(const uint32_t* w, uint64_t len, const zkir_public_inputs* expect, bool whole_run, uint32_t* states_out, uint32_t* counters_out = nullptr,
                const zkir::TapeStages* stages = nullptr, zkir::StarkQueries* defer = nullptr, const RateCheck* rate = nullptr, const zkir::MemStages* mem = nullptr);
int host_stark_run(void*, const zkir::StarkQueries* list, uint32_t n, int* codes);
int host_stark_queries_of(const zkir::StarkQueries& Q, uint32_t first);
inline int header_words_of(int mode) { return HEADER_WORDS + (mode >= 2 ? 4 : 0); }     // modes 2 / 3: + (oc, ic) of the first row, of the last row
// (mode 3) the bytes of cell `addr` (a multiple of 8) in the VM's INITIAL memory: the code words at 0x1000, the data section right behind them (vm.rs:153-170), zero elsewhere
uint64_t image_cell(const uint8_t* blob, size_t n, uint64_t addr) {
  if (!blob || n < 32) return 0;
  uint32_t code_size, data_size; memcpy(&code_size, blob + 16, 4); memcpy(&data_size, blob + 20, 4);
  if (32 + (uint64_t)code_size + data_size > n) return 0;
  uint64_t v = 0;
  for (int k = 0; k < 8; k++) { const uint64_t a = addr + k; if (a >= 0x1000 && a - 0x1000 < (uint64_t)code_size + data_size) v |= (uint64_t)blob[32 + (a - 0x1000)] << (8 * k); }
  return v;
}

// (mode 2) the I/O section of a proof, after the program: [n_in] [inputs: four 16-bit pieces each] [n_out] [outputs] [halt kind] [halt code: four pieces]
struct IoSection { std::vector<uint64_t> in, out; uint32_t halt_kind = ZKIR_HALT_CYCLE_LIMIT; uint64_t halt_code = 0; size_t words = 0; };
bool parse_io_section(const uint32_t* w, size_t avail, IoSection& io) {
  size_t p = 0;
  auto u64 = [&](uint64_t& v) { if (p + 4 > avail) return false; v = 0; for (int i = 0; i < 4; i++) { if (w[p + i] > 0xFFFF) return false; v |= (uint64_t)w[p + i] << (16 * i); } p += 4; return true; };
  for (int tape = 0; tape < 2; tape++) {
    if (p >= avail) return false;
    const size_t n = w[p++];
    if (n > ((size_t)1 << 28) || p + 4 * n > avail) return false;
    std::vector<uint64_t>& t = tape ? io.out : io.in;
    t.resize(n);
    for (size_t k = 0; k < n; k++) if (!u64(t[k])) return false;
  }
  if (p >= avail) return false;
  io.halt_kind = w[p++];
  if (io.halt_kind > 2 || !u64(io.halt_code)) return false;
  io.words = p;
  return true;
}
bool io_digest_matches(const uint32_t* digest4, const IoSection& io, uint64_t cycles) {
  std::vector<uint64_t> b;
  b.push_back(io.in.size()); b.insert(b.end(), io.in.begin(), io.in.end()); b.push_back(io.out.size()); b.insert(b.end(), io.out.begin(), io.out.end());
  b.push_back(io.halt_kind); b.push_back(io.halt_kind == ZKIR_HALT_EXIT ? io.halt_code : 0); b.push_back(cycles);
  uint32_t dg[4];
  zkir_digest_bytes((const uint8_t*)b.data(), b.size() * 8, dg);
  return !memcmp(dg, digest4, 16);
}
int halt_binding(const uint32_t* w, const uint32_t* last_state, int halt_kind, uint64_t halt_code);
bool last_row_writes(const uint32_t* w, const uint32_t* last_state, int halt_kind, uint64_t* value);

// Host wall time of a verification's phases: [0] parsing (the record checks of the tapes among it), [1] the sections' chunk digests, [2] the hash tape's share of the table
// side, [3] the wide tape's, [4] the rest.  Kept per thread for zkir_verify_last_stages; printed on stderr when ZKIR_VERIFY_TIMES is set (nothing by default).
struct LastStages { double ms[5] = {0, 0, 0, 0, 0}; uint32_t device_stages = 0; bool valid = false; };
thread_local LastStages last_stages;
struct LastQueries { uint64_t hash_jobs = 0, value_jobs = 0, uploaded_words = 0; uint32_t launches = 0; };      // zkir_verify_queries_last: the device query stage of the thread's last verification
thread_local LastQueries last_queries;
struct LastMemory { uint64_t cells = 0, uploaded_words = 0; uint32_t launches = 0; };      // zkir_verify_memory_last: the device memory stages of the thread's last verification
thread_local LastMemory last_memory;
struct LastTapes { uint64_t records = 0, uploaded_words = 0; uint32_t launches = 0; };      // zkir_verify_tapes_last: the tape list stage of the thread's last many-proof verification
thread_local LastTapes last_tapes;
struct StageClock {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  double ms[5] = {0, 0, 0, 0, 0};
  void lap(int k) { const auto now = std::chrono::steady_clock::now(); ms[k] += std::chrono::duration<double, std::milli>(now - t).count(); t = now; }
  ~StageClock() {
    lap(4);
    for (int k = 0; k < 5; k++) last_stages.ms[k] = ms[k];
    last_stages.device_stages = 0; last_stages.valid = true;
    last_queries = LastQueries{};                                            // (every host verification: the *_on_device entries note theirs once the stage has run)
    last_memory = LastMemory{};                                              // (likewise: zkir_verify_memory_device notes its own afterwards)
    last_tapes = LastTapes{};                                                // (likewise: the *_many_tapes_* entries)
    if (getenv("ZKIR_VERIFY_TIMES"))
      fprintf(stderr, "zkir_verify: parse %.3f ms | section digests %.3f | hash table side %.3f | wide table side %.3f | rest %.3f\n", ms[0], ms[1], ms[2], ms[3], ms[4]);
  }
};

// ---- the host forms of the tape stages (verify_stages.h) ----------------------------------------------------------------------------------------------------------------
E4 lk_e4(const uint32_t* lk_m, int at) { E4 e; memcpy(e.c, lk_m + at, 16); return e; }
int host_hash_check(void* self, const uint32_t* w, size_t avail, uint64_t n_real, uint64_t code_end, size_t* used) {
  return hashcall::parse_section(w, avail, n_real, code_end, static_cast<zkir::HostTapes*>(self)->hcalls, used);
}
int host_wide_check(void* self, const uint32_t* sec, size_t n_wide, uint64_t n_real) {
  zkir::HostTapes& h = *static_cast<zkir::HostTapes*>(self);
  h.wide = sec; h.n_wide = n_wide;
  for (size_t k = 0; k < n_wide; k++) {
    const uint32_t* c = sec + 1 + 8 * k;
    if (c[1] >= (1u << 20) || c[2] >= (1u << 20) || c[3] >= (1u << 24) || c[4] >= (1u << 20) || c[5] >= (1u << 20) || c[6] >= (1u << 24) || c[7] < 3 || c[7] > 7) return 57;
    if (c[0] >= n_real || (k && c[0] <= c[-8]) || (c[7] >= 4 && !(c[4] | c[5] | c[6]))) return 57;
  }
  return 0;
}
// The chunks are independent: long sections (a 2^22-cycle hash chain's tape is 34 M words = 4 M permutations) are hashed on several host threads.
void section_digests_host(const uint32_t* sw, size_t sl, uint32_t* dg) {
  const size_t n_chunks = (sl + 511) / 512;
  hashcall::for_calls(n_chunks, hashcall::parts_for(n_chunks / 8), [&](unsigned, size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; k++) hash_elems(sw + 512 * k, sl - 512 * k < 512 ? sl - 512 * k : 512, dg + 4 * k);
  });
}
int host_digests(void*, int, const uint32_t* sw, size_t sl, uint32_t* dg) { section_digests_host(sw, sl, dg); return 0; }
// The digest inside the new bytes is computed HERE (hashcall::new_bytes).
int host_hash_side(void* self, const uint32_t* lk_m, uint32_t T[4]) {
  const std::vector<hashcall::Call>& hcalls = static_cast<zkir::HostTapes*>(self)->hcalls;
  E4 T_hash = bb::e_zero();
  if (!hcalls.empty()) {
    const E4 alpha_l = lk_e4(lk_m, air::LK_ALPHA);
    E4 lam[air::N_TUPLE + 1];
    for (int j = 0; j <= air::N_TUPLE; j++) lam[j] = lk_e4(lk_m, air::LK_LAM + 4 * j);
    auto mem_d = [&](uint64_t addr, uint32_t t, uint64_t bytes) {
      E4 fp = bb::e_mul_fm(lam[air::N_TUPLE], bb::to_mont((uint32_t)air::TAG_MEM));
      fp.c[0] = bb::add(fp.c[0], bb::to_mont((uint32_t)(addr & 0xFFFFF)));
      fp = bb::e_add(fp, bb::e_mul_fm(lam[1], bb::to_mont((uint32_t)((addr >> 20) & 0xFFFFF))));
      fp = bb::e_add(fp, bb::e_mul_fm(lam[2], bb::to_mont(t)));
      for (int k = 0; k < 8; k++) fp = bb::e_add(fp, bb::e_mul_fm(lam[3 + k], bb::to_mont((uint32_t)((bytes >> (8 * k)) & 0xFF))));
      return bb::e_sub(alpha_l, fp);
    };
    const unsigned parts = hashcall::parts_for(hcalls.size());
    std::vector<E4> Tpart(parts, bb::e_zero());
    hashcall::for_calls(hcalls.size(), parts, [&](unsigned part, size_t lo, size_t hi) {      // (host threads; each part inverts its own batch)
      std::vector<E4> hd; std::vector<int8_t> hsign; std::vector<uint64_t> nb;
      for (size_t ci = lo; ci < hi; ci++) {
        const hashcall::Call& c = hcalls[ci];
        const uint32_t e[11] = {(uint32_t)(c.cycle % bb::P), (uint32_t)(c.in_ptr & 0xFFFFF), (uint32_t)((c.in_ptr >> 20) & 0xFFFFF), (uint32_t)(c.in_ptr >> 40), (uint32_t)(c.len & 0xFFFFF),
                                (uint32_t)((c.len >> 20) & 0xFFFFF), (uint32_t)(c.len >> 40), (uint32_t)(c.out_ptr & 0xFFFFF), (uint32_t)((c.out_ptr >> 20) & 0xFFFFF), (uint32_t)(c.out_ptr >> 40), c.kind};
        E4 fp = bb::e_mul_fm(lam[air::N_TUPLE], bb::to_mont((uint32_t)air::TAG_HASH));
        for (int j = 0; j < 11; j++) fp = bb::e_add(fp, bb::e_mul_fm(lam[j], bb::to_mont(e[j])));
        hd.push_back(bb::e_sub(alpha_l, fp)); hsign.push_back(1);
        hashcall::new_bytes(c, nb);
        for (size_t k = 0; k < c.cells.size(); k++) {
          hd.push_back(mem_d(c.cells[k].addr, c.cells[k].t, c.cells[k].bytes)); hsign.push_back(-1);
          hd.push_back(mem_d(c.cells[k].addr, (uint32_t)((c.cycle + 1) % bb::P), nb[k])); hsign.push_back(1);
        }
      }
      std::vector<E4> hpre(hd.size());
      E4 hacc = bb::e_one_m();
      for (size_t i = 0; i < hd.size(); i++) { hpre[i] = hacc; hacc = bb::e_mul_m(hacc, hd[i]); }
      E4 hinv = bb::e_inv_m(hacc), Tp = bb::e_zero();
      for (size_t i = hd.size(); i-- > 0;) {
        const E4 di = bb::e_mul_m(hinv, hpre[i]);
        hinv = bb::e_mul_m(hinv, hd[i]);
        Tp = hsign[i] > 0 ? bb::e_add(Tp, di) : bb::e_sub(Tp, di);
      }
      Tpart[part] = Tp;
    });
    for (const E4& tp : Tpart) T_hash = bb::e_add(T_hash, tp);
  }
  memcpy(T, T_hash.c, 16);
  return 0;
}
// The result is computed HERE (air::wide_result).
int host_wide_side(void* self, const uint32_t* lk_m, uint32_t T[4]) {
  const zkir::HostTapes& h = *static_cast<zkir::HostTapes*>(self);
  const uint32_t* wide_words = h.wide; const size_t n_wide = h.n_wide;
  E4 T_wide = bb::e_zero();
  if (n_wide) {
    const E4 alpha_l = lk_e4(lk_m, air::LK_ALPHA);
    E4 lam[air::N_TUPLE + 1];
    for (int j = 0; j <= air::N_TUPLE; j++) lam[j] = lk_e4(lk_m, air::LK_LAM + 4 * j);
    const unsigned parts = hashcall::parts_for(n_wide / 4);
    std::vector<E4> Tpart(parts, bb::e_zero());
    hashcall::for_calls(n_wide, parts, [&](unsigned part, size_t lo, size_t hi) {             // (host threads; each part inverts its own batch)
      std::vector<E4> wd(hi - lo), wpre(hi - lo);
      for (size_t k = lo; k < hi; k++) {
        const uint32_t* r = wide_words + 1 + 8 * k;
        const uint64_t a = (uint64_t)r[1] | ((uint64_t)r[2] << 20) | ((uint64_t)r[3] << 40), b = (uint64_t)r[4] | ((uint64_t)r[5] << 20) | ((uint64_t)r[6] << 40);
        const uint64_t y = air::wide_result(r[7], a, b);
        const uint32_t e[11] = {r[0] % bb::P, r[1], r[2], r[3], r[4], r[5], r[6], (uint32_t)(y & 0xFFFFF), (uint32_t)((y >> 20) & 0xFFFFF), (uint32_t)(y >> 40), r[7]};
        E4 fp = bb::e_mul_fm(lam[air::N_TUPLE], bb::to_mont((uint32_t)air::TAG_WIDE));
        for (int j = 0; j < 11; j++) fp = bb::e_add(fp, bb::e_mul_fm(lam[j], bb::to_mont(e[j])));
        wd[k - lo] = bb::e_sub(alpha_l, fp);
      }
      E4 wacc = bb::e_one_m(), Tp = bb::e_zero();
      for (size_t k = 0; k < wd.size(); k++) { wpre[k] = wacc; wacc = bb::e_mul_m(wacc, wd[k]); }
      E4 winv = bb::e_inv_m(wacc);
      for (size_t k = wd.size(); k-- > 0;) { Tp = bb::e_add(Tp, bb::e_mul_m(winv, wpre[k])); winv = bb::e_mul_m(winv, wd[k]); }
      Tpart[part] = Tp;
    });
    for (const E4& tp : Tpart) T_wide = bb::e_add(T_wide, tp);
  }
  memcpy(T, T_wide.c, 16);
  return 0;
}

// ---- the host forms of the memory stages (verify_stages.h): what a device stage leaves small sections to, and zkir_mem_section_check_host / zkir_mem_table_side_host ----
int host_mem_check(void* self, const uint32_t* sec, size_t avail, int mode, uint64_t code_words, size_t* used) {
  if (avail < 1) return 4;
  const size_t nc = sec[0];
  if (nc > ((size_t)1 << 28) || (avail - 1) / 7 < nc) return 4;
  for (size_t k = 0; k < nc; k++) {
    const uint32_t* c = sec + 1 + 7 * k;
    const int code = air::mem_cell_code(c, k ? c - 7 : nullptr, mode, code_words);
    if (code) return code;
  }
  if (self) { zkir::HostMem& h = *static_cast<zkir::HostMem*>(self); h.sec = sec; h.n = nc; }
  *used = 1 + 7 * nc;
  return 0;
}
int host_mem_digests(void*, const uint32_t* sec, size_t len, uint32_t* dg) { section_digests_host(sec, len, dg); return 0; }
// sec: a CHECKED section of n cells.  Host threads; each part inverts its own batch of 2 (hi - lo) denominators.
void mem_side_sum(const uint32_t* sec, size_t n, const uint8_t* blob, size_t blob_len, const uint32_t* lk_m, uint32_t T[4]) {
  E4 T_mem = bb::e_zero();
  if (n) {
    const E4 alpha_l = lk_e4(lk_m, air::LK_ALPHA);
    E4 lam[air::N_TUPLE + 1];
    for (int j = 0; j <= air::N_TUPLE; j++) lam[j] = lk_e4(lk_m, air::LK_LAM + 4 * j);
    auto mem_d = [&](const uint32_t* c, uint32_t t, uint64_t bytes) {
      E4 fp = bb::e_mul_fm(lam[air::N_TUPLE], bb::to_mont((uint32_t)air::TAG_MEM));
      fp.c[0] = bb::add(fp.c[0], bb::to_mont(c[0]));
      fp = bb::e_add(fp, bb::e_mul_fm(lam[1], bb::to_mont(c[1])));
      fp = bb::e_add(fp, bb::e_mul_fm(lam[2], bb::to_mont(t)));
      for (int k = 0; k < 8; k++) fp = bb::e_add(fp, bb::e_mul_fm(lam[3 + k], bb::to_mont((uint32_t)((bytes >> (8 * k)) & 0xFF))));
      return bb::e_sub(alpha_l, fp);
    };
    const unsigned parts = hashcall::parts_for(n / 4);
    std::vector<E4> Tpart(parts, bb::e_zero());
    hashcall::for_calls(n, parts, [&](unsigned part, size_t lo, size_t hi) {
      std::vector<E4> d(2 * (hi - lo)), pre(2 * (hi - lo));
      for (size_t k = lo; k < hi; k++) {
        const uint32_t* c = sec + 1 + 7 * k;
        const uint64_t addr = (uint64_t)c[0] | ((uint64_t)c[1] << 20), fin = (uint64_t)c[3] | ((uint64_t)c[4] << 16) | ((uint64_t)c[5] << 32) | ((uint64_t)c[6] << 48);
        d[2 * (k - lo)] = mem_d(c, 0, image_cell(blob, blob_len, addr));
        d[2 * (k - lo) + 1] = mem_d(c, c[2], fin);
      }
      E4 acc = bb::e_one_m(), Tp = bb::e_zero();
      for (size_t i = 0; i < d.size(); i++) { pre[i] = acc; acc = bb::e_mul_m(acc, d[i]); }
      E4 inv = bb::e_inv_m(acc);
      for (size_t i = d.size(); i-- > 0;) {
        const E4 di = bb::e_mul_m(inv, pre[i]);
        inv = bb::e_mul_m(inv, d[i]);
        Tp = (i & 1) ? bb::e_sub(Tp, di) : bb::e_add(Tp, di);               // + initial tuple, - final tuple
      }
      Tpart[part] = Tp;
    });
    for (const E4& tp : Tpart) T_mem = bb::e_add(T_mem, tp);
  }
  memcpy(T, T_mem.c, 16);
}
int host_mem_side(void* self, const uint32_t* lk_m, const uint8_t* blob, size_t blob_len, uint32_t T[4]) {
  const zkir::HostMem& h = *static_cast<zkir::HostMem*>(self);
  mem_side_sum(h.sec, h.n, blob, blob_len, lk_m, T);
  return 0;
}

}  // namespace

namespace zkir {
TapeStages host_tape_stages(HostTapes* h) { return TapeStages{h, host_hash_check, host_wide_check, host_digests, host_hash_side, host_wide_side}; }
int verify_with_stages(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, const TapeStages& stages) {
  return verify_impl(proof, proof_words, expect, true, nullptr, nullptr, &stages);
}
MemStages host_mem_stages(HostMem* h) { return MemStages{h, host_mem_check, host_mem_digests, host_mem_side}; }
uint64_t mem_image_cell(const uint8_t* blob, size_t blob_len, uint64_t addr) { return image_cell(blob, blob_len, addr); }
const uint8_t* mem_image_of(const uint8_t* blob, size_t blob_len, uint64_t* image_len) {      // (image_cell's rule)
  *image_len = 0;
  if (!blob || blob_len < 32) return nullptr;
  uint32_t code_size, data_size; memcpy(&code_size, blob + 16, 4); memcpy(&data_size, blob + 20, 4);
  if (32 + (uint64_t)code_size + data_size > blob_len) return nullptr;
  *image_len = (uint64_t)code_size + data_size;
  return blob + 32;
}
uint64_t stark_proof_blob_bytes(const uint32_t* proof, uint64_t proof_words) {
  if (!proof || proof_words < 10 || proof[9] > 4) return 0;
  const uint64_t at = (uint64_t)header_words_of((int)proof[9]);
  if (proof_words <= at) return 0;
  return std::min<uint64_t>(proof[at], 2 * (proof_words - at - 1));
}
void section_chunk_digests(const uint32_t* sw, size_t sl, uint32_t* dg) { section_digests_host(sw, sl, dg); }
const char* mem_side_args(const uint32_t* sec, uint64_t n_words, const uint8_t* blob, size_t blob_len, const uint32_t alpha[4], const uint32_t lambda[4], const uint32_t* sum,
                          uint32_t* lk, uint64_t* n) {
  if (!sec || !alpha || !lambda || !sum || (!blob && blob_len)) return "null argument";
  if (n_words < 1 || sec[0] > (1u << 28) || n_words != 1 + 7 * (uint64_t)sec[0]) return "the section must be [n] + 7 n words";
  for (int k = 0; k < 4; k++) if (alpha[k] >= bb::P || lambda[k] >= bb::P) return "alpha and lambda must be canonical";
  *n = sec[0];
  for (int k = 0; k < air::N_LK; k++) lk[k] = 0;
  E4 a, l1, lam = bb::e_one_m();
  memcpy(a.c, alpha, 16); memcpy(l1.c, lambda, 16);
  a = bb::e_to_mont(a); l1 = bb::e_to_mont(l1);
  memcpy(lk + air::LK_ALPHA, a.c, 16);
  for (int j = 0; j <= air::N_TUPLE; j++) { memcpy(lk + air::LK_LAM + 4 * j, lam.c, 16); lam = bb::e_mul_m(lam, l1); }
  return nullptr;
}
void verify_note_memory(uint64_t cells, uint32_t launches, uint64_t uploaded_words) { last_memory = LastMemory{cells, uploaded_words, launches}; }
void verify_note_tapes(uint64_t records, uint32_t launches, uint64_t uploaded_words) { last_tapes = LastTapes{records, uploaded_words, launches}; }
void verify_note_device_stages(uint32_t n) { last_stages.device_stages = n; }
void verify_note_queries(uint64_t hash_jobs, uint64_t value_jobs, uint32_t launches, uint64_t uploaded_words) { last_queries = LastQueries{hash_jobs, value_jobs, uploaded_words, launches}; }
StarkQueryStage host_stark_query_stage() { return StarkQueryStage{nullptr, host_stark_run}; }
int stark_host_queries_from(const StarkQueries& q, uint32_t first) { return first >= q.num_queries ? 0 : host_stark_queries_of(q, first); }
int stark_verify_collect(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, bool whole_run, const TapeStages* stages, StarkQueries* out,
                         const MemStages* mem) {
  return verify_impl(proof, proof_words, expect, whole_run, nullptr, nullptr, stages, out, nullptr, mem);
}
}  // namespace zkir

extern "C" {

// Static check of the quotient kernel's lazy arithmetic on the constraint list (air::BoundOps): 0 = sound; else 1 and the broken rule in `why`.
int zkir_air_check_bounds(uint32_t deferred, char* why, size_t why_len) {
  const char* w = air::check_bounds((int)deferred);                 // `deferred` = the mode: 0, 1 or 2
  if (why && why_len) snprintf(why, why_len, "%s", w ? w : "");
  return w ? 1 : 0;
}

void zkir_digest_bytes(const uint8_t* b, size_t n, uint32_t out[4]) {
  std::vector<uint32_t> e;
  e.reserve(4 + (n + 1) / 2);
  for (int i = 0; i < 4; i++) e.push_back((uint32_t)(((uint64_t)n >> (16 * i)) & 0xFFFF));
  for (size_t i = 0; i < n; i += 2) e.push_back((uint32_t)b[i] | (i + 1 < n ? (uint32_t)b[i + 1] << 8 : 0u));
  hash_elems(e.data(), e.size(), out);
}

int zkir_public_inputs_of(const zkir_delta_log* log, const uint8_t* blob, size_t blob_len, const uint64_t* inputs, size_t n_inputs, uint32_t deferred,
                          zkir_public_inputs* out) {
  if (!log || !out || (!blob && blob_len) || (!inputs && n_inputs)) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_public_inputs_of: null argument"}); return ZKIR_ERR_ARGUMENT; }
  // cycles / outputs / halt reason must be those of the FINISHED run: the whole log, any shard of it, or the trace window of the
  // rank that executed the run to its end (multi-GPU: the last rank) — not a window that stopped before the halt
  if (log->window_open) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_public_inputs_of: this trace window ended before the run did (its outputs / halt reason are not the run's)"}); return ZKIR_ERR_ARGUMENT; }
  memset(out, 0, sizeof *out);
  out->n_real = log->cycles;
  out->deferred = deferred > 4 ? 1 : deferred;                             // the proof's mode: 0 default, 1 deferred model, 2 default + the I/O argument, 3 = 2 + the memory argument (zkir_memcheck_witness_of)
  // the claim in the clear (mode 2 proofs carry it; BORROWED: the caller's inputs, the log's outputs)
  out->inputs = inputs; out->n_inputs = n_inputs;
  out->outputs = log->outputs.data(); out->n_outputs = log->outputs.size();
  out->halt_kind = (uint32_t)log->halt_kind; out->halt_code = log->halt_kind == ZKIR_HALT_EXIT ? log->halt_code : 0;
  out->writes_before = out->reads_before = 0;                              // a whole run; the caller of a SEGMENT proof sets them
  uint32_t entry = 0x1000;
  if (blob_len >= 16) memcpy(&entry, blob + 12, 4);                        // ProgramHeader.entry_point, program.rs:189-213
  out->entry_point = entry;
  zkir_digest_bytes(blob, blob_len, out->program_digest);
  out->program_blob = blob; out->program_blob_len = blob_len;              // borrowed: the prover reads the instruction ROM from it
  if (log->cycle_base == 0 && log->n_rows == log->cycles) { out->hash_outs = log->hash_outs.size() ? log->hash_outs.data() : nullptr; out->n_hash_outs = log->hash_outs.size(); }   // (a whole traced run: the device witness of mode 4 reads what its hash calls wrote)
  std::vector<uint64_t> io;
  io.push_back(n_inputs); io.insert(io.end(), inputs, inputs + n_inputs);
  io.push_back(log->outputs.size()); io.insert(io.end(), log->outputs.begin(), log->outputs.end());
  io.push_back((uint64_t)log->halt_kind); io.push_back(log->halt_kind == ZKIR_HALT_EXIT ? log->halt_code : 0); io.push_back(log->cycles);
  zkir_digest_bytes((const uint8_t*)io.data(), io.size() * 8, out->io_digest);
  return ZKIR_OK;
}

uint64_t zkir_public_inputs_size(void) { return sizeof(zkir_public_inputs); }
uint64_t zkir_hash_call_cells_host(uint64_t in_ptr, uint64_t len, uint64_t out_ptr, uint32_t kind, uint64_t cell, uint64_t* rank) {
  if (rank) *rank = ~0ull;
  if (!hashcall::in_range(in_ptr, len, out_ptr, kind)) return ~0ull;
  if (rank) *rank = hashcall::rank_of(in_ptr, len, out_ptr, cell);
  return hashcall::n_cells_of(in_ptr, len, out_ptr);
}

int zkir_verify(const uint32_t* w, uint64_t len, const zkir_public_inputs* expect) { return verify_impl(w, len, expect, true, nullptr); }
// zkir_merkle_verify_launch's verdicts on the host: hash_elems over the record's row (or its leaf digest as it stands), check_path over its siblings
int zkir_merkle_verify_host(const uint32_t root[4], uint32_t width, uint64_t n_leaves, const uint64_t* indices, uint64_t n_idx, const uint32_t* openings, uint32_t flags, uint32_t* verdicts,
                            uint32_t summary[2]) {
  if (!root || !verdicts || (n_idx && (!indices || !openings))) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_merkle_verify_host: null root, indices, openings or verdicts"}); return ZKIR_ERR_ARGUMENT; }
  if (n_leaves == 0 || (n_leaves & (n_leaves - 1))) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_merkle_verify_host: n_leaves must be a power of two"}); return ZKIR_ERR_ARGUMENT; }
  const bool digest_form = flags & ZKIR_OPEN_LEAF_DIGEST;
  if (digest_form && width != 0) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_merkle_verify_host: the digest form has width 0"}); return ZKIR_ERR_ARGUMENT; }
  int depth = 0;
  while (((uint64_t)1 << depth) < n_leaves) depth++;
  const size_t lead = digest_form ? 4 : width, rec = lead + 4 * (size_t)depth;
  uint32_t failed = 0, first = 0xFFFFFFFFu;
  for (uint64_t i = 0; i < n_idx; i++) {
    const uint32_t* r = openings + i * rec;
    uint32_t v = 0;
    if (indices[i] >= n_leaves) v = 3;
    else {
      for (size_t k = 0; k < rec && !v; k++) if (r[k] >= bb::P) v = 2;
      if (!v) {
        uint32_t dg[4];
        if (digest_form) memcpy(dg, r, 16); else hash_elems(r, width, dg);
        if (!check_path(dg, (size_t)indices[i], r + lead, depth, root)) v = 1;
      }
    }
    verdicts[i] = v;
    if (v) { failed++; if (first == 0xFFFFFFFFu) first = (uint32_t)i; }
  }
  if (summary) { summary[0] = failed; summary[1] = first; }
  return ZKIR_OK;
}
int zkir_verify_queries_last(uint64_t* hash_jobs, uint64_t* value_jobs, uint32_t* launches, uint64_t* uploaded_words) {
  if (hash_jobs) *hash_jobs = last_queries.hash_jobs;
  if (value_jobs) *value_jobs = last_queries.value_jobs;
  if (launches) *launches = last_queries.launches;
  if (uploaded_words) *uploaded_words = last_queries.uploaded_words;
  return ZKIR_OK;
}
int zkir_verify_last_stages(double ms[5], uint32_t* device_stages) {
  if (!last_stages.valid) return ZKIR_ERR_ARGUMENT;
  if (ms) for (int k = 0; k < 5; k++) ms[k] = last_stages.ms[k];
  if (device_stages) *device_stages = last_stages.device_stages;
  return ZKIR_OK;
}
int zkir_verify_memory_last(uint64_t* cells, uint32_t* launches, uint64_t* uploaded_words) {
  if (cells) *cells = last_memory.cells;
  if (launches) *launches = last_memory.launches;
  if (uploaded_words) *uploaded_words = last_memory.uploaded_words;
  return ZKIR_OK;
}
int zkir_verify_tapes_last(uint64_t* records, uint32_t* launches, uint64_t* uploaded_words) {
  if (records) *records = last_tapes.records;
  if (launches) *launches = last_tapes.launches;
  if (uploaded_words) *uploaded_words = last_tapes.uploaded_words;
  return ZKIR_OK;
}
int zkir_mem_section_check_host(const uint32_t* sec, uint64_t n_words, uint32_t mode, uint64_t code_words, int32_t* verdict) {
  if (!verdict || (!sec && n_words)) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_mem_section_check_host: null argument"}); return ZKIR_ERR_ARGUMENT; }
  size_t used = 0;
  *verdict = host_mem_check(nullptr, sec, (size_t)n_words, (int)mode, code_words, &used);
  return ZKIR_OK;
}
int zkir_mem_table_side_host(const uint32_t* sec, uint64_t n_words, const uint8_t* blob, size_t blob_len, const uint32_t alpha[4], const uint32_t lambda[4], uint32_t sum[4]) {
  uint32_t lk[air::N_LK];
  uint64_t n = 0;
  size_t used = 0;
  const char* why = zkir::mem_side_args(sec, n_words, blob, blob_len, alpha, lambda, sum, lk, &n);
  if (!why && host_mem_check(nullptr, sec, (size_t)n_words, 3, 0, &used)) why = "the section's cells are not in range and strictly increasing";
  if (why) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, std::string("zkir_mem_table_side_host: ") + why}); return ZKIR_ERR_ARGUMENT; }
  try {
    uint32_t T[4];
    mem_side_sum(sec, (size_t)n, blob, blob_len, lk, T);
    E4 t; memcpy(t.c, T, 16);
    t = bb::e_from_mont(t);
    memcpy(sum, t.c, 16);
  } catch (const std::exception& e) { zkir::set_last_error({ZKIR_ERR_OTHER, std::string("zkir_mem_table_side_host: ") + e.what()}); return ZKIR_ERR_OTHER; }
  return ZKIR_OK;
}

// ---- (mode 3) the memory witness: a sequential replay of the run's loads and stores over 8-byte cells (see include/zkir_amd.h) ----
}  // extern "C"
struct zkir_memcheck_witness {
  std::vector<uint64_t> old; std::vector<uint32_t> told;                   // per row
  std::vector<uint64_t> cell_addr, cell_bytes; std::vector<uint32_t> cell_time;
  uint64_t n_accesses = 0;
  std::vector<uint32_t> hash_words; uint64_t n_hash = 0;                   // (mode 4) the hash calls as the proof's hash section (hashcall.h)
};
extern "C" {
int zkir_memcheck_witness_of(const zkir_delta_log* log, const uint8_t* blob, size_t blob_len, zkir_memcheck_witness** out) { return zkir_memcheck_witness_of_mode(log, blob, blob_len, 3, out); }
uint64_t zkir_memcheck_witness_n_hash_calls(const zkir_memcheck_witness* w) { return w ? w->n_hash : 0; }
int zkir_memcheck_witness_of_mode(const zkir_delta_log* log, const uint8_t* blob, size_t blob_len, uint32_t mode, zkir_memcheck_witness** out) {
  if (out) *out = nullptr;
  auto refuse = [](const std::string& m) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_memcheck_witness_of: " + m}); return ZKIR_ERR_ARGUMENT; };
  if (!log || !out || !blob) return refuse("null argument");
  if (log->cycle_base != 0 || log->window_open || log->n_rows != log->cycles) return refuse("the memory argument spans a whole run: not a shard, a window or an untraced log");
  const uint64_t n = log->n_rows;
  if (n >= (1ull << 30)) return refuse("more than 2^30 rows");
  auto* w = new zkir_memcheck_witness;
  w->old.assign(n, 0); w->told.assign(n, 0);
  // cell -> (bytes, time): open addressing over the touched cells (a run touches far fewer cells than it has rows)
  struct Slot { uint64_t addr, bytes; uint32_t t; uint32_t used; };
  size_t cap = 1024; std::vector<Slot> tab(cap, Slot{0, 0, 0, 0}); size_t used = 0;
  auto find = [&](uint64_t addr) -> Slot& {
    if (2 * (used + 1) > cap) {
      std::vector<Slot> nt(cap * 2, Slot{0, 0, 0, 0});
      for (const Slot& s : tab) if (s.used) { size_t h = (size_t)((s.addr >> 3) * 0x9E3779B97F4A7C15ull >> 20) & (cap * 2 - 1); while (nt[h].used) h = (h + 1) & (cap * 2 - 1); nt[h] = s; }
      tab.swap(nt); cap *= 2;
    }
    size_t h = (size_t)((addr >> 3) * 0x9E3779B97F4A7C15ull >> 20) & (cap - 1);
    while (tab[h].used && tab[h].addr != addr) h = (h + 1) & (cap - 1);
    if (!tab[h].used) { tab[h] = Slot{addr, image_cell(blob, blob_len, addr), 0, 1}; used++; }
    return tab[h];
  };
  uint64_t reg[16] = {0};
  std::vector<hashcall::Call> hcalls;
  const zkir_reg_event* ev = log->reg_events.data(); const size_t n_ev = log->reg_events.size(); size_t e = 0;
  const uint32_t* inst = log->inst.data();
  for (uint64_t i = 0; i < n; i++) {
    while (e < n_ev && ev[e].vis <= i) { reg[ev[e].reg] = ev[e].value; e++; }        // the pre-state of row i
    if (i + 1 >= n) break;                                                            // the halt row executes nothing the AIR describes
    const uint32_t word = inst[i], op = word & 0x7F;
    if (op == air::OP_ECALL) {
      if (reg[10] < 3 || reg[10] > 6) continue;
      if (mode != 4) { delete w; return refuse("the run executes a hash syscall (row " + std::to_string(i) + "): its memory effect is not stated by the AIR"); }
      // (mode 4) a hash call: its record for the tape, its effect on the replayed memory (the message is read out of the OLD bytes; every touched cell gets the call's time)
      hashcall::Call hc{i, reg[11], reg[12], reg[13], (uint32_t)reg[10], {}};
      if (!hashcall::in_range(hc.in_ptr, hc.len, hc.out_ptr, hc.kind)) { delete w; return refuse("the hash syscall at row " + std::to_string(i) + " is outside what a proof states (kind 3 / 5 / 6, at most 1 MiB of input, buffers below 2^40, a SHA-256 output at a multiple of 4)"); }
      std::vector<uint64_t> addrs, nbv;
      hashcall::cells_of(hc.in_ptr, hc.len, hc.out_ptr, addrs);
      for (const uint64_t a : addrs) { const Slot& c = find(a); hc.cells.push_back(hashcall::Cell{a, c.bytes, c.t}); }
      hashcall::new_bytes(hc, nbv);
      for (size_t k = 0; k < addrs.size(); k++) { Slot& c = find(addrs[k]); c.bytes = nbv[k]; c.t = (uint32_t)(i + 1); }
      hcalls.push_back(std::move(hc));
      continue;
    }
    if (!air::is_load(op) && !air::is_store(op)) continue;
    const uint32_t fa = (word >> 7) & 0xF, fb = (word >> 11) & 0xF;
    const int64_t imm = (int64_t)(int32_t)(word & 0xFFFF8000u) >> 15;                 // imm17, sign-extended
    const uint64_t ea = reg[air::is_load(op) ? fb : fa] + (uint64_t)imm;              // wrapping u64 add (execute.rs:477-575)
    if (ea >> 40) { delete w; return refuse("address " + std::to_string(ea) + " at row " + std::to_string(i) + " is not below 2^40"); }
    const int width = air::mem_width(op), off = (int)(ea & 7);
    Slot& c = find(ea - off);
    w->old[i] = c.bytes; w->told[i] = c.t; w->n_accesses++;
    if (air::is_store(op)) {
      const uint64_t mask = width == 8 ? ~0ull : ((1ull << (8 * width)) - 1);
      c.bytes = (c.bytes & ~(mask << (8 * off))) | ((reg[fb] & mask) << (8 * off));
    }
    c.t = (uint32_t)(i + 1);
  }
  std::vector<const Slot*> order;
  for (const Slot& s : tab) if (s.used) order.push_back(&s);
  std::sort(order.begin(), order.end(), [](const Slot* a, const Slot* b) { return a->addr < b->addr; });
  for (const Slot* s : order) { w->cell_addr.push_back(s->addr); w->cell_bytes.push_back(s->bytes); w->cell_time.push_back(s->t); }
  if (mode == 4) { hashcall::put_section(hcalls, w->hash_words); w->n_hash = hcalls.size(); }
  *out = w;
  return ZKIR_OK;
}
void zkir_memcheck_witness_free(zkir_memcheck_witness* w) { delete w; }
uint64_t zkir_memcheck_witness_n_cells(const zkir_memcheck_witness* w) { return w ? w->cell_addr.size() : 0; }
uint64_t zkir_memcheck_witness_n_accesses(const zkir_memcheck_witness* w) { return w ? w->n_accesses : 0; }
int zkir_public_inputs_set_params(zkir_public_inputs* pub, const zkir_prover_params* params) {
  if (!pub || !params) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_public_inputs_set_params: null argument"}); return ZKIR_ERR_ARGUMENT; }
  const uint32_t fp = (params->num_queries & 0xFFFF) | (params->pow_bits << 16);
  if (params->mode != pub->deferred || params->num_queries > 0xFFFF || params->pow_bits > 0xFFFF || !air::fri_params_ok(fp)) {
    zkir::set_last_error({ZKIR_ERR_ARGUMENT, "zkir_prover_params: mode must be the public inputs' (zkir_public_inputs_of's `deferred`: 0 default, 1 deferred model, 2 + I/O argument, 3 + memory "
                                             "argument), num_queries 0 (= 50) or 50..128, pow_bits 0 (= 12) or 12..24"});
    return ZKIR_ERR_ARGUMENT;
  }
  pub->fri_params = fp;
  return ZKIR_OK;
}

void zkir_public_inputs_set_memory(zkir_public_inputs* pub, const zkir_memcheck_witness* w) {
  if (!pub || !w) return;
  if (pub->deferred < 3) pub->deferred = 3;                               // (a mode-4 proof keeps its mode: the witness is the same)
  pub->mem_old = w->old.data(); pub->mem_told = w->told.data();
  pub->cell_addr = w->cell_addr.data(); pub->cell_bytes = w->cell_bytes.data(); pub->cell_time = w->cell_time.data(); pub->n_cells = w->cell_addr.size();
  pub->hash_section = w->hash_words.empty() ? nullptr : w->hash_words.data(); pub->hash_section_words = w->hash_words.size();
}

int zkir_verify_segment(const uint32_t* w, uint64_t len, const zkir_public_inputs* expect, uint32_t first_state[68], uint32_t last_state[68]) {
  uint32_t st[2 * NS];
  const int rc = verify_impl(w, len, expect, false, st);
  if (rc == 0) { if (first_state) memcpy(first_state, st, NS * 4); if (last_state) memcpy(last_state, st + NS, NS * 4); }
  return rc;
}

uint32_t zkir_proof_state_words(void) { return NS; }

int zkir_verify_chain(const uint32_t* const* proofs, const uint64_t* lens, uint32_t n, const zkir_public_inputs* expect) {
  if (proofs && lens && n == 1 && proofs[0] && lens[0] > 9 && proofs[0][9] >= 3) return verify_impl(proofs[0], lens[0], expect, true, nullptr, nullptr);   // a mode-3 proof is a whole run by itself (never a segment): a "chain" of one
  return zkir::verify_chain_with_stage(proofs, lens, n, expect, zkir::host_stark_query_stage());
}
}  // extern "C"

// The segments' host parts run first, segment after segment up to the first one that fails there; then ONE run of the stage over the collected segments' queries; then
// the verdict in the order the sequential verifier returns it: per segment its host code, its query code, check 30, check 43 — then the linking checks.
namespace {
// What zkir_verify_chain and zkir_verify_rate_chain share once every segment is accepted on its own: checks 41, 42, `expect` (43 / 44) and the mode-2 argument across the
// segments.  st: per segment first | last state; cnt: per segment the four counter words; total: sum (n_i - 1) + 1.  rate: 'ZKSR' segments — expect->fri_params is not
// consulted (the segments' own parameters are compared with segment 0's by the caller).
int chain_link_checks(const uint32_t* const* proofs, const uint64_t* lens, uint32_t n, const zkir_public_inputs* expect, const std::vector<uint32_t>& st, const std::vector<uint32_t>& cnt,
                      uint64_t total, bool rate) {
  const uint32_t* w0 = proofs[0];
  const uint64_t entry = (uint64_t)w0[10] | ((uint64_t)w0[11] << 20) | ((uint64_t)w0[12] << 40);
  uint32_t init[NS];
  initial_state(entry, init);
  if (memcmp(init, &st[0], sizeof init)) return 41;
  for (uint32_t i = 1; i < n; i++)
    if (memcmp(&st[(size_t)i * 2 * NS], &st[(size_t)(i - 1) * 2 * NS + NS], NS * 4)) return 42;
  if (expect) {
    if (expect->deferred != w0[9] || expect->entry_point != entry || memcmp(expect->program_digest, w0 + 13, 16) || memcmp(expect->io_digest, w0 + 17, 16)) return 43;
    if (!rate)
      for (uint32_t i = 0; i < n; i++)                                      // every segment made with the parameters the caller expects
        if (!air::fri_params_ok(expect->fri_params) || proofs[i][4] != (uint32_t)air::num_queries_of(expect->fri_params) || proofs[i][6] != (uint32_t)air::pow_bits_of(expect->fri_params)) return 43;
    if (expect->n_real != total) return 44;
  }
  if (w0[9] == 2) {
    // (mode 2) the I/O argument across segments: the same tapes in every segment (45), counters from (0, 0) linking up (46) to "every output written" (51),
    // tapes + halt reason + TOTAL cycle count hash to the io digest (50), the last segment ends on the instruction the halt reason names (52 / 53)
    const size_t HW = (size_t)header_words_of(2);
    auto io_at = [&](const uint32_t* w) { return HW + 1 + ((size_t)w[HW] + 1) / 2; };
    IoSection io0;
    if (!parse_io_section(w0 + io_at(w0), (size_t)lens[0] - io_at(w0), io0)) return 4;
    for (uint32_t i = 1; i < n; i++) { const uint32_t* w = proofs[i]; if (io_at(w) != io_at(w0) || io_at(w) + io0.words > (size_t)lens[i] || memcmp(w + io_at(w), w0 + io_at(w0), io0.words * 4)) return 45; }
    if (cnt[0] || cnt[1]) return 51;
    for (uint32_t i = 1; i < n; i++) if (cnt[(size_t)i * 4] != cnt[(size_t)(i - 1) * 4 + 2] || cnt[(size_t)i * 4 + 1] != cnt[(size_t)(i - 1) * 4 + 3]) return 46;
    {
      uint64_t tail_value = 0;
      const bool tail = last_row_writes(proofs[n - 1], proofs[n - 1] + 21 + NS, (int)io0.halt_kind, &tail_value);            // (see verify_impl: the last row of a run cut by its cycle limit)
      if (cnt[(size_t)(n - 1) * 4 + 2] + (tail ? 1 : 0) != io0.out.size() || (tail && io0.out.back() != tail_value)) return 51;
    }
    if (!io_digest_matches(w0 + 17, io0, total)) return 50;
    const int hb = halt_binding(proofs[n - 1], proofs[n - 1] + 21 + NS, (int)io0.halt_kind, io0.halt_code);
    if (hb) return hb;
  }
  return 0;
}
}  // namespace

int zkir::verify_chain_with_stage(const uint32_t* const* proofs, const uint64_t* lens, uint32_t n, const zkir_public_inputs* expect, const zkir::StarkQueryStage& stage) {
  if (!proofs || !lens || n < 1) return 40;
  std::vector<uint32_t> st((size_t)n * 2 * NS), cnt((size_t)n * 4, 0);
  uint64_t total = 1;
  std::vector<zkir::StarkQueries> Q(n);
  uint32_t n_ok = 0; int host_rc = 0;
  for (; n_ok < n; n_ok++) {
    host_rc = verify_impl(proofs[n_ok], lens[n_ok], nullptr, false, &st[(size_t)n_ok * 2 * NS], &cnt[(size_t)n_ok * 4], nullptr, &Q[n_ok]);
    if (host_rc) break;
  }
  std::vector<int> codes(n_ok ? n_ok : 1, 0);
  if (n_ok) { const int src = stage.run(stage.self, Q.data(), n_ok, codes.data()); if (src) return src; }
  for (uint32_t i = 0; i < n_ok; i++) {
    const int rc = codes[i] ? codes[i] : zkir::stark_length_check(Q[i]);
    if (rc) return 1000 * (int)(i + 1) + rc;
    const uint32_t* w = proofs[i];
    total += ((uint64_t)w[7] | ((uint64_t)w[8] << 30)) - 1;
    if (memcmp(w + 9, proofs[0] + 9, 12 * 4)) return 43;                   // mode, entry point, program digest, io digest
  }
  if (n_ok < n) return 1000 * (int)(n_ok + 1) + host_rc;
  return chain_link_checks(proofs, lens, n, expect, st, cnt, total, false);
}

// The same for 'ZKSR' segments (zkir_verify_rate_chain): the fronts run with a collecting stage (verify_stages.h) up to the first segment that fails there, ONE run of the
// list stage serves the collected embedded proofs, and the verdict is the sequential verifier's: per segment its code (100 + c for the embedded proof's query code c), then
// check 43 — here also the rate and the parameters (header words 4, 5, 6) against segment 0's — then the linking checks.
int zkir::rate_chain_with_stage(const uint32_t* const* proofs, const uint64_t* lens, uint32_t n, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits,
                                const zkir::PcsManyStage& stage) {
  if (!proofs || !lens || n < 1) return 40;
  std::vector<uint32_t> st((size_t)n * 2 * NS), cnt((size_t)n * 4, 0);
  uint64_t total = 1;
  std::vector<zkir::PcsCollected> Q(n);
  uint32_t n_ok = 0; int host_rc = 0;
  for (; n_ok < n; n_ok++) {
    host_rc = zkir::rate_segment_verify_with_stage(proofs[n_ok], lens[n_ok], nullptr, min_queries, min_pow_bits, zkir::pcs_collect_stage(&Q[n_ok]), &st[(size_t)n_ok * 2 * NS], &cnt[(size_t)n_ok * 4]);
    if (host_rc) break;
  }
  std::vector<int> codes(n_ok ? n_ok : 1, 0);
  if (n_ok) { const int src = stage.run(stage.self, Q.data(), n_ok, codes.data()); if (src) return src; }
  for (uint32_t i = 0; i < n_ok; i++) {
    if (codes[i]) return 1000 * (int)(i + 1) + 100 + codes[i];
    const uint32_t* w = proofs[i];
    total += ((uint64_t)w[7] | ((uint64_t)w[8] << 30)) - 1;
    if (memcmp(w + 9, proofs[0] + 9, 12 * 4) || memcmp(w + 4, proofs[0] + 4, 3 * 4)) return 43;      // mode, entry point, digests; num_queries, log_blowup, pow_bits
  }
  if (n_ok < n) return 1000 * (int)(n_ok + 1) + host_rc;
  return chain_link_checks(proofs, lens, n, expect, st, cnt, total, true);
}

extern "C" {
// ---- what the run CLAIMS (round 4): its I/O tapes and how it ended -------------------------------------------------------------------
// The io digest a proof carries is a hash of (inputs, outputs, halt kind, exit code, cycles) that the AIR does not look inside.  These two calls take
// the claim in the clear and check, on top of zkir_verify / zkir_verify_chain:
//   50  the claim does not hash to the proof's io digest (or its cycle count is not the proof's row count);
//   52  the HALT ROW — the last executed row, whose state the AIR pins to the public last state — is not the instruction the claim names: EBREAK for an
//       Ebreak halt, ECALL for an Exit halt (vm.rs:302-347, syscall.rs:101-107), looked up in the program the proof carries at the last state's pc; a
//       CycleLimit halt (vm.rs:211-214) names no instruction: the claim is "this many cycles were executed";
//   53  an Exit halt whose ECALL does not read R10 = 0 (SYSCALL_EXIT) and R11 = the claimed exit code in that state.
// So a prover can no longer end a run at an arbitrary instruction and call it an exit.  The OUTPUTS stay unproven: they are bound into the
// transcript, not derived from the trace (air.h: "Not constrained").
namespace {
int halt_binding(const uint32_t* w, const uint32_t* last_state, int halt_kind, uint64_t halt_code) {
  if (halt_kind == ZKIR_HALT_CYCLE_LIMIT) return 0;
  if (halt_kind != ZKIR_HALT_EBREAK && halt_kind != ZKIR_HALT_EXIT) return 52;
  const int HW = header_words_of((int)w[9]);
  const uint64_t blob_len = w[HW];
  std::vector<uint8_t> blob(blob_len);
  for (uint64_t i = 0; i < blob_len; i += 2) { const uint32_t h = w[HW + 1 + i / 2]; blob[i] = (uint8_t)(h & 0xFF); if (i + 1 < blob_len) blob[i + 1] = (uint8_t)(h >> 8); }
  if (blob_len < 32) return 52;
  uint32_t code_size; memcpy(&code_size, blob.data() + 16, 4);
  const uint64_t pc = (uint64_t)last_state[1] | ((uint64_t)last_state[2] << 20) | ((uint64_t)last_state[3] << 40);
  if (pc < 0x1000 || (pc & 3) || pc - 0x1000 >= code_size || 32 + (pc - 0x1000) + 4 > blob_len) return 52;
  uint32_t word; memcpy(&word, blob.data() + 32 + (pc - 0x1000), 4);
  if ((word & 0x7F) != (halt_kind == ZKIR_HALT_EBREAK ? 0x51u : 0x50u)) return 52;                  // opcode.rs:154-228: ECALL 0x50, EBREAK 0x51
  if (halt_kind == ZKIR_HALT_EXIT) {
    auto reg = [&](int r) {                                                                          // raw 64-bit register value from its limbs (30-bit limbs when Accumulated)
      const uint32_t* l = last_state + 4 + 3 * r; const int bits = last_state[52 + r] ? 30 : 20;
      return (uint64_t)l[0] | ((uint64_t)l[1] << bits) | ((uint64_t)l[2] << (2 * bits));
    };
    if (reg(10) != 0 || reg(11) != halt_code) return 53;
  }
  return 0;
}
// the last executed row of a run that stopped at its cycle limit, if it is a WRITE ecall (R10 = 2): the value it writes (R11 of the public last state)
bool last_row_writes(const uint32_t* w, const uint32_t* last, int halt_kind, uint64_t* value) {
  if (halt_kind != ZKIR_HALT_CYCLE_LIMIT) return false;
  const int HW = header_words_of((int)w[9]);
  const uint64_t blob_len = w[HW];
  if (blob_len < 32) return false;
  auto byte = [&](uint64_t i) { const uint32_t h = w[HW + 1 + i / 2]; return (uint32_t)((i & 1) ? (h >> 8) : (h & 0xFF)); };
  const uint32_t code_size = byte(16) | (byte(17) << 8) | (byte(18) << 16) | (byte(19) << 24);
  const uint64_t pc = (uint64_t)last[1] | ((uint64_t)last[2] << 20) | ((uint64_t)last[3] << 40);
  if (pc < 0x1000 || (pc & 3) || pc - 0x1000 >= code_size || 32 + (pc - 0x1000) + 4 > blob_len) return false;
  if ((byte(32 + (pc - 0x1000)) & 0x7F) != 0x50) return false;                                          // opcode.rs:154-228: ECALL
  auto reg = [&](int r) { const uint32_t* l = last + 4 + 3 * r; const int bits = last[52 + r] ? 30 : 20; return (uint64_t)l[0] | ((uint64_t)l[1] << bits) | ((uint64_t)l[2] << (2 * bits)); };
  if (reg(10) != 2) return false;
  *value = reg(11);
  return true;
}
bool io_claim_matches(const uint32_t* w, uint64_t cycles, const uint64_t* inputs, size_t n_in, const uint64_t* outputs, size_t n_out, int halt_kind, uint64_t halt_code) {
  std::vector<uint64_t> io;
  io.push_back(n_in); io.insert(io.end(), inputs, inputs + n_in);
  io.push_back(n_out); io.insert(io.end(), outputs, outputs + n_out);
  io.push_back((uint64_t)halt_kind); io.push_back(halt_kind == ZKIR_HALT_EXIT ? halt_code : 0); io.push_back(cycles);
  uint32_t dg[4];
  zkir_digest_bytes((const uint8_t*)io.data(), io.size() * 8, dg);
  return !memcmp(dg, w + 17, 16);
}
}  // namespace

int zkir_verify_io(const uint32_t* w, uint64_t len, const zkir_public_inputs* expect, const uint64_t* inputs, size_t n_in, const uint64_t* outputs, size_t n_out, int halt_kind,
                   uint64_t halt_code) {
  if ((!inputs && n_in) || (!outputs && n_out)) return 50;
  uint32_t st[2 * NS];
  const int rc = verify_impl(w, len, expect, true, st);
  if (rc) return rc;
  const uint64_t n_real = (uint64_t)w[7] | ((uint64_t)w[8] << 30);
  if (!io_claim_matches(w, n_real, inputs, n_in, outputs, n_out, halt_kind, halt_code)) return 50;
  return halt_binding(w, st + NS, halt_kind, halt_code);
}

int zkir_verify_chain_io(const uint32_t* const* proofs, const uint64_t* lens, uint32_t n, const zkir_public_inputs* expect, const uint64_t* inputs, size_t n_in,
                         const uint64_t* outputs, size_t n_out, int halt_kind, uint64_t halt_code) {
  if ((!inputs && n_in) || (!outputs && n_out)) return 50;
  const int rc = zkir_verify_chain(proofs, lens, n, expect);
  if (rc) return rc;
  uint64_t total = 1;
  for (uint32_t i = 0; i < n; i++) total += ((uint64_t)proofs[i][7] | ((uint64_t)proofs[i][8] << 30)) - 1;
  if (!io_claim_matches(proofs[0], total, inputs, n_in, outputs, n_out, halt_kind, halt_code)) return 50;
  return halt_binding(proofs[n - 1], proofs[n - 1] + 21 + NS, halt_kind, halt_code);                // the last segment's last state (header words 21 + NS ..)
}

}  // extern "C"

namespace {

// sum_c alpha^c C_c(zeta) == Q(zeta) Z_H(zeta) on openings or evaluations (main | aux at zeta: tz, the same at zeta w: tzw, the quotient's four: qzs; Montgomery E4) — check 10
// of verify_impl, and of a list entry that deferred it (zkir::mem_deferred_check).  lk_m: air.h LK_*, complete; first / last / cnt: canonical words.
bool constraints_at_zeta(const E4* tz, const E4* tzw, const E4* qzs, const uint32_t* lk_m, const E4& alpha, const E4& zeta, int log_n, uint64_t n_real, int mode, int WM,
                         const uint32_t* first, const uint32_t* last, const uint32_t* cnt) {
  const size_t N = (size_t)1 << log_n;
  const uint32_t wn = bb::root_of_unity(log_n);
  std::vector<E4> ap(air::N_CONSTRAINTS);                                  // (modes 0 / 1 use the first N_CONSTRAINTS_BASE)
  ap[0] = bb::e_one_m();
  for (int c = 1; c < air::N_CONSTRAINTS; c++) ap[c] = bb::e_mul_m(ap[c - 1], alpha);
  E4 zh = m_pow(zeta, N); zh.c[0] = bb::sub(zh.c[0], bb::R1);
  E4 d1 = zeta; d1.c[0] = bb::sub(d1.c[0], bb::R1);
  E4 dl = zeta; dl.c[0] = bb::sub(dl.c[0], bb::to_mont(bb::pow(wn, n_real - 1)));
  const E4 is_first = bb::e_mul_m(zh, bb::e_inv_m(d1)), is_last = bb::e_mul_m(zh, bb::e_inv_m(dl));
  E4 is_trans = zeta; is_trans.c[0] = bb::sub(is_trans.c[0], bb::to_mont(bb::inv(wn)));
  uint32_t first_m[NS], last_m[NS];
  for (int i = 0; i < NS; i++) { first_m[i] = bb::to_mont(first[i]); last_m[i] = bb::to_mont(last[i]); }
  uint32_t cnt_m[4];
  for (int k = 0; k < 4; k++) cnt_m[k] = bb::to_mont(cnt[k]);
  VerifierOps o{tz, tzw, tz + WM, tzw + WM, lk_m, ap.data(), bb::e_zero(), mode, is_first, is_last, is_trans};
  air::eval(o, first_m, last_m, mode, cnt_m);
  E4 qz = bb::e_zero();                                                    // Q(zeta) = sum_i X^i q_i(zeta): basis element X^i times the E4 opening
  for (int i = 0; i < 4; i++) { E4 basis = bb::e_zero(); basis.c[i] = bb::R1; qz = bb::e_add(qz, bb::e_mul_m(basis, qzs[i])); }
  return e_eq(o.acc, bb::e_mul_m(qz, zh));
}

int verify_impl(const uint32_t* w, uint64_t len, const zkir_public_inputs* expect, bool whole_run, uint32_t* states_out, uint32_t* counters_out, const zkir::TapeStages* stages,
                zkir::StarkQueries* defer, const RateCheck* rate, const zkir::MemStages* mem) {
  StageClock clk;                                                         // (diagnostics: the host wall time of the call's phases, kept for zkir_verify_last_stages)
  zkir::HostTapes host_tapes;
  const zkir::TapeStages host_stages = zkir::host_tape_stages(&host_tapes);
  const zkir::TapeStages& S = stages ? *stages : host_stages;
  if (!w) return 1;
  size_t p = 0;
  auto need = [&](size_t k) { return p + k <= len; };
  if (!need(HEADER_WORDS) || w[0] != (rate ? RATE_MAGIC : PROOF_MAGIC) || w[9] > 4 || w[1] != (rate ? RATE_VERSION : air::proof_version((int)w[9]))) return 1;
  const int log_n = (int)w[2];
  if (w[9] > 4) return 2;
  const int mode = (int)w[9];                                              // 0 default, 1 deferred, 2 default + the I/O argument, 3 = 2 + the memory argument
  if (mode >= 3 && !whole_run) return 2;                                   // the memory check spans the whole run: a mode-3 proof is never a segment
  const int HW = header_words_of(mode), WA = air::aux_width(mode);
  if (!need(HW)) return 1;
  const int WM = (int)w[3], WT = WM + WA;                                  // committed main-trace columns (checked against the mode below); main + aux
  // the prover's parameters (header words 4 and 6): exactly what `expect` names (0 = the defaults) when there is one; otherwise anything from the defaults up
  // ('ZKSR': the evaluation proof's ranges, 1 .. 128 queries and 0 .. 24 bits, at least what the caller asks for; word 5 is log_blowup; `expect->fri_params` is not consulted)
  if (w[4] > (uint32_t)air::MAX_NUM_QUERIES || w[6] > (uint32_t)air::MAX_POW_BITS) return 2;
  const int NUM_QUERIES = (int)w[4], POW_BITS = (int)w[6];
  if (rate) { if (w[4] < 1 || w[5] < 1 || w[5] > 3 || w[2] + w[5] > 27 || w[4] < rate->min_queries || w[6] < rate->min_pow_bits) return 2; }
  else if (expect ? (!air::fri_params_ok(expect->fri_params) || NUM_QUERIES != air::num_queries_of(expect->fri_params) || POW_BITS != air::pow_bits_of(expect->fri_params))
             : (NUM_QUERIES < air::DEFAULT_NUM_QUERIES || POW_BITS < air::DEFAULT_POW_BITS)) return 2;
  if (w[3] != (uint32_t)air::committed_width(mode) || (!rate && w[5] != (uint32_t)LOG_FINAL) || w[2] < (uint32_t)LOG_FINAL || w[2] > 26) return 2;
  if (w[7] >= (1u << 30) || w[10] >= (1u << 20) || w[11] >= (1u << 20) || w[12] >= (1u << 24)) return 2;
  zkir_public_inputs pub;
  memset(&pub, 0, sizeof pub);
  pub.n_real = (uint64_t)w[7] | ((uint64_t)w[8] << 30); pub.deferred = w[9];
  pub.entry_point = (uint64_t)w[10] | ((uint64_t)w[11] << 20) | ((uint64_t)w[12] << 40);
  memcpy(pub.program_digest, w + 13, 16); memcpy(pub.io_digest, w + 17, 16);
  const uint32_t* first = w + 21; const uint32_t* last = w + 21 + NS;       // boundary states: pinned to rows 0 and n_real - 1 by the AIR
  for (int i = 0; i < 2 * NS; i++) if (first[i] >= bb::P) return 3;
  if (pub.n_real == 0 || zkir_padded_log_n(pub.n_real) != (uint32_t)log_n) return 2;
  uint32_t cnt[4] = {0, 0, 0, 0};                                          // (mode 2) (oc, ic) of the first row, of the last row
  if (mode >= 2) { for (int k = 0; k < 4; k++) { if (w[HEADER_WORDS + k] >= bb::P) return 3; cnt[k] = w[HEADER_WORDS + k]; } }
  if (counters_out) memcpy(counters_out, cnt, sizeof cnt);
  if (expect && (expect->n_real != pub.n_real || expect->deferred != pub.deferred || expect->entry_point != pub.entry_point ||
                 memcmp(expect->program_digest, pub.program_digest, 16) || memcmp(expect->io_digest, pub.io_digest, 16))) return 6;
  if (whole_run) { uint32_t init[NS]; initial_state(pub.entry_point, init); if (memcmp(init, first, sizeof init)) return 7; }   // a run starts in the VM's initial state
  if (states_out) memcpy(states_out, first, 2 * NS * 4);
  p = (size_t)HW;
  const size_t N = (size_t)1 << log_n;
  for (size_t i = 2; i < len; i++) if (w[i] >= bb::P) return 3;
  // ---- the program carried in the proof: [byte length][16-bit halfwords]; it must be the program the header names (check 8) ----
  if (!need(1)) return 4;
  const size_t blob_len = w[p++];
  if (blob_len > ((size_t)1 << 30) || !need((blob_len + 1) / 2)) return 4;
  std::vector<uint8_t> blob(blob_len);
  for (size_t i = 0; i < blob_len; i += 2) {
    const uint32_t h = w[p + i / 2];
    if (h > 0xFFFF || (i + 1 >= blob_len && h > 0xFF)) return 8;
    blob[i] = (uint8_t)(h & 0xFF); if (i + 1 < blob_len) blob[i + 1] = (uint8_t)(h >> 8);
  }
  p += (blob_len + 1) / 2;
  { uint32_t dg[4]; zkir_digest_bytes(blob.data(), blob_len, dg); if (memcmp(dg, pub.program_digest, 16)) return 8; }
  auto le32 = [&](size_t at) { return (uint32_t)blob[at] | ((uint32_t)blob[at + 1] << 8) | ((uint32_t)blob[at + 2] << 16) | ((uint32_t)blob[at + 3] << 24); };
  if (blob_len < 32) return 8;
  const uint64_t code_size = le32(16);
  if (code_size % 4 || 32 + code_size > blob_len || le32(12) != pub.entry_point) return 8;
  const size_t n_code = (size_t)(code_size / 4);
  // (mode 2) the tapes and the halt reason the io digest is a digest of: the digest with the cycle count (50; a whole run's is its row count, a chain checks the total),
  // the counters' ends (51), the halt row named by the halt reason (52 / 53)
  IoSection io;
  const uint32_t* io_words = w + p;
  if (mode >= 2) {
    if (!parse_io_section(w + p, (size_t)len - p, io)) return 4;
    p += io.words;
    if (cnt[0] > cnt[2] || cnt[1] > cnt[3] || cnt[2] > io.out.size() || cnt[3] > io.in.size()) return 51;
    if (whole_run) {
      if (!io_digest_matches(pub.io_digest, io, pub.n_real)) return 50;
      // A run that stops at its CYCLE LIMIT has executed its last row too (vm.rs:211-214, :302-347: cycles == rows) while the counters describe what happened BEFORE a row: if
      // that row is a WRITE ecall, the last output is the R11 of the public last state and is not counted yet
      uint64_t tail_value = 0;
      const bool tail = last_row_writes(w, last, (int)io.halt_kind, &tail_value);
      if (cnt[0] || cnt[1] || cnt[2] + (tail ? 1 : 0) != io.out.size() || (tail && io.out.back() != tail_value)) return 51;
      const int hb = halt_binding(w, last, (int)io.halt_kind, io.halt_code);
      if (hb) return hb;
    }
  }
  // (mode 3) the touched cells: [n] then per cell [address limb 0 (20 bits, a multiple of 8)] [limb 1 (20 bits)] [time of the last access] [final bytes: four 16-bit pieces],
  // canonical and by strictly increasing address — every cell has ONE initial tuple (check 54)
  struct Cell { uint64_t addr, bytes; uint32_t t; };
  std::vector<Cell> cells;
  const uint32_t* mem_words = nullptr; size_t mem_len = 0;
  if (mode >= 3 && mem) {                                                  // (a memory stage: its verdict on the section — 4, 54 or 55, as below)
    size_t used = 0;
    const int mrc = mem->check(mem->self, w + p, (size_t)(len - p), mode, n_code, &used);
    if (mrc) return mrc;
    mem_words = w + p; mem_len = used;
    p += mem_len;
  } else if (mode >= 3) {
    if (!need(1)) return 4;
    const size_t nc = w[p];
    if (nc > ((size_t)1 << 28) || !need(1 + 7 * nc)) return 4;
    mem_words = w + p; mem_len = 1 + 7 * nc;
    cells.resize(nc);
    for (size_t k = 0; k < nc; k++) {
      const uint32_t* c = w + p + 1 + 7 * k;
      // limb ranges, byte pieces and strictly increasing addresses (54), then (v11, check 55) no access to the CODE: instruction fetch is tied to the program's words, so a
      // store into [0x1000, 0x1000 + code_size) would change what the VM executes next (vm.rs:175) but not what the AIR lets through — every accessed cell is in this list (the
      // memory check does not balance otherwise), and none may overlap the code
      // (mode 4) .. except the BOUNDARY cell (code_size % 8 == 4: the last code word and the first four data bytes): the AIR states there that no store writes its low half
      const int ccode = air::mem_cell_code(c, k ? c - 7 : nullptr, mode, (uint64_t)n_code);
      if (ccode) return ccode;
      cells[k] = Cell{(uint64_t)c[0] | ((uint64_t)c[1] << 20), (uint64_t)c[3] | ((uint64_t)c[4] << 16) | ((uint64_t)c[5] << 32) | ((uint64_t)c[6] << 48), c[2]};
    }
    p += mem_len;
  }
  // (mode 4) the hash calls: records in increasing cycle order, ranges in the clear, every touched cell's previous access before the call (56); no output on code bytes (55)
  // (the record checks, the sections' chunk digests and their shares of the table side are the three stages behind zkir::TapeStages: verify_stages.h)
  const uint32_t* hash_words = nullptr; size_t hash_len = 0;
  if (mode == 4) {
    hash_words = w + p;
    const int hrc = S.hash_check(S.self, w + p, (size_t)(len - p), pub.n_real, air::CODE_BASE + 4 * (uint64_t)n_code, &hash_len);
    if (hrc) return hrc;
    p += hash_len;
  }
  // (mode 4 d) the wide tape: records in increasing cycle order, limbs in range, an opcode 3..7, no zero divisor (57)
  const uint32_t* wide_words = nullptr; size_t wide_len = 0, n_wide = 0;
  if (mode == 4) {
    if (!need(1)) return 4;
    n_wide = w[p];
    if (n_wide > pub.n_real) return 57;
    if (!need(1 + 8 * n_wide)) return 4;
    wide_words = w + p; wide_len = 1 + 8 * n_wide;
    const int wrc = S.wide_check(S.self, wide_words, n_wide, pub.n_real);
    if (wrc) return wrc;
    p += wide_len;
  }
  if (!need(n_code + air::RC_TABLE + (mode >= 3 ? air::MEM_MULT : 0))) return 4;
  const uint32_t* rom_mult = w + p; p += n_code;
  const uint32_t* rc_mult = w + p; p += air::RC_TABLE;
  const uint32_t* mem_mult = nullptr;
  if (mode >= 3) { mem_mult = w + p; p += air::MEM_MULT; }
  if (!need(12)) return 4;
  const uint32_t* troot = w + p; p += 4; const uint32_t* aroot = w + p; p += 4; const uint32_t* qroot = w + p; p += 4;
  auto get_m = [&](size_t at) { E4 e; memcpy(e.c, w + at, 16); return bb::e_to_mont(e); };      // proof word -> Montgomery E4
  // (zkir_prove's format) the openings at zeta and zeta w, the FRI part's roots, final layer and nonce; a 'ZKSR' proof carries its embedded evaluation proof here (rate_tail)
  size_t at_tz = 0, at_tzw = 0, at_qz = 0, at_fin = 0, n_fin = 0;
  std::vector<E4> t_z, t_zw, q_z, fin;
  int n_layers = 0;
  std::vector<int> ks;
  const uint32_t* lroots = nullptr;
  uint32_t pow_nonce = 0;
  if (!rate) {
    if (!need((size_t)(2 * WT + 4) * 4)) return 4;
    at_tz = p; at_tzw = p + 4 * (size_t)WT; at_qz = p + 8 * (size_t)WT;
    t_z.resize(WT); t_zw.resize(WT); q_z.resize(4);                         // main columns, then aux columns
    for (int k = 0; k < WT; k++) { t_z[k] = get_m(at_tz + 4 * k); t_zw[k] = get_m(at_tzw + 4 * k); }
    for (int i = 0; i < 4; i++) q_z[i] = get_m(at_qz + 4 * i);
    p += (size_t)(2 * WT + 4) * 4;
    if (!need(1)) return 4;
    n_layers = (int)w[p++];
    ks = zkir::fri_schedule(log_n, 1);
    if (n_layers != (int)ks.size()) return 5;
    n_fin = zkir::fri_final_size(1);
    if (!need((size_t)4 * n_layers + 4 * n_fin + 1)) return 4;
    lroots = w + p; p += 4 * (size_t)n_layers;
    at_fin = p;
    fin.resize(n_fin);
    for (size_t i = 0; i < n_fin; i++) { fin[i] = get_m(p); p += 4; }
    pow_nonce = w[p++];
  }
  clk.lap(0);
  // ---- transcript ----
  Challenger ch;
  ch.observe_n(w + 2, (size_t)HW - 2);
  ch.observe_n(troot, 4);
  if (mode >= 2)                                                           // (v11) the tapes and the halt reason, fixed before the lookup challenges (a segment's too) — so::observe_section
    for (size_t at = 0; at < io.words; at += 512) { uint32_t dg[4]; hash_elems(io_words + at, io.words - at < 512 ? io.words - at : 512, dg); ch.observe_n(dg, 4); }
  // the touched cells enter through a two-level sponge: chunks of 512 words hashed on their own, the digests observed (so::observe_section); (mode 4) the hash calls likewise.
  auto observe_section = [&](const uint32_t* sw, size_t sl) {
    std::vector<uint32_t> dg(4 * ((sl + 511) / 512));
    section_digests_host(sw, sl, dg.data());
    ch.observe_n(dg.data(), dg.size());
  };
  clk.lap(4);
  if (mode >= 3 && mem) {
    std::vector<uint32_t> dg(4 * ((mem_len + 511) / 512));
    const int drc = mem->digests(mem->self, mem_words, mem_len, dg.data());
    if (drc) return drc;
    ch.observe_n(dg.data(), dg.size());
  } else if (mode >= 3) observe_section(mem_words, mem_len);
  if (mode == 4) {
    std::vector<uint32_t> dg;
    for (int which = 0; which < 2; which++) {
      const uint32_t* sw = which ? wide_words : hash_words; const size_t sl = which ? wide_len : hash_len;
      dg.resize(4 * ((sl + 511) / 512));
      const int drc = S.digests(S.self, which, sw, sl, dg.data());
      if (drc) return drc;
      ch.observe_n(dg.data(), dg.size());
    }
  }
  clk.lap(1);
  ch.observe_n(rom_mult, n_code);
  ch.observe_n(rc_mult, air::RC_TABLE);
  if (mode >= 3) ch.observe_n(mem_mult, air::MEM_MULT);
  const E4 alpha_l = bb::e_to_mont(ch.sample_ext()), lambda = bb::e_to_mont(ch.sample_ext());
  // lookup parameters (air.h LK_*), Montgomery: alpha, lambda^0..10, T / N — T is the table side of the lookup identity, computed HERE
  // from the program in the proof and the multiplicities: sum_t m_t / (alpha - t) + sum_u r_u / (alpha - fingerprint(ROM row u))
  uint32_t lk_m[air::N_LK];
  zkir::MemDeferred* deferred = nullptr;                                   // (a list entry's memory stage) check 10 waits for the cells' share of the table side
  {
    E4 lam[air::N_TUPLE + 1];
    lam[0] = bb::e_one_m();
    for (int j = 1; j <= air::N_TUPLE; j++) lam[j] = bb::e_mul_m(lam[j - 1], lambda);
    for (int k = 0; k < 4; k++) lk_m[air::LK_ALPHA + k] = alpha_l.c[k];
    for (int j = 0; j <= air::N_TUPLE; j++) for (int k = 0; k < 4; k++) lk_m[air::LK_LAM + 4 * j + k] = lam[j].c[k];
    const size_t n_tab = (size_t)air::RC_TABLE + n_code;
    std::vector<E4> d(n_tab + (mode >= 3 ? (size_t)air::MEM_MULT + 2 * cells.size() : 0));
    E4 T_hash = bb::e_zero();                                              // (mode 4) the hash calls' share, summed by its own threads below
    for (int t = 0; t < air::RC_TABLE; t++) { d[t] = alpha_l; d[t].c[0] = bb::sub(d[t].c[0], bb::to_mont((uint32_t)t)); }
    if (mode >= 3) {
      // the LOW3, BYTE and NIBBLE tables, then the two ends of the memory check: per touched cell the INITIAL tuple (time 0, the program image's bytes) and the FINAL one
      auto tagged = [&](uint32_t v, int tag) { E4 e = bb::e_sub(alpha_l, bb::e_mul_fm(lam[air::N_TUPLE], bb::to_mont((uint32_t)tag))); e.c[0] = bb::sub(e.c[0], bb::to_mont(v)); return e; };
      E4* m = d.data() + n_tab;
      for (int t = 0; t < air::RC_TABLE; t++) m[t] = bb::e_sub(tagged((uint32_t)t, air::TAG_LOW3), bb::e_mul_fm(lam[1], bb::to_mont((uint32_t)(t & 7))));
      for (int t = 0; t < 256; t++) m[air::RC_TABLE + t] = tagged((uint32_t)t, air::TAG_BYTE);
      for (int t = 0; t < 16; t++) m[air::RC_TABLE + 256 + t] = tagged((uint32_t)t, air::TAG_NIB);
      for (int which = 0; which < 3; which++) for (int t = 0; t < 256; t++)      // the bitwise tables (a, b, a op b): a + lambda b + lambda^2 r + (8 + which) lambda^11
        m[air::LG_BASE + 256 * which + t] = bb::e_sub(bb::e_sub(tagged((uint32_t)(t >> 4), air::TAG_AND + which), bb::e_mul_fm(lam[1], bb::to_mont((uint32_t)(t & 15)))),
                                                      bb::e_mul_fm(lam[2], bb::to_mont(air::logic_of(which, (uint32_t)(t >> 4), (uint32_t)(t & 15)))));
      for (int t = 0; t < air::RC_TABLE; t++) m[air::L6_BASE + t] = bb::e_sub(tagged((uint32_t)t, air::TAG_LOW6), bb::e_mul_fm(lam[1], bb::to_mont((uint32_t)(t & 63))));   // LOW6: (v, v & 63)
      auto mem_d = [&](const Cell& c, uint32_t t, uint64_t bytes) {
        E4 fp = bb::e_mul_fm(lam[air::N_TUPLE], bb::to_mont((uint32_t)air::TAG_MEM));
        fp.c[0] = bb::add(fp.c[0], bb::to_mont((uint32_t)(c.addr & 0xFFFFF)));
        fp = bb::e_add(fp, bb::e_mul_fm(lam[1], bb::to_mont((uint32_t)((c.addr >> 20) & 0xFFFFF))));
        fp = bb::e_add(fp, bb::e_mul_fm(lam[2], bb::to_mont(t)));
        for (int k = 0; k < 8; k++) fp = bb::e_add(fp, bb::e_mul_fm(lam[3 + k], bb::to_mont((uint32_t)((bytes >> (8 * k)) & 0xFF))));
        return bb::e_sub(alpha_l, fp);
      };
      for (size_t k = 0; k < cells.size(); k++) { m[air::MEM_MULT + 2 * k] = mem_d(cells[k], 0, image_cell(blob.data(), blob_len, cells[k].addr)); m[air::MEM_MULT + 2 * k + 1] = mem_d(cells[k], cells[k].t, cells[k].bytes); }
      // (mode 4) the hash calls: + 1 / (alpha - fp(call)) per call (its ECALL row looks it up) and the call's memory accesses, which no row states: per touched cell
      // - 1 / (alpha - fp(cell, told, old bytes)) + 1 / (alpha - fp(cell, cycle + 1, new bytes)), the digest inside the new bytes computed by the verifier; (mode 4 d) the
      // wide tape: + 1 / (alpha - fp(cycle, rs1, rs2, what the reference writes, opcode)) per record, the result computed by the verifier
      if (mode == 4) {
        E4 Th = bb::e_zero(), Tw = bb::e_zero();
        clk.lap(4);
        // (a list entry's tape stage) both shares wait with check 10; a memory stage that defers too must defer into the same record
        if (S.defer && S.defer->tapes_armed && !(mem && mem->defer && mem->defer->armed && mem->defer != S.defer)) deferred = S.defer;
        else {
          const int hs = S.hash_side(S.self, lk_m, Th.c);
          clk.lap(2);
          if (hs) return hs;
          const int ws = S.wide_side(S.self, lk_m, Tw.c);
          clk.lap(3);
          if (ws) return ws;
          T_hash = bb::e_add(Th, Tw);
        }
      }
      // (a memory stage) the cells' two ends are the stage's sum: `cells` is empty here, so none of them is in d
      if (mem && mem->defer && mem->defer->armed) deferred = mem->defer;
      else if (mem) {
        E4 Tm = bb::e_zero();
        const int ms = mem->side(mem->self, lk_m, blob.data(), blob_len, Tm.c);
        if (ms) return ms;
        T_hash = bb::e_add(T_hash, Tm);
      }
    }
    for (size_t u = 0; u < n_code; u++) {
      const uint32_t cw = le32(32 + 4 * u);
      const uint64_t pc = 0x1000 + 4 * (uint64_t)u;
      const uint32_t f[air::N_TUPLE] = {(uint32_t)(pc & 0xFFFFF), (uint32_t)((pc >> 20) & 0xFFFFF), (uint32_t)(pc >> 40), cw & 0x7F, (cw >> 7) & 0xF, (cw >> 11) & 0xF,
                                        (cw >> 15) & 0xF, cw >> 19, cw >> 31, air::opclass_of(cw & 0x7F, mode), air::variant_bit(cw & 0x7F, mode)};
      E4 fp = lam[air::N_TUPLE];
      for (int j = 0; j < air::N_TUPLE; j++) fp = bb::e_add(fp, bb::e_mul_fm(lam[j], bb::to_mont(f[j])));
      d[air::RC_TABLE + u] = bb::e_sub(alpha_l, fp);
    }
    // batch inversion (Montgomery's trick): one e_inv_m, three products per element
    std::vector<E4> pre(d.size());
    E4 acc = bb::e_one_m();
    for (size_t i = 0; i < d.size(); i++) { pre[i] = acc; acc = bb::e_mul_m(acc, d[i]); }
    E4 inv = bb::e_inv_m(acc);
    E4 T = bb::e_zero();
    for (size_t i = d.size(); i-- > 0;) {
      const E4 di = bb::e_mul_m(inv, pre[i]);
      inv = bb::e_mul_m(inv, d[i]);
      if (i >= n_tab + (size_t)air::MEM_MULT) { T = ((i - n_tab - (size_t)air::MEM_MULT) & 1) ? bb::e_sub(T, di) : bb::e_add(T, di); continue; }   // (mode 3) + initial tuple, - final tuple
      const uint32_t m = i < (size_t)air::RC_TABLE ? rc_mult[i] : i < n_tab ? rom_mult[i - air::RC_TABLE] : mem_mult[i - n_tab];
      if (m) T = bb::e_add(T, bb::e_mul_fm(di, bb::to_mont(m)));
    }
    T = bb::e_add(T, T_hash);
    lk_m[air::LK_NIN] = 0;
    { const uint64_t Bc = air::boundary_cell(4 * (uint64_t)n_code); lk_m[air::LK_B0] = bb::to_mont((uint32_t)(Bc & 0xFFFFF)); lk_m[air::LK_B1] = bb::to_mont((uint32_t)((Bc >> 20) & 0xFFFFF)); }   // (mode 4) the boundary cell
    if (mode >= 2) {
      // the tapes' share of the table side: every output index in [oc_first, oc_last) and every input index in [ic_first, ic_last) exactly once,
      // fingerprint = index + lambda v0 + lambda^2 v1 + lambda^3 v2 + tag lambda^N_TUPLE (tag 2 = outputs, 3 = inputs), v = the (20, 20, 24)-bit limbs of the value
      lk_m[air::LK_NIN] = bb::to_mont((uint32_t)(io.in.size() % bb::P));
      auto term = [&](uint64_t k, uint64_t v, uint32_t tag) {
        const uint32_t g[4] = {(uint32_t)(k % bb::P), (uint32_t)(v & 0xFFFFF), (uint32_t)((v >> 20) & 0xFFFFF), (uint32_t)(v >> 40)};
        E4 fp = bb::e_mul_fm(lam[air::N_TUPLE], bb::to_mont(tag));
        for (int j = 0; j < 4; j++) fp = bb::e_add(fp, bb::e_mul_fm(lam[j], bb::to_mont(g[j])));
        T = bb::e_add(T, bb::e_inv_m(bb::e_sub(alpha_l, fp)));
      };
      for (uint64_t k = cnt[0]; k < cnt[2]; k++) term(k, io.out[k], 2);
      for (uint64_t k = cnt[1]; k < cnt[3]; k++) term(k, io.in[k], 3);
    }
    if (deferred) memcpy(deferred->T_m, T.c, 16);                            // (without the cells' share: LK_TN below is not final, and nothing reads it before check 10)
    const E4 tn = bb::e_mul_fm(T, bb::to_mont(bb::inv((uint32_t)(N % bb::P))));
    for (int k = 0; k < 4; k++) lk_m[air::LK_TN + k] = tn.c[k];
  }
  ch.observe_n(aroot, 4);
  const E4 alpha = bb::e_to_mont(ch.sample_ext());
  ch.observe_n(qroot, 4);
  const E4 zeta = bb::e_to_mont(ch.sample_ext());
  // ---- 1. constraints at zeta: sum_c alpha^c C_c(zeta) == Q(zeta) Z_H(zeta), on the openings the proof states (main | aux at zeta, the same at zeta w, the quotient's four) ----
  const uint32_t wn = bb::root_of_unity(log_n), wn_m = bb::to_mont(wn);
  auto constraints_hold = [&](const E4* tz, const E4* tzw, const E4* qzs) {
    return constraints_at_zeta(tz, tzw, qzs, lk_m, alpha, zeta, log_n, pub.n_real, mode, WM, first, last, cnt);
  };
  // (deferred) check 10 BY VALUE: what constraints_hold reads, kept for zkir::mem_deferred_check; the front goes on as if the check held
  auto keep_check10 = [&](const E4* tz, const E4* tzw, const E4* qzs) {
    zkir::MemDeferred& D = *deferred;
    D.mode = mode; D.log_n = log_n; D.WM = WM; D.n_real = pub.n_real;
    D.ev.resize(4 * (size_t)(2 * WT + 4));
    memcpy(D.ev.data(), tz[0].c, 16 * (size_t)WT); memcpy(D.ev.data() + 4 * (size_t)WT, tzw[0].c, 16 * (size_t)WT); memcpy(D.ev.data() + 8 * (size_t)WT, qzs[0].c, 64);
    D.lk_m.assign(lk_m, lk_m + air::N_LK);
    D.states.assign(first, first + 2 * NS);
    memcpy(D.cnt, cnt, 16); memcpy(D.alpha_m, alpha.c, 16); memcpy(D.zeta_m, zeta.c, 16);
    D.blob = std::move(blob);                                              // (nothing behind check 10 reads the program)
    D.filled = true;
  };
  if (rate) {
    // ---- the 'ZKSR' tail: the embedded 'ZKBE' proof opens main (WM) | aux (WA) | quotient (4) with masks {3, 3, 1} at [zeta, zeta w], under the header's rate and parameters
    // (5: it states another shape; 4: too short to hold its evaluations); its evaluations satisfy the constraints (10); the evaluation proof's own verifier, told the outer
    // roots and points, accepts it (100 + its code)
    const uint32_t* e = w + p;
    const uint64_t elen = len - p;
    const size_t at_ev = 15 + 12 + 8, n_ev = (size_t)(2 * WT + 4);
    if (elen < at_ev + 4 * n_ev) return 4;
    const uint32_t shape[15] = {BATCH_EVAL_MAGIC, 1, (uint32_t)log_n, w[5], 3, 2, w[4], w[6], e[8], (uint32_t)WM, 3, (uint32_t)WA, 3, 4, 1};
    if (memcmp(e, shape, sizeof shape)) return 5;
    std::vector<E4> ev(n_ev);                                               // exponent order: main | aux | quotient at zeta, main | aux at zeta w
    for (size_t k = 0; k < n_ev; k++) { E4 x; memcpy(x.c, e + at_ev + 4 * k, 16); ev[k] = bb::e_to_mont(x); }
    if (deferred) keep_check10(ev.data(), ev.data() + WT + 4, ev.data() + WT);
    else if (!constraints_hold(ev.data(), ev.data() + WT + 4, ev.data() + WT)) return 10;
    uint32_t pts[8];
    const E4 z = bb::e_from_mont(zeta), zw = bb::e_from_mont(bb::e_mul_fm(zeta, wn_m));
    memcpy(pts, z.c, 16); memcpy(pts + 4, zw.c, 16);
    const int c = zkir::pcs_verify_with_stage(2, e, elen, troot, pts, nullptr, *rate->stage);       // (troot | aroot | qroot are consecutive proof words)
    return c ? 100 + c : 0;
  }
  ch.observe_n(w + at_tz, (size_t)(2 * WT + 4) * 4);
  const E4 gamma = bb::e_to_mont(ch.sample_ext());
  std::vector<E4> betas;
  if (!fri_transcript(ch, lroots, n_layers, w + at_fin, n_fin, pow_nonce, POW_BITS, betas)) return 12;
  if (deferred) keep_check10(t_z.data(), t_zw.data(), q_z.data());
  else if (!constraints_hold(t_z.data(), t_zw.data(), q_z.data())) return 10;
  // ---- 2. final codeword has degree < 4: the four upper coefficients of its interpolant over an order-8 coset vanish ----
  if (!fri_final_degree_ok(fin, 1)) return 11;
  // ---- 3. queries: the stage behind zkir::StarkQueryStage (verify_stages.h) gets what has been CHECKED and what has been DRAWN ----
  zkir::StarkQueries local_q;
  zkir::StarkQueries& Q = defer ? *defer : local_q;
  std::vector<E4> gp(2 * WT + 4);
  gp[0] = bb::e_one_m();
  for (size_t k = 1; k < gp.size(); k++) gp[k] = bb::e_mul_m(gp[k - 1], gamma);
  E4 a0 = bb::e_zero(), b0 = bb::e_zero();
  for (int k = 0; k < WT; k++) { a0 = bb::e_add(a0, bb::e_mul_m(gp[k], t_z[k])); b0 = bb::e_add(b0, bb::e_mul_m(gp[WT + k], t_zw[k])); }
  for (int i = 0; i < 4; i++) a0 = bb::e_add(a0, bb::e_mul_m(gp[2 * WT + i], q_z[i]));
  const E4 zeta_w = bb::e_mul_fm(zeta, wn_m);
  const int depth0 = log_n + 1;
  if (n_layers > (int)zkir::PCS_MAX_LAYERS) return 5;                       // (no log_n <= 26 has that many)
  Q.w = w; Q.len = len;
  Q.log_n = (uint32_t)log_n; Q.mode = (uint32_t)mode; Q.WM = (uint32_t)WM; Q.WA = (uint32_t)WA; Q.num_queries = (uint32_t)NUM_QUERIES; Q.n_layers = (uint32_t)n_layers;
  for (int j = 0; j < n_layers; j++) Q.ks[j] = (uint32_t)ks[j];
  Q.at_roots = (uint64_t)(troot - w); Q.at_lroots = (uint64_t)(lroots - w); Q.at_fin = at_fin; Q.at_queries = p;
  Q.qsize = 1 + 2 * ((size_t)WM + 4 * depth0) + 2 * ((size_t)WA + 4 * depth0) + 2 * ((size_t)4 + 4 * depth0) + (size_t)zkir::fri_query_words((uint32_t)depth0, ks);
  // the indices are drawn first (the transcript is sequential); the queries are independent of each other and all the same size
  Q.qs.resize(NUM_QUERIES);
  for (auto& q : Q.qs) q = ch.sample_bits(log_n);
  static_assert(sizeof(E4) == 16, "a vector of E4 is copied as 4 words an element");
  Q.betas_m.resize(4 * (size_t)n_layers); if (n_layers) memcpy(Q.betas_m.data(), betas[0].c, 16 * (size_t)n_layers);
  Q.gamma_m.resize(4 * gp.size()); memcpy(Q.gamma_m.data(), gp[0].c, 16 * gp.size());
  memcpy(Q.zeta_m, zeta.c, 16); memcpy(Q.zeta_w_m, zeta_w.c, 16); memcpy(Q.a0_m, a0.c, 16); memcpy(Q.b0_m, b0.c, 16);
  if (defer) return 0;                                                     // (the caller runs the stage over all it has collected, then check 30)
  int code = 0;
  const zkir::StarkQueryStage stage = zkir::host_stark_query_stage();
  const int src = stage.run(stage.self, &Q, 1, &code);
  if (src) return src;
  if (code) return code;
  return zkir::stark_length_check(Q);
}

// The host form of the STARK query stage (verify_stages.h): proof after proof, each proof's queries on a few host threads (round 5: ~10,000 Poseidon2 permutations — the
// Merkle paths — were 11 of the verifier's 12 ms on one core).  A proof's verdict is its first failing query's, in query order: exactly what a sequential loop returns.
int host_stark_queries_of(const zkir::StarkQueries& Q, uint32_t first) {
  const uint32_t* w = Q.w; const uint64_t len = Q.len;
  const int log_n = (int)Q.log_n, WM = (int)Q.WM, WA = (int)Q.WA, WT = WM + WA, n_layers = (int)Q.n_layers, NUM_QUERIES = (int)Q.num_queries, depth0 = log_n + 1;
  const size_t N = (size_t)1 << log_n, qsize = (size_t)Q.qsize, p_queries = (size_t)Q.at_queries, n_fin = zkir::fri_final_size(1);
  const uint32_t *troot = w + Q.at_roots, *aroot = troot + 4, *qroot = troot + 8, *lroots = w + Q.at_lroots;
  auto e4_at = [](const uint32_t* c) { E4 e; memcpy(e.c, c, 16); return e; };
  std::vector<E4> gp(2 * (size_t)WT + 4), betas(n_layers), fin(n_fin);
  for (size_t k = 0; k < gp.size(); k++) gp[k] = e4_at(Q.gamma_m.data() + 4 * k);
  for (int j = 0; j < n_layers; j++) betas[j] = e4_at(Q.betas_m.data() + 4 * j);
  for (size_t i = 0; i < n_fin; i++) fin[i] = bb::e_to_mont(e4_at(w + Q.at_fin + 4 * i));
  const E4 zeta = e4_at(Q.zeta_m), zeta_w = e4_at(Q.zeta_w_m), a0 = e4_at(Q.a0_m), b0 = e4_at(Q.b0_m);
  const uint32_t w2n = bb::root_of_unity(log_n + 1);
  const uint32_t* ks = Q.ks;
  const std::vector<uint32_t>& qs = Q.qs;
  auto check_query = [&](int t) -> int {
    size_t p = p_queries + (size_t)t * qsize;
    auto need = [&](size_t k) { return p + k <= len; };
    const uint32_t q = qs[t];
    if (!need(1) || w[p++] != q) return 20;
    E4 deep[2];
    const uint32_t* tl[2]; const uint32_t* al[2]; const uint32_t* ql[2];
    for (int s2 = 0; s2 < 2; s2++) {
      const size_t pos = (size_t)q + (s2 ? N : 0);
      if (!need((size_t)WM + 4 * depth0)) return 4;
      tl[s2] = w + p; p += WM;
      uint32_t dg[4]; hash_elems(tl[s2], WM, dg);
      if (!check_path(dg, pos, w + p, depth0, troot)) return 21;
      p += 4 * (size_t)depth0;
    }
    for (int s2 = 0; s2 < 2; s2++) {
      const size_t pos = (size_t)q + (s2 ? N : 0);
      if (!need((size_t)WA + 4 * depth0)) return 4;
      al[s2] = w + p; p += WA;
      uint32_t dg[4]; hash_elems(al[s2], WA, dg);
      if (!check_path(dg, pos, w + p, depth0, aroot)) return 27;
      p += 4 * (size_t)depth0;
    }
    for (int s2 = 0; s2 < 2; s2++) {
      const size_t pos = (size_t)q + (s2 ? N : 0);
      if (!need((size_t)4 + 4 * depth0)) return 4;
      ql[s2] = w + p; p += 4;
      uint32_t dg[4]; hash_elems(ql[s2], 4, dg);
      if (!check_path(dg, pos, w + p, depth0, qroot)) return 22;
      p += 4 * (size_t)depth0;
    }
    for (int s2 = 0; s2 < 2; s2++) {
      const size_t pos = (size_t)q + (s2 ? N : 0);
      const uint32_t x_m = bb::to_mont(bb::mul(bb::GEN, bb::pow(w2n, pos)));
      E4 A = bb::e_zero(), B = bb::e_zero();                               // canonical column value x Montgomery gamma^k = canonical; lifted to Montgomery at the end
      for (int k = 0; k < WM; k++) { A = bb::e_add(A, bb::e_mul_fm(gp[k], tl[s2][k])); B = bb::e_add(B, bb::e_mul_fm(gp[WT + k], tl[s2][k])); }
      for (int k = 0; k < WA; k++) { A = bb::e_add(A, bb::e_mul_fm(gp[WM + k], al[s2][k])); B = bb::e_add(B, bb::e_mul_fm(gp[WT + WM + k], al[s2][k])); }
      for (int i = 0; i < 4; i++) A = bb::e_add(A, bb::e_mul_fm(gp[2 * WT + i], ql[s2][i]));
      A = bb::e_to_mont(A); B = bb::e_to_mont(B);
      E4 dz = bb::e_zero(); dz.c[0] = x_m; E4 dzw = dz;
      dz = bb::e_sub(dz, zeta); dzw = bb::e_sub(dzw, zeta_w);
      deep[s2] = bb::e_add(bb::e_mul_m(bb::e_sub(A, a0), bb::e_inv_m(dz)), bb::e_mul_m(bb::e_sub(B, b0), bb::e_inv_m(dzw)));
    }
    FriWalk walk(log_n + 1, q);
    for (int j = 0; j < n_layers; j++) {
      const size_t layer_words = 4 * ((size_t)1 << ks[j]) + 4 * (size_t)(walk.log_m - ks[j]);
      if (!need(layer_words)) return 4;
      const FriLayerSeen seen = fri_walk_step(walk, w + p, (int)ks[j], lroots + 4 * j, betas[j]);
      p += layer_words;
      if (!seen.leaf_ok) return 23;
      if (j == 0) { if (!e_eq(seen.v0, deep[0]) || !e_eq(seen.v1, deep[1])) return 24; }
      else if (!seen.carried_ok) return 25;
    }
    if (!e_eq(fin[walk.carried_idx & (n_fin - 1)], walk.carried)) return 26;
    return 0;
  };
  std::vector<int> codes(NUM_QUERIES, 0);
  {
    unsigned n_thr = std::thread::hardware_concurrency() / 2;               // (half the logical cores, at most eight: SMT siblings and a busy host do not help a 10 ms job)
    n_thr = n_thr < 1 ? 1 : n_thr > 8 ? 8 : n_thr;
    if (const char* e = getenv("ZKIR_VERIFY_THREADS")) { const int v = atoi(e); if (v >= 1 && v <= 64) n_thr = (unsigned)v; }
    std::atomic<int> next{(int)first};
    auto work = [&]() { for (int t; (t = next.fetch_add(1)) < NUM_QUERIES;) codes[t] = check_query(t); };
    if ((log_n < 14 && !getenv("ZKIR_VERIFY_THREADS")) || (first && NUM_QUERIES - (int)first < 8)) n_thr = 1;            // (a small proof is checked faster than threads start)
    std::vector<std::thread> th;
    for (unsigned k = 1; k < n_thr; k++) {
      try { th.emplace_back(work); } catch (...) { break; }                 // (a host that refuses a thread — pids limit, sandbox — must not take the verdict down:
    }                                                                        //  the queries left over are checked on the calling thread, the threads that did start are joined)
    work();
    for (auto& x : th) x.join();
  }
  for (int t = (int)first; t < NUM_QUERIES; t++) if (codes[t]) return codes[t];
  return 0;
}
int host_stark_run(void*, const zkir::StarkQueries* list, uint32_t n, int* codes) {
  for (uint32_t i = 0; i < n; i++) codes[i] = host_stark_queries_of(list[i], 0);
  return 0;
}

}  // namespace

// ================================================================================================
// zkir_lowdeg_verify — the verifier of a LOW-DEGREE PROOF OF A COMMITMENT (zkir_lowdeg_prove, lowdeg.inl; spec: tests/lowdeg_ref.py).  Host only.
//
// The proof says: every column of the matrix committed under the root is close to a polynomial of degree < N = 2^log_n over the coset 31 <w_M>, M = N << b.  It says nothing
// else — no constraint, no opening at a point.  Batched FRI over C(x) = sum_k gamma^k col_k(x); the schedule, the final-degree check and the query width follow b.
//   [0..8)  'ZKLD', version 1, log_n, b, width, num_queries, pow_bits, n_layers | [8..12) the root | n_layers x 4 layer roots | n_fin x 4 final layer (n_fin = 4 << b) | nonce |
//   per query: q (< M/2), record(q), record(q + M/2) (zkir_merkle_open_launch's records), per layer 4 * 2^k values (value t = c[idx + t g]) and 4 * depth sibling words
// Transcript (the Challenger above): header, root, gamma; per layer root, beta; the final words; check_pow(nonce); q_t = sample_bits(log_n + b - 1).
// Codes, first failing check in this order, lowest query first: 1 malformed (length not EXACTLY the header's, magic, version, a range, n_layers), 2 not the expected root,
// 3 a word >= p (the whole proof is scanned before any product), 4 the final layer is not of degree < 4, 5 grinding, 6 a query's index word, 7 a matrix record does not hash to
// the root, 8 layer-0 values are not sum gamma^k row at q / q + M/2 (checked BEFORE layer 0's path), 9 a FRI leaf's path, 10 carried value != v[slot], 11 final value.
// ================================================================================================
namespace {

bool lowdeg_params_ok(uint32_t log_n, uint32_t b, uint32_t width, uint32_t num_queries) {
  return log_n >= 3 && log_n <= 26 && b >= 1 && b <= 3 && log_n + b <= 27 && width >= 1 && width <= 512 && num_queries >= 1 && num_queries <= 128;
}

constexpr uint32_t FRI_PART_MAX_MATS = zkir::PCS_MAX_MATS;

// The layer-0 value (Montgomery E4) the codeword has at row `pos`, from that row's opened words (rows[m]: matrix m's widths[m] words), by the rule PcsQueries states as data
E4 layer0_want(const zkir::PcsQueries& Q, size_t pos, const uint32_t* const* rows) {
  auto gp = [&](size_t e) { return E4{{Q.gamma_m[4 * e], Q.gamma_m[4 * e + 1], Q.gamma_m[4 * e + 2], Q.gamma_m[4 * e + 3]}}; };
  if (Q.n_points == 0) {
    const uint32_t* row = rows[0];
    E4 A = bb::e_zero();                                                    // canonical word x Montgomery gamma^k = canonical; lifted to Montgomery at the end
    for (size_t k = 0; k < Q.widths[0]; k++) A = bb::e_add(A, bb::e_mul_fm(gp(k), row[k]));
    return bb::e_to_mont(A);
  }
  const uint32_t x_m = bb::to_mont(bb::mul(bb::GEN, bb::pow(bb::root_of_unity((int)Q.log_M), pos)));
  E4 A[2] = {bb::e_zero(), bb::e_zero()};
  for (uint32_t si = 0; si < Q.n_sel; si++) {
    const zkir::PcsQueries::Sel& s = Q.sel[si];
    for (size_t k = 0; k < Q.widths[s.mat]; k++) A[s.point] = bb::e_add(A[s.point], bb::e_mul_fm(gp(s.e0 + k), rows[s.mat][k]));
  }
  E4 F = bb::e_zero();
  for (uint32_t i = 0; i < Q.n_points; i++) {
    E4 z, a; memcpy(z.c, Q.z_m[i], 16); memcpy(a.c, Q.a_m[i], 16);
    E4 d = z; d.c[0] = bb::sub(d.c[0], x_m);
    F = bb::e_add(F, bb::e_mul_m(bb::e_sub(a, bb::e_to_mont(A[i])), bb::e_inv_m(d)));
  }
  return F;
}

// The host form of the query stage (verify_stages.h): checks 6 .. 11, query after query
int host_query_run(void*, const zkir::PcsQueries& Q) {
  const uint32_t* w = Q.w;
  const int n_layers = (int)Q.n_layers, log_M = (int)Q.log_M;
  const size_t M = (size_t)1 << log_M, n_fin = zkir::fri_final_size((int)Q.b), at_queries = (size_t)Q.at_queries, qsize = (size_t)Q.qsize;
  const uint32_t n_mats = Q.n_mats;
  const uint32_t *widths = Q.widths, *roots = w + Q.at_roots, *lroots = w + Q.at_lroots, *qs = Q.qs;
  const uint32_t* ks = Q.ks;
  auto get_m = [&](size_t at) { return bb::e_to_mont(E4{{w[at], w[at + 1], w[at + 2], w[at + 3]}}); };
  std::vector<E4> fin(n_fin), betas(n_layers);
  for (size_t i = 0; i < n_fin; i++) fin[i] = get_m((size_t)Q.at_fin + 4 * i);
  for (int j = 0; j < n_layers; j++) memcpy(betas[j].c, Q.betas_m + 4 * j, 16);
  auto check_query = [&](int t) -> int {
    size_t p = at_queries + (size_t)t * qsize;
    const uint32_t q = qs[t];
    if (w[p++] != q) return 6;
    const uint32_t* rows[2][FRI_PART_MAX_MATS];                            // a query's records: matrix by matrix, row q then row q + M/2
    for (uint32_t m = 0; m < n_mats; m++)
      for (int s2 = 0; s2 < 2; s2++) {
        const size_t pos = (size_t)q + (s2 ? M / 2 : 0);
        const uint32_t* row = w + p;
        uint32_t dg[4]; hash_elems(row, widths[m], dg);
        if (!check_path(dg, pos, row + widths[m], log_M, roots + 4 * m)) return 7;
        rows[s2][m] = row;
        p += (size_t)widths[m] + 4 * (size_t)log_M;
      }
    E4 comb[2];
    for (int s2 = 0; s2 < 2; s2++) comb[s2] = layer0_want(Q, (size_t)q + (s2 ? M / 2 : 0), rows[s2]);
    FriWalk walk(log_M, q);
    for (int j = 0; j < n_layers; j++) {
      const int k = (int)ks[j];
      const size_t layer_words = 4 * ((size_t)1 << k) + 4 * (size_t)(walk.log_m - k);
      const FriLayerSeen seen = fri_walk_step(walk, w + p, k, lroots + 4 * j, betas[j]);
      p += layer_words;
      if (j == 0 && (!e_eq(seen.v0, comb[0]) || !e_eq(seen.v1, comb[1]))) return 8;
      if (!seen.leaf_ok) return 9;
      if (j > 0 && !seen.carried_ok) return 10;
    }
    if (!e_eq(fin[walk.carried_idx & (n_fin - 1)], walk.carried)) return 11;
    return 0;
  };
  // (the queries are independent; checked one after the other: a proof has at most 128 of them and its verdict is this loop's)
  for (int t = 0; t < (int)Q.num_queries; t++) { const int code = check_query(t); if (code) return code; }
  return 0;
}

// What zkir_lowdeg_verify, zkir_eval_verify and zkir_batch_eval_verify (and their *_device forms) share: checks 4 .. 11 of a proof whose FRI part (layer roots | final layer |
// nonce | queries) starts at word `at_lroots`.  A query opens n_mats (1 .. FRI_PART_MAX_MATS) matrices of widths[m] columns under the roots at word at_roots: record_m(q),
// record_m(q + M/2) matrix by matrix.  The caller has checked the shape and the words' range, hands over the transcript as it stands once gamma is drawn, and has filled Q's
// layer-0 rule (n_points, the gamma table, the selected pairs, z, a) — the one thing the proofs disagree about.  Checks 4 and 5 and the sampling are here; checks 6 .. 11 are
// the stage's (verify_stages.h).
int fri_part_verify(const uint32_t* w, uint64_t len, size_t at_roots, size_t at_lroots, uint32_t log_n, uint32_t b, uint32_t n_mats, const uint32_t* widths, uint32_t num_queries, uint32_t pow_bits,
                    const std::vector<int>& ks, Challenger& ch, zkir::PcsQueries& Q, const zkir::QueryStage& stage) {
  const int n_layers = (int)ks.size();
  const int log_M = (int)(log_n + b);
  const size_t n_fin = zkir::fri_final_size((int)b);
  const uint32_t* lroots = w + at_lroots;
  const size_t at_fin = at_lroots + 4 * (size_t)n_layers, at_nonce = at_fin + 4 * n_fin, at_queries = at_nonce + 1;
  auto get_m = [&](size_t at) { return bb::e_to_mont(E4{{w[at], w[at + 1], w[at + 2], w[at + 3]}}); };
  std::vector<E4> fin(n_fin);
  for (size_t i = 0; i < n_fin; i++) fin[i] = get_m(at_fin + 4 * i);
  // ---- 4: the final layer has degree < 4 ----
  if (!fri_final_degree_ok(fin, (int)b)) return 4;
  // ---- the transcript after gamma; 5: grinding ----
  std::vector<E4> betas;
  if (!fri_transcript(ch, lroots, n_layers, w + at_fin, n_fin, w[at_nonce], (int)pow_bits, betas)) return 5;
  std::vector<uint32_t> qs(num_queries);
  for (auto& q : qs) q = ch.sample_bits(log_M - 1);
  // ---- 6 .. 11: the query stage ----
  if (n_layers > (int)zkir::PCS_MAX_LAYERS || n_mats > zkir::PCS_MAX_MATS) return 1;      // (no header that passed check 1 states either)
  Q.w = w; Q.len = len;
  Q.log_M = (uint32_t)log_M; Q.b = b; Q.n_mats = n_mats; Q.n_layers = (uint32_t)n_layers; Q.num_queries = num_queries;
  for (uint32_t m = 0; m < n_mats; m++) Q.widths[m] = widths[m];
  for (int j = 0; j < n_layers; j++) Q.ks[j] = (uint32_t)ks[j];
  Q.at_roots = at_roots; Q.at_lroots = at_lroots; Q.at_fin = at_fin; Q.at_queries = at_queries; Q.qsize = (len - at_queries) / num_queries;
  Q.qs = qs.data(); Q.betas_m = betas[0].c;
  static_assert(sizeof(E4) == 16, "a vector of E4 is read as 4 words an element");
  return stage.run(stage.self, Q);
}

}  // namespace

extern "C" {

uint64_t zkir_lowdeg_proof_words(uint32_t log_n, uint32_t log_blowup, uint32_t width, uint32_t num_queries) {
  if (!lowdeg_params_ok(log_n, log_blowup, width, num_queries)) return 0;
  const std::vector<int> ks = zkir::fri_schedule((int)log_n, (int)log_blowup);
  const uint64_t qsize = 1 + 2 * ((uint64_t)width + 4 * (uint64_t)(log_n + log_blowup)) + zkir::fri_query_words(log_n + log_blowup, ks);
  return 12 + 4 * (uint64_t)ks.size() + 4 * (uint64_t)zkir::fri_final_size((int)log_blowup) + 1 + (uint64_t)num_queries * qsize;
}

namespace {
int lowdeg_verify_impl(const uint32_t* w, uint64_t len, const uint32_t* expect_root, const zkir::QueryStage& stage) {
  // ---- 1: shape ----
  if (!w || len < 12 || w[0] != 0x444C4B5Au || w[1] != 1) return 1;
  const uint32_t log_n = w[2], b = w[3], width = w[4], num_queries = w[5], pow_bits = w[6];
  if (!lowdeg_params_ok(log_n, b, width, num_queries) || pow_bits > 24) return 1;
  const std::vector<int> ks = zkir::fri_schedule((int)log_n, (int)b);
  if (w[7] != (uint32_t)ks.size() || len != zkir_lowdeg_proof_words(log_n, b, width, num_queries)) return 1;
  // ---- 2: the root ----
  const uint32_t* root = w + 8;
  if (expect_root && memcmp(root, expect_root, 16)) return 2;
  // ---- 3: canonical words ----
  for (uint64_t i = 0; i < len; i++) if (w[i] >= bb::P) return 3;
  // ---- the transcript up to gamma ----
  Challenger ch;
  ch.observe_n(w, 8);
  ch.observe_n(root, 4);
  const E4 gamma = bb::e_to_mont(ch.sample_ext());
  std::vector<E4> gp(width);
  gp[0] = bb::e_one_m();
  for (size_t k = 1; k < width; k++) gp[k] = bb::e_mul_m(gp[k - 1], gamma);
  // ---- 4 .. 11; 8: layer-0 values are sum gamma^k row ----
  zkir::PcsQueries Q{};
  Q.n_points = 0; Q.n_sel = 0; Q.n_gamma = width; Q.gamma_m = gp[0].c;
  return fri_part_verify(w, len, 8, 12, log_n, b, 1, &width, num_queries, pow_bits, ks, ch, Q, stage);
}
}  // namespace

int zkir_lowdeg_verify(const uint32_t* w, uint64_t len, const uint32_t* expect_root) { return lowdeg_verify_impl(w, len, expect_root, zkir::host_query_stage()); }

// ================================================================================================
// zkir_eval_verify and zkir_batch_eval_verify — the verifiers of an EVALUATION PROOF (zkir_eval_prove / zkir_batch_eval_prove, eval_open.inl).  Host only.
//
// The proof says: n_mats (1 .. 4) matrices committed over the same coset 31 <w_M>, M = N << b, each under its own root, have every column close to a polynomial of degree
// < N, and matrix m's columns take the proof's values at the points z_i (of the n_points (1 or 2) shared ones, in E4) its mask_m selects.  ONE batched FRI over
// F(x) = sum_i (a_i - A_i(x)) / (z_i - x), A_i(x) = sum gamma^e col_{m,k}(x), a_i = sum gamma^e y[i][m][k]; the exponent e runs consecutively for i over the points, for m
// over the matrices with bit i of mask_m set, in order, for k < width_m.  F is a polynomial of degree < N - 1 exactly when every claim holds.
// Two headers state it, and everything after the header is one layout:
//   'ZKBE' (spec: tests/batch_eval_ref.py)  [0..9) magic, version 1, log_n, b, n_mats, n_points, num_queries, pow_bits, n_layers | (width_m, mask_m) per matrix
//   'ZKEV' (spec: tests/eval_ref.py)        [0..9) magic, version 1, log_n, b, width, n_points, num_queries, pow_bits, n_layers: ONE matrix opened at every point (a full mask)
//   then: the n_mats roots | 4 n_points point words | the evaluations in the exponent order, 4 words each (one matrix: point-major) | the low-degree proof's layout:
//   n_layers x 4 layer roots | n_fin x 4 final layer | nonce | the queries; a query: q, then for each matrix in order record_m(q), record_m(q + M/2) (width_m + 4 log_M
//   words each), then per layer the values and the path
// Transcript: every word up to and including the evaluations, gamma; per layer root, beta; the final words; check_pow(nonce); q_t = sample_bits(log_n + b - 1).
// Codes, first failing check in this order, lowest query first: 1 malformed (length not EXACTLY the header's, magic, version, a range, n_points, n_layers; 'ZKBE': n_mats, a
// width, the width total (at most 512: one product per column per point in a 96-bit sum), a mask (0, or a bit at or above n_points), a point no matrix is opened at), 2 not
// the expected roots (all n_mats), 13 not the expected points or not the expected evaluations (NULL: any), 3 a word >= p, 12 a point in the base field (coordinates 1 .. 3 all
// zero) or two equal points, 4 the final layer is not of degree < 4, 5 grinding, 6 a query's index word, 7 a matrix record does not hash to its root (lowest matrix first
// within a query), 8 layer-0 values are not F at rows q / q + M/2, recomputed from all the opened records, the points and the evaluations (checked BEFORE layer 0's path),
// 9 a FRI leaf's path, 10 carried value != v[slot], 11 final value.
// ================================================================================================
namespace {

struct BatchShape { uint32_t n_mats, n_points, widths[4], masks[4]; uint64_t n_evals, sum_width; };
// the (width, mask) pairs of a batch are ones a proof can state
bool batch_shape_ok(uint32_t n_mats, uint32_t n_points, const uint32_t* widths, const uint32_t* masks, BatchShape* out) {
  if (n_mats < 1 || n_mats > 4 || n_points < 1 || n_points > 2) return false;
  BatchShape sh{};
  sh.n_mats = n_mats; sh.n_points = n_points;
  uint32_t used = 0;
  for (uint32_t m = 0; m < n_mats; m++) {
    if (widths[m] < 1 || widths[m] > 512 || masks[m] < 1 || masks[m] >= (1u << n_points)) return false;
    sh.widths[m] = widths[m]; sh.masks[m] = masks[m];
    sh.sum_width += widths[m]; used |= masks[m];
    sh.n_evals += (uint64_t)widths[m] * (uint64_t)__builtin_popcount(masks[m]);
  }
  if (sh.sum_width > 512 || used != (1u << n_points) - 1) return false;
  *out = sh;
  return true;
}

// Everything after check 1 of either header: the roots section starts at word at_roots, the shape and the length are checked, ks is the schedule of (log_n, b).
int eval_core_verify(const BatchShape& sh, size_t at_roots, const uint32_t* w, uint64_t len, const std::vector<int>& ks, const uint32_t* expect_roots, const uint32_t* expect_points,
                     const uint32_t* expect_evals, const zkir::QueryStage& stage) {
  const uint32_t log_n = w[2], b = w[3], n_mats = sh.n_mats, n_points = sh.n_points, num_queries = w[6], pow_bits = w[7];
  const uint32_t *roots = w + at_roots, *pts = roots + 4 * (size_t)n_mats, *ys = pts + 4 * (size_t)n_points;
  const size_t at_lroots = at_roots + 4 * (size_t)n_mats + 4 * (size_t)n_points + 4 * (size_t)sh.n_evals;
  // ---- 2, 13: what the caller expects, read at the sizes the header states ----
  if (expect_roots && memcmp(roots, expect_roots, 16 * (size_t)n_mats)) return 2;
  if (expect_points && memcmp(pts, expect_points, 16 * (size_t)n_points)) return 13;
  if (expect_evals && memcmp(ys, expect_evals, 16 * (size_t)sh.n_evals)) return 13;
  // ---- 3: canonical words ----
  for (uint64_t i = 0; i < len; i++) if (w[i] >= bb::P) return 3;
  // ---- 12: the points lie outside the base field (so z - x is invertible for every x of it) and differ ----
  for (uint32_t i = 0; i < n_points; i++) if (!(pts[4 * i + 1] | pts[4 * i + 2] | pts[4 * i + 3])) return 12;
  if (n_points == 2 && !memcmp(pts, pts + 4, 16)) return 12;
  // ---- the transcript up to gamma ----
  Challenger ch;
  ch.observe_n(w, at_lroots);
  const E4 gamma = bb::e_to_mont(ch.sample_ext());
  auto get_m = [&](const uint32_t* at) { return bb::e_to_mont(E4{{at[0], at[1], at[2], at[3]}}); };
  std::vector<E4> gp((size_t)sh.n_evals);
  gp[0] = bb::e_one_m();
  for (size_t k = 1; k < gp.size(); k++) gp[k] = bb::e_mul_m(gp[k - 1], gamma);
  zkir::PcsQueries Q{};                                                     // the selected (point, matrix) pairs in the exponent order
  E4 z[2], a[2];
  {
    size_t e = 0;
    for (uint32_t i = 0; i < n_points; i++) {
      z[i] = get_m(pts + 4 * i);
      a[i] = bb::e_zero();
      for (uint32_t m = 0; m < n_mats; m++) {
        if (!((sh.masks[m] >> i) & 1)) continue;
        Q.sel[Q.n_sel++] = {i, m, (uint32_t)e};
        for (size_t k = 0; k < sh.widths[m]; k++, e++) a[i] = bb::e_add(a[i], bb::e_mul_m(gp[e], get_m(ys + 4 * e)));
      }
      memcpy(Q.z_m[i], z[i].c, 16); memcpy(Q.a_m[i], a[i].c, 16);
    }
  }
  Q.n_points = n_points; Q.n_gamma = (uint32_t)gp.size(); Q.gamma_m = gp[0].c;
  // ---- 4 .. 11; 8: layer-0 values are F at the two rows, from all the matrices' records ----
  return fri_part_verify(w, len, at_roots, at_lroots, log_n, b, n_mats, sh.widths, num_queries, pow_bits, ks, ch, Q, stage);
}

}  // namespace

uint64_t zkir_batch_eval_proof_words(uint32_t log_n, uint32_t log_blowup, uint32_t n_mats, const uint32_t* widths, const uint32_t* masks, uint32_t n_points, uint32_t num_queries) {
  BatchShape sh;
  if (!widths || !masks || !batch_shape_ok(n_mats, n_points, widths, masks, &sh)) return 0;
  const uint64_t ld = zkir_lowdeg_proof_words(log_n, log_blowup, 1, num_queries);      // one matrix of one column: 12 header and root words, 2 (1 + 4 log_M) record words a query
  if (ld == 0) return 0;
  const uint64_t log_M = (uint64_t)log_n + log_blowup;
  return ld - 12 + 9 + 6 * (uint64_t)n_mats + 4 * (uint64_t)n_points + 4 * sh.n_evals + (uint64_t)num_queries * (2 * sh.sum_width - 2 + 8 * log_M * (n_mats - 1));
}

// the batch of one matrix with a full mask, less its (width, mask) pair
uint64_t zkir_eval_proof_words(uint32_t log_n, uint32_t log_blowup, uint32_t width, uint32_t n_points, uint32_t num_queries) {
  if (n_points < 1 || n_points > 2) return 0;
  const uint32_t mask = (1u << n_points) - 1;
  const uint64_t words = zkir_batch_eval_proof_words(log_n, log_blowup, 1, &width, &mask, n_points, num_queries);
  return words ? words - 2 : 0;
}

namespace {
int eval_verify_impl(const uint32_t* w, uint64_t len, const uint32_t* expect_root, const uint32_t* expect_points, const uint32_t* expect_evals, const zkir::QueryStage& stage) {
  // ---- 1: shape ----
  if (!w || len < 9 || w[0] != 0x56454B5Au || w[1] != 1) return 1;
  const uint32_t log_n = w[2], b = w[3], width = w[4], n_points = w[5], num_queries = w[6], pow_bits = w[7];
  if (n_points < 1 || n_points > 2) return 1;
  const uint32_t mask = (1u << n_points) - 1;                               // one matrix is opened at every point
  BatchShape sh;
  if (!batch_shape_ok(1, n_points, &width, &mask, &sh) || !lowdeg_params_ok(log_n, b, 1, num_queries) || pow_bits > 24) return 1;
  const std::vector<int> ks = zkir::fri_schedule((int)log_n, (int)b);
  if (w[8] != (uint32_t)ks.size() || len != zkir_eval_proof_words(log_n, b, width, n_points, num_queries)) return 1;
  return eval_core_verify(sh, 9, w, len, ks, expect_root, expect_points, expect_evals, stage);
}

int batch_eval_verify_impl(const uint32_t* w, uint64_t len, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals, const zkir::QueryStage& stage) {
  // ---- 1: shape ----
  if (!w || len < 9 || w[0] != 0x45424B5Au || w[1] != 1) return 1;
  const uint32_t log_n = w[2], b = w[3], n_mats = w[4], n_points = w[5], num_queries = w[6], pow_bits = w[7];
  if (n_mats < 1 || n_mats > 4 || n_points < 1 || n_points > 2 || len < 9 + 2 * (uint64_t)n_mats) return 1;
  uint32_t widths[4], masks[4];
  for (uint32_t m = 0; m < n_mats; m++) { widths[m] = w[9 + 2 * m]; masks[m] = w[10 + 2 * m]; }
  BatchShape sh;
  if (!batch_shape_ok(n_mats, n_points, widths, masks, &sh) || !lowdeg_params_ok(log_n, b, 1, num_queries) || pow_bits > 24) return 1;
  const std::vector<int> ks = zkir::fri_schedule((int)log_n, (int)b);
  if (w[8] != (uint32_t)ks.size() || len != zkir_batch_eval_proof_words(log_n, b, n_mats, widths, masks, n_points, num_queries)) return 1;
  return eval_core_verify(sh, 9 + 2 * (size_t)n_mats, w, len, ks, expect_roots, expect_points, expect_evals, stage);
}
}  // namespace

int zkir_eval_verify(const uint32_t* w, uint64_t len, const uint32_t* expect_root, const uint32_t* expect_points, const uint32_t* expect_evals) {
  return eval_verify_impl(w, len, expect_root, expect_points, expect_evals, zkir::host_query_stage());
}
int zkir_batch_eval_verify(const uint32_t* w, uint64_t len, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals) {
  return batch_eval_verify_impl(w, len, expect_roots, expect_points, expect_evals, zkir::host_query_stage());
}
int zkir_verify_rate(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits) {
  return zkir::rate_verify_with_stage(proof, proof_words, expect, min_queries, min_pow_bits, zkir::host_query_stage());
}
// a 'ZKSR' proof of a SEGMENT of a run (zkir_prove_rate_segment): zkir_verify_rate without check 7; the boundary states out on acceptance
int zkir_verify_rate_segment(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits, uint32_t first_state[68],
                             uint32_t last_state[68]) {
  uint32_t st[2 * NS];
  const int rc = zkir::rate_segment_verify_with_stage(proof, proof_words, expect, min_queries, min_pow_bits, zkir::host_query_stage(), st, nullptr);
  if (rc == 0) { if (first_state) memcpy(first_state, st, NS * 4); if (last_state) memcpy(last_state, st + NS, NS * 4); }
  return rc;
}
int zkir_verify_rate_chain(const uint32_t* const* proofs, const uint64_t* proof_words, uint32_t n_segments, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits) {
  if (proofs && proof_words && n_segments == 1 && proofs[0] && proof_words[0] > 9 && proofs[0][9] >= 3) return zkir_verify_rate(proofs[0], proof_words[0], expect, min_queries, min_pow_bits);      // a whole run by itself
  return zkir::rate_chain_with_stage(proofs, proof_words, n_segments, expect, min_queries, min_pow_bits, zkir::host_pcs_many_stage());
}

}  // extern "C"

// ================================================================================================
// zkir_mixed_eval_verify — the verifier of an EVALUATION PROOF OVER SEVERAL HEIGHTS (zkir_mixed_eval_prove, mixed_eval.inl; spec: tests/mixed_eval_ref.py).  Host code; zkir_mixed_eval_verify_device
// (mixed_verify.inl) runs the same code with the query stage (verify_stages.h: MixedQueries, checks 6 .. 11) on the device.
//
// The proof says: n_groups (2 or 3) groups at one rate b, of strictly decreasing heights; group h is what a 'ZKBE' proof states at height log_n_h (1 .. 4 matrices over
// 31 <w_{M_h}>, M_h = N_h << b, each under its own root; its own 1 or 2 points; a mask per matrix).  ONE gamma, drawn after everything up to the evaluations; its exponent runs
// consecutively through the groups in order and inside a group in 'ZKBE''s order.  F_h = 'ZKBE''s quotient of group h with those exponents.  ONE FRI (fri_mixed_schedule: every
// M_h is a committed layer's size): layer 0 is F_0, and the layer of size M_h is the fold of the layer before it PLUS F_h, by index.
//   [0..7) 'ZKMH', version 1, b, n_groups, num_queries, pow_bits, n_layers | per group: log_n, n_mats, n_points, (width, mask) per matrix | all roots (groups in order, matrices
//   in order) | all points | all evaluations in the exponent order | n_layers x 4 layer roots | n_fin x 4 final layer | nonce | the queries; a query: q, then group 0's matrices
//   record_m(q), record_m(q + M_0/2), then each lower group's matrices ONE record_m(q mod M_h) (width_m + 4 log M_h words), then per layer the values and the path
// Transcript: every word up to and including the evaluations, gamma; per layer root, beta; the final words; check_pow(nonce); q_t = sample_bits(log M_0 - 1).
// Codes, 'ZKBE''s in 'ZKBE''s order: 1 malformed (length not EXACTLY the header's, magic, version, a range, n_groups, heights not strictly decreasing, a group's shape,
// n_layers), 2 roots, 13 points / evaluations, 3 a word >= p, 12 a point in the base field or two equal points within a group, 4 final layer, 5 grinding, 6 index word, 7 a
// record (in the order they stand in the query), 8 layer-0 values from group 0's records, 9 a FRI leaf's path, 10 carried value — BEFORE the step into the layer of size M_h the
// carried value becomes carried + F_h(q mod M_h), recomputed from group h's records by layer0_want's rule at log M_h — 11 final value.  (A false evaluation followed by the honest procedure
// folds a quotient with a pole: check 4, in any group.  Layers committed for other evaluations than the stated ones: 8 in group 0, 10 in a lower group.)
// ================================================================================================
namespace {

constexpr uint32_t MIXED_MAGIC = 0x484D4B5Au, MIXED_MAX_GROUPS = 3;
struct MixedShape {
  uint32_t b, n_groups, log_n[MIXED_MAX_GROUPS];
  BatchShape g[MIXED_MAX_GROUPS];
  uint64_t n_mats, n_points, n_evals;                                      // over all the groups
};
// the groups are ones a proof can state (flat arrays, groups concatenated)
bool mixed_shape_ok(uint32_t b, uint32_t n_groups, const uint32_t* log_ns, const uint32_t* n_mats, const uint32_t* n_points, const uint32_t* widths, const uint32_t* masks, MixedShape* out) {
  if (b < 1 || b > 3 || n_groups < 2 || n_groups > MIXED_MAX_GROUPS) return false;
  MixedShape sh{};
  sh.b = b; sh.n_groups = n_groups;
  for (uint32_t h = 0; h < n_groups; h++) {
    if (log_ns[h] < 3 || log_ns[h] > 26 || log_ns[h] + b > 27 || (h && log_ns[h] >= log_ns[h - 1])) return false;
    if (n_mats[h] < 1 || n_mats[h] > 4 || !batch_shape_ok(n_mats[h], n_points[h], widths + sh.n_mats, masks + sh.n_mats, &sh.g[h])) return false;
    sh.log_n[h] = log_ns[h];
    sh.n_mats += n_mats[h]; sh.n_points += n_points[h]; sh.n_evals += sh.g[h].n_evals;
  }
  *out = sh;
  return true;
}
uint64_t mixed_words(const MixedShape& sh, uint32_t num_queries, std::vector<int>* ks_out) {
  const std::vector<int> ks = zkir::fri_mixed_schedule(sh.log_n, sh.n_groups, (int)sh.b);
  uint64_t head = 7, qsize = 1 + zkir::fri_query_words(sh.log_n[0] + sh.b, ks);
  for (uint32_t h = 0; h < sh.n_groups; h++) {
    head += 3 + 2 * (uint64_t)sh.g[h].n_mats;
    qsize += (h ? 1 : 2) * (sh.g[h].sum_width + 4 * (uint64_t)(sh.log_n[h] + sh.b) * sh.g[h].n_mats);
  }
  if (ks_out) *ks_out = ks;
  return head + 4 * sh.n_mats + 4 * sh.n_points + 4 * sh.n_evals + 4 * (uint64_t)ks.size() + 4 * (uint64_t)zkir::fri_final_size((int)sh.b) + 1 + (uint64_t)num_queries * qsize;
}

}  // namespace

extern "C" {

uint64_t zkir_mixed_eval_proof_words(uint32_t log_blowup, uint32_t n_groups, const uint32_t* log_ns, const uint32_t* n_mats, const uint32_t* n_points, const uint32_t* widths,
                                     const uint32_t* masks, uint32_t num_queries) {
  MixedShape sh;
  if (!log_ns || !n_mats || !n_points || !widths || !masks || num_queries < 1 || num_queries > 128) return 0;
  if (n_groups < 2 || n_groups > MIXED_MAX_GROUPS) return 0;               // (before the arrays are read: they have n_groups entries)
  for (uint32_t h = 0; h < n_groups; h++) if (n_mats[h] < 1 || n_mats[h] > 4) return 0;      // (widths and masks have sum n_mats entries)
  if (!mixed_shape_ok(log_blowup, n_groups, log_ns, n_mats, n_points, widths, masks, &sh)) return 0;
  return mixed_words(sh, num_queries, nullptr);
}

}  // extern "C"

namespace {

// The host form of the mixed query stage (verify_stages.h): checks 6 .. 11, query after query
int host_mixed_query_run(void*, const zkir::MixedQueries& MQ) {
  const uint32_t* w = MQ.w;
  const zkir::PcsQueries* Q = MQ.g;
  const uint32_t n_groups = MQ.n_groups;
  const int n_layers = (int)MQ.n_layers, log_M = (int)Q[0].log_M;
  const size_t M = (size_t)1 << log_M, n_fin = zkir::fri_final_size((int)MQ.b), at_queries = (size_t)MQ.at_queries, qsize = (size_t)MQ.qsize;
  const uint32_t *roots = w + MQ.at_roots, *lroots = w + MQ.at_lroots;
  const uint32_t* ks = MQ.ks;
  std::vector<E4> fin(n_fin), betas(n_layers);
  for (size_t i = 0; i < n_fin; i++) { const uint32_t* a = w + MQ.at_fin + 4 * i; fin[i] = bb::e_to_mont(E4{{a[0], a[1], a[2], a[3]}}); }
  for (int j = 0; j < n_layers; j++) memcpy(betas[j].c, MQ.betas_m + 4 * j, 16);
  for (uint32_t t = 0; t < MQ.num_queries; t++) {
    const uint32_t q = MQ.qs[t];
    size_t p = at_queries + (size_t)t * qsize;
    if (w[p++] != q) return 6;
    const uint32_t* rows[MIXED_MAX_GROUPS][2][4];                           // group 0: rows q and q + M_0/2; a lower group: the row q mod M_h at [h][0]
    for (uint32_t h = 0; h < n_groups; h++) {
      const int log_Mh = (int)Q[h].log_M;
      for (uint32_t m = 0; m < Q[h].n_mats; m++)
        for (int s2 = 0; s2 < (h ? 1 : 2); s2++) {
          const size_t pos = h ? (q & (((size_t)1 << log_Mh) - 1)) : (size_t)q + (s2 ? M / 2 : 0);
          const uint32_t* row = w + p;
          uint32_t dg[4]; hash_elems(row, Q[h].widths[m], dg);
          if (!check_path(dg, pos, row + Q[h].widths[m], log_Mh, roots + 4 * (MQ.first_mat[h] + m))) return 7;
          rows[h][s2][m] = row;
          p += (size_t)Q[h].widths[m] + 4 * (size_t)log_Mh;
        }
    }
    const E4 comb[2] = {layer0_want(Q[0], q, rows[0][0]), layer0_want(Q[0], (size_t)q + M / 2, rows[0][1])};
    FriWalk walk(log_M, q);
    for (int j = 0; j < n_layers; j++) {
      const int k = (int)ks[j];
      for (uint32_t h = 1; h < n_groups; h++)                                // the layer of size M_h is the fold plus F_h: what is carried into it gains F_h(q mod M_h)
        if ((int)Q[h].log_M == walk.log_m) walk.carried = bb::e_add(walk.carried, layer0_want(Q[h], walk.carried_idx, rows[h][0]));
      const size_t layer_words = 4 * ((size_t)1 << k) + 4 * (size_t)(walk.log_m - k);
      const FriLayerSeen seen = fri_walk_step(walk, w + p, k, lroots + 4 * j, betas[j]);
      p += layer_words;
      if (j == 0 && (!e_eq(seen.v0, comb[0]) || !e_eq(seen.v1, comb[1]))) return 8;
      if (!seen.leaf_ok) return 9;
      if (j > 0 && !seen.carried_ok) return 10;
    }
    if (!e_eq(fin[walk.carried_idx & (n_fin - 1)], walk.carried)) return 11;
  }
  return 0;
}

int mixed_eval_verify_impl(const uint32_t* w, uint64_t len, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals, const zkir::MixedQueryStage& stage) {
  // ---- 1: shape ----
  if (!w || len < 7 || w[0] != MIXED_MAGIC || w[1] != 1) return 1;
  const uint32_t b = w[2], n_groups = w[3], num_queries = w[4], pow_bits = w[5];
  if (b < 1 || b > 3 || n_groups < 2 || n_groups > MIXED_MAX_GROUPS || num_queries < 1 || num_queries > 128 || pow_bits > 24) return 1;
  uint32_t log_ns[MIXED_MAX_GROUPS], n_mats[MIXED_MAX_GROUPS], n_points[MIXED_MAX_GROUPS], widths[4 * MIXED_MAX_GROUPS], masks[4 * MIXED_MAX_GROUPS];
  size_t at = 7, n_m = 0;
  for (uint32_t h = 0; h < n_groups; h++) {
    if (len < at + 3) return 1;
    log_ns[h] = w[at]; n_mats[h] = w[at + 1]; n_points[h] = w[at + 2];
    if (n_mats[h] < 1 || n_mats[h] > 4 || len < at + 3 + 2 * (uint64_t)n_mats[h]) return 1;
    for (uint32_t m = 0; m < n_mats[h]; m++, n_m++) { widths[n_m] = w[at + 3 + 2 * m]; masks[n_m] = w[at + 4 + 2 * m]; }
    at += 3 + 2 * (size_t)n_mats[h];
  }
  MixedShape sh;
  if (!mixed_shape_ok(b, n_groups, log_ns, n_mats, n_points, widths, masks, &sh)) return 1;
  std::vector<int> ks;
  if (len != mixed_words(sh, num_queries, &ks) || w[6] != (uint32_t)ks.size()) return 1;
  const size_t at_roots = at, at_points = at_roots + 4 * (size_t)sh.n_mats, at_evals = at_points + 4 * (size_t)sh.n_points, at_lroots = at_evals + 4 * (size_t)sh.n_evals;
  const uint32_t *roots = w + at_roots, *pts = w + at_points, *ys = w + at_evals;
  // ---- 2, 13: what the caller expects, read at the sizes the header states ----
  if (expect_roots && memcmp(roots, expect_roots, 16 * (size_t)sh.n_mats)) return 2;
  if (expect_points && memcmp(pts, expect_points, 16 * (size_t)sh.n_points)) return 13;
  if (expect_evals && memcmp(ys, expect_evals, 16 * (size_t)sh.n_evals)) return 13;
  // ---- 3: canonical words ----
  for (uint64_t i = 0; i < len; i++) if (w[i] >= bb::P) return 3;
  // ---- 12: every point lies outside the base field; the points of one group differ ----
  {
    const uint32_t* p = pts;
    for (uint32_t h = 0; h < n_groups; p += 4 * (size_t)n_points[h], h++) {
      for (uint32_t i = 0; i < n_points[h]; i++) if (!(p[4 * i + 1] | p[4 * i + 2] | p[4 * i + 3])) return 12;
      if (n_points[h] == 2 && !memcmp(p, p + 4, 16)) return 12;
    }
  }
  // ---- the transcript up to gamma; each group's layer-0 rule (layer0_want's data) with the group's exponents ----
  Challenger ch;
  ch.observe_n(w, at_lroots);
  const E4 gamma = bb::e_to_mont(ch.sample_ext());
  auto get_m = [&](const uint32_t* a) { return bb::e_to_mont(E4{{a[0], a[1], a[2], a[3]}}); };
  std::vector<E4> gp((size_t)sh.n_evals);
  gp[0] = bb::e_one_m();
  for (size_t k = 1; k < gp.size(); k++) gp[k] = bb::e_mul_m(gp[k - 1], gamma);
  zkir::MixedQueries MQ{};
  zkir::PcsQueries* Q = MQ.g;
  uint32_t* first_mat = MQ.first_mat;
  {
    size_t e = 0, m0 = 0, p0 = 0;
    for (uint32_t h = 0; h < n_groups; h++) {
      zkir::PcsQueries& q = Q[h];
      const BatchShape& g = sh.g[h];
      q.log_M = log_ns[h] + b; q.b = b; q.n_mats = g.n_mats; q.n_points = g.n_points;
      q.n_gamma = (uint32_t)gp.size(); q.gamma_m = gp[0].c;                 // (e0 below counts from the proof's first exponent)
      for (uint32_t m = 0; m < g.n_mats; m++) q.widths[m] = g.widths[m];
      for (uint32_t i = 0; i < g.n_points; i++) {
        const E4 z = get_m(pts + 4 * (p0 + i));
        E4 a = bb::e_zero();
        for (uint32_t m = 0; m < g.n_mats; m++) {
          if (!((g.masks[m] >> i) & 1)) continue;
          q.sel[q.n_sel++] = {i, m, (uint32_t)e};
          for (size_t k = 0; k < g.widths[m]; k++, e++) a = bb::e_add(a, bb::e_mul_m(gp[e], get_m(ys + 4 * e)));
        }
        memcpy(q.z_m[i], z.c, 16); memcpy(q.a_m[i], a.c, 16);
      }
      first_mat[h] = (uint32_t)m0; m0 += g.n_mats; p0 += g.n_points;
    }
  }
  // ---- 4: the final layer; the transcript after gamma; 5: grinding ----
  const int n_layers = (int)ks.size(), log_M = (int)(log_ns[0] + b);
  const size_t n_fin = zkir::fri_final_size((int)b);
  const uint32_t* lroots = w + at_lroots;
  const size_t at_fin = at_lroots + 4 * (size_t)n_layers, at_nonce = at_fin + 4 * n_fin, at_queries = at_nonce + 1, qsize = (size_t)((len - at_queries) / num_queries);
  std::vector<E4> fin(n_fin), betas;
  for (size_t i = 0; i < n_fin; i++) fin[i] = get_m(w + at_fin + 4 * i);
  if (!fri_final_degree_ok(fin, (int)b)) return 4;
  if (!fri_transcript(ch, lroots, n_layers, w + at_fin, n_fin, w[at_nonce], (int)pow_bits, betas)) return 5;
  std::vector<uint32_t> qs(num_queries);
  for (auto& q : qs) q = ch.sample_bits(log_M - 1);
  // ---- 6 .. 11: the query stage ----
  if (n_layers > (int)zkir::MIXED_MAX_LAYERS || sh.n_mats + sh.g[0].n_mats + (uint64_t)n_layers > zkir::MIXED_MAX_SLOTS) return 1;      // (no header that passed check 1 states either)
  MQ.w = w; MQ.len = len;
  MQ.n_groups = n_groups; MQ.b = b; MQ.n_layers = (uint32_t)n_layers; MQ.num_queries = num_queries;
  for (int j = 0; j < n_layers; j++) MQ.ks[j] = (uint32_t)ks[j];
  MQ.at_roots = at_roots; MQ.at_lroots = at_lroots; MQ.at_fin = at_fin; MQ.at_queries = at_queries; MQ.qsize = qsize;
  MQ.qs = qs.data(); MQ.betas_m = betas[0].c;
  return stage.run(stage.self, MQ);
}

}  // namespace

extern "C" {

int zkir_mixed_eval_verify(const uint32_t* w, uint64_t len, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals) {
  return mixed_eval_verify_impl(w, len, expect_roots, expect_points, expect_evals, zkir::host_mixed_query_stage());
}

}  // extern "C"

namespace zkir {
QueryStage host_query_stage() { return QueryStage{nullptr, host_query_run}; }
int rate_verify_with_stage(const uint32_t* proof, uint64_t n_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits, const QueryStage& stage, const TapeStages* tapes,
                           const MemStages* mem) {
  const RateCheck rate{min_queries, min_pow_bits, &stage};
  return verify_impl(proof, n_words, expect, true, nullptr, nullptr, tapes, nullptr, &rate, mem);
}
int pcs_verify_with_stage(int kind, const uint32_t* proof, uint64_t n_words, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals, const QueryStage& stage) {
  if (kind == 0) return lowdeg_verify_impl(proof, n_words, expect_roots, stage);
  if (kind == 1) return eval_verify_impl(proof, n_words, expect_roots, expect_points, expect_evals, stage);
  return batch_eval_verify_impl(proof, n_words, expect_roots, expect_points, expect_evals, stage);
}
int rate_segment_verify_with_stage(const uint32_t* proof, uint64_t n_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits, const QueryStage& stage,
                                   uint32_t* states_out, uint32_t* counters_out) {
  const RateCheck rate{min_queries, min_pow_bits, &stage};
  return verify_impl(proof, n_words, expect, false, states_out, counters_out, nullptr, nullptr, &rate);
}
namespace {
int pcs_collect_run(void* self, const PcsQueries& Q) {
  PcsCollected& c = *static_cast<PcsCollected*>(self);
  c.q = Q;
  c.qs.assign(Q.qs, Q.qs + Q.num_queries);
  c.betas_m.assign(Q.betas_m, Q.betas_m + 4 * (size_t)Q.n_layers);
  c.gamma_m.assign(Q.gamma_m, Q.gamma_m + 4 * (size_t)Q.n_gamma);
  c.q.qs = c.qs.data(); c.q.betas_m = c.betas_m.data(); c.q.gamma_m = c.gamma_m.data();
  c.filled = true;
  return 0;
}
int host_pcs_many_run(void*, const PcsCollected* list, uint32_t n, int* codes) {
  for (uint32_t i = 0; i < n; i++) { codes[i] = host_query_run(nullptr, list[i].q); if (codes[i] < 0) return codes[i]; }
  return 0;
}
}  // namespace
QueryStage pcs_collect_stage(PcsCollected* out) { return QueryStage{out, pcs_collect_run}; }
PcsManyStage host_pcs_many_stage() { return PcsManyStage{nullptr, host_pcs_many_run}; }
MixedQueryStage host_mixed_query_stage() { return MixedQueryStage{nullptr, host_mixed_query_run}; }
int mixed_eval_verify_with_stage(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals, const MixedQueryStage& stage) {
  return mixed_eval_verify_impl(proof, n_words, expect_roots, expect_points, expect_evals, stage);
}

// ---- the memory stages over a list of proofs (verify_stages.h) ----
MemLocated mem_section_locate(const uint32_t* w, uint64_t len, bool rate) {
  MemLocated L;
  if (!w || len < (uint64_t)HEADER_WORDS || w[0] != (rate ? RATE_MAGIC : PROOF_MAGIC) || (w[9] != 3 && w[9] != 4)) return L;
  const int mode = (int)w[9];
  size_t p = (size_t)header_words_of(mode);
  if (p >= len) return L;
  const size_t blob_len = w[p++];
  if (blob_len > ((size_t)1 << 30) || blob_len < 32 || p + (blob_len + 1) / 2 > len) return L;
  const uint64_t code_size = (uint64_t)(w[p + 8] & 0xFFFF) | ((uint64_t)(w[p + 9] & 0xFFFF) << 16);      // blob bytes 16 .. 19 (the front has checked the halfwords by then)
  p += (blob_len + 1) / 2;
  IoSection io;
  if (!parse_io_section(w + p, (size_t)len - p, io)) return L;
  p += io.words;
  L.ok = true; L.at = p; L.avail = len - p; L.mode = mode; L.code_words = code_size / 4;
  return L;
}
bool mem_deferred_check(const MemDeferred& d, const uint32_t T_mem[4]) {
  const size_t WT = (d.ev.size() / 4 - 4) / 2;
  std::vector<E4> ev(d.ev.size() / 4);
  memcpy(ev[0].c, d.ev.data(), d.ev.size() * 4);
  std::vector<uint32_t> lk(d.lk_m);
  E4 T, Tm, alpha, zeta;
  memcpy(T.c, d.T_m, 16); memcpy(Tm.c, T_mem, 16); memcpy(alpha.c, d.alpha_m, 16); memcpy(zeta.c, d.zeta_m, 16);
  const uint64_t N = (uint64_t)1 << d.log_n;
  const E4 tn = bb::e_mul_fm(bb::e_add(T, Tm), bb::to_mont(bb::inv((uint32_t)(N % bb::P))));
  for (int k = 0; k < 4; k++) lk[air::LK_TN + k] = tn.c[k];
  return constraints_at_zeta(ev.data(), ev.data() + WT, ev.data() + 2 * WT, lk.data(), alpha, zeta, d.log_n, d.n_real, d.mode, d.WM, d.states.data(), d.states.data() + NS, d.cnt);
}
namespace {
int host_mem_many_prepare(void*, const MemSection* list, uint32_t n, int* verdicts, uint32_t* digests) {
  uint64_t chunk0 = 0;
  for (uint32_t i = 0; i < n; i++) {
    size_t used = 0;
    verdicts[i] = host_mem_check(nullptr, list[i].sec, 1 + 7 * (size_t)list[i].n, list[i].mode, list[i].code_words, &used);
    if (!verdicts[i]) section_digests_host(list[i].sec, used, digests + 4 * chunk0);
    chunk0 += mem_section_chunks(list[i].n);
  }
  return 0;
}
int host_mem_many_side(void*, const MemSection* list, const MemSideJob* jobs, uint32_t n_jobs, uint32_t* sums) {
  for (uint32_t j = 0; j < n_jobs; j++) { const MemSection& S = list[jobs[j].section]; mem_side_sum(S.sec, (size_t)S.n, jobs[j].blob, jobs[j].blob_len, jobs[j].lk_m, sums + 4 * j); }
  return 0;
}

// One proof of a list entry: its MemStages answer from what prepare returned where the front hands over the located section, else from the host stage functions.
struct ManyMemProof {
  const uint32_t* w = nullptr;
  MemLocated loc;
  int slot = -1;                                                 // the proof's section in the list (-1: none went to the list stage)
  uint64_t n = 0;
  int verdict = 0; const uint32_t* dg = nullptr;                 // prepare's answers
  HostMem host;
  MemDeferred def;
};
int mm_check(void* p, const uint32_t* sec, size_t avail, int mode, uint64_t code_words, size_t* used) {
  ManyMemProof& P = *static_cast<ManyMemProof*>(p);
  if (P.slot < 0 || sec != P.w + P.loc.at || avail != P.loc.avail || mode != P.loc.mode || code_words != P.loc.code_words) return host_mem_check(&P.host, sec, avail, mode, code_words, used);
  if (P.verdict) return P.verdict;
  P.def.armed = true;
  *used = 1 + 7 * (size_t)P.n;
  return 0;
}
int mm_digests(void* p, const uint32_t* sec, size_t len, uint32_t* dg) {
  ManyMemProof& P = *static_cast<ManyMemProof*>(p);
  if (!P.def.armed) return host_mem_digests(nullptr, sec, len, dg);
  if (len != 1 + 7 * (size_t)P.n) { set_last_error({ZKIR_ERR_OTHER, "zkir_verify_many_memory: a front asked for the digests of another section than the one it checked"}); return -ZKIR_ERR_OTHER; }
  memcpy(dg, P.dg, 16 * (size_t)mem_section_chunks(P.n));
  return 0;
}
int mm_side(void* p, const uint32_t* lk_m, const uint8_t* blob, size_t blob_len, uint32_t T[4]) {
  ManyMemProof& P = *static_cast<ManyMemProof*>(p);
  if (!P.def.armed) return host_mem_side(&P.host, lk_m, blob, blob_len, T);
  set_last_error({ZKIR_ERR_OTHER, "zkir_verify_many_memory: a deferring front asked for its table side"});
  return -ZKIR_ERR_OTHER;
}
// ---- the tape stages over a list of proofs (verify_stages.h) ----
int host_tape_many_prepare(void*, const TapeSection* list, uint32_t n, int* hv, uint64_t* used, int* wv, uint32_t* digests) {
  uint64_t chunk0 = 0;
  for (uint32_t i = 0; i < n; i++) {
    const TapeSection& S = list[i];
    HostTapes h; size_t u = 0;
    hv[i] = host_hash_check(&h, S.hash, (size_t)S.avail, S.n_real, S.code_end, &u);
    used[i] = hv[i] ? 0 : u;
    wv[i] = S.wide ? host_wide_check(&h, S.wide, (size_t)S.n_wide, S.n_real) : 0;
    const uint64_t c0 = tape_section_chunks(S, 0), c1 = tape_section_chunks(S, 1);
    if (!hv[i] && c0) section_digests_host(S.hash, u, digests + 4 * chunk0);      // (a passing section is whole: u = hash_words)
    if (c1) section_digests_host(S.wide, 1 + 8 * (size_t)S.n_wide, digests + 4 * (chunk0 + c0));
    chunk0 += c0 + c1;
  }
  return 0;
}
int host_tape_many_sides(void*, const TapeSection* list, const TapeSideJob* jobs, uint32_t n_jobs, uint32_t* sums) {
  for (uint32_t j = 0; j < n_jobs; j++) {
    const TapeSection& S = list[jobs[j].section];
    HostTapes h; size_t u = 0;
    memset(sums + 8 * (size_t)j, 0, 32);
    if (jobs[j].hash) {
      if (host_hash_check(&h, S.hash, (size_t)S.avail, S.n_real, S.code_end, &u)) { set_last_error({ZKIR_ERR_OTHER, "the tape list stage: a side was asked for of a hash section that fails its check"}); return -ZKIR_ERR_OTHER; }
      host_hash_side(&h, jobs[j].lk_m, sums + 8 * (size_t)j);
    }
    if (jobs[j].wide && S.wide) { h.wide = S.wide; h.n_wide = (size_t)S.n_wide; host_wide_side(&h, jobs[j].lk_m, sums + 8 * (size_t)j + 4); }
  }
  return 0;
}
// One mode-4 proof of a list entry: its TapeStages answer from what prepare returned where the front hands over what was located, else from the host stage functions.
struct ManyTapeProof {
  TapeSection sec{};
  int slot = -1;                                                 // the proof's tapes in the list (-1: none went to the list stage)
  int hv = 0, wv = 0; uint64_t used = 0; const uint32_t* dg = nullptr;      // prepare's answers
  bool hash_batch = false, wide_batch = false;                   // the front's check was answered by the list: that share waits for the sides call
  HostTapes host;                                                // what the host stage functions keep where they ran instead
  MemDeferred* def = nullptr;
};
int tm_hash_check(void* p, const uint32_t* w, size_t avail, uint64_t n_real, uint64_t code_end, size_t* used) {
  ManyTapeProof& P = *static_cast<ManyTapeProof*>(p);
  // (an EMPTY hash tape beside a wide tape that went to the list has nothing to defer: the host stage, one word)
  if (P.slot < 0 || w != P.sec.hash || avail != P.sec.avail || n_real != P.sec.n_real || code_end != P.sec.code_end || P.sec.hash[0] == 0) return host_hash_check(&P.host, w, avail, n_real, code_end, used);
  if (P.hv) return P.hv;
  P.hash_batch = true; P.def->tapes_armed = true;
  *used = (size_t)P.used;
  return 0;
}
int tm_wide_check(void* p, const uint32_t* sec, size_t n_wide, uint64_t n_real) {
  ManyTapeProof& P = *static_cast<ManyTapeProof*>(p);
  if (P.slot < 0 || !P.sec.wide || sec != P.sec.wide || n_wide != P.sec.n_wide || n_real != P.sec.n_real) return host_wide_check(&P.host, sec, n_wide, n_real);
  if (P.wv) return P.wv;
  P.wide_batch = true; P.def->tapes_armed = true;
  return 0;
}
int tm_digests(void* p, int which, const uint32_t* sw, size_t sl, uint32_t* dg) {
  ManyTapeProof& P = *static_cast<ManyTapeProof*>(p);
  if (!(which ? P.wide_batch : P.hash_batch)) return host_digests(nullptr, which, sw, sl, dg);
  if (sl != (which ? 1 + 8 * (size_t)P.sec.n_wide : (size_t)P.used)) { set_last_error({ZKIR_ERR_OTHER, "zkir_verify_many_tapes: a front asked for the digests of another section than the one it checked"}); return -ZKIR_ERR_OTHER; }
  memcpy(dg, P.dg + (which ? 4 * (size_t)tape_section_chunks(P.sec, 0) : 0), 16 * (size_t)tape_section_chunks(P.sec, which));
  return 0;
}
int tm_side(ManyTapeProof& P, bool wide, const uint32_t* lk_m, uint32_t T[4]) {
  if (!P.def->tapes_armed) return wide ? host_wide_side(&P.host, lk_m, T) : host_hash_side(&P.host, lk_m, T);
  set_last_error({ZKIR_ERR_OTHER, "zkir_verify_many_tapes: a deferring front asked for a table side"});
  return -ZKIR_ERR_OTHER;
}
int tm_hash_side(void* p, const uint32_t* lk_m, uint32_t T[4]) { return tm_side(*static_cast<ManyTapeProof*>(p), false, lk_m, T); }
int tm_wide_side(void* p, const uint32_t* lk_m, uint32_t T[4]) { return tm_side(*static_cast<ManyTapeProof*>(p), true, lk_m, T); }
struct TapeManyDone {
  const TapeManyStage* st; bool called = false;
  void call() { if (!called && st && st->done) st->done(st->self); called = true; }
  ~TapeManyDone() { call(); }
};
struct MemManyDone {                                             // the stage's done on every way out
  const MemManyStage& st; bool called = false;
  void call() { if (!called && st.done) st.done(st.self); called = true; }
  ~MemManyDone() { call(); }
};

// Phase A, the fronts and phase B of a list entry; front(i, mem, tapes) is proof i's front (mem: NULL where the memory batch stays with the inline host code; tapes: NULL
// where no tape batch went through the list stage, and the front keeps the tape stages it always had) and answers its verdict so far (negative: no verdict for the call).
// out[i]: 10 where a deferred check failed, else the front's answer.  tr: NULL, or the tape list stage around the same fronts.
template <typename Front>
int mem_many_fronts(const uint32_t* const* proofs, const uint64_t* proof_words, uint32_t n, bool rate, const MemManyStage& st, uint64_t min_cells, const MemManyProbe& probe,
                    const TapeManyRun* tr, Front front, std::vector<int32_t>& out, MemManyNote* note) {
  *note = MemManyNote{};
  if (tr && tr->note) *tr->note = TapeManyNote{};
  TapeManyDone tdone{tr ? tr->stage : nullptr};
  MemManyDone done{st};
  std::vector<ManyMemProof> P(n);
  std::vector<MemSection> list;
  uint64_t cells = 0, chunks = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t* w = proofs[i];
    P[i].w = w;
    P[i].loc = mem_section_locate(w, proof_words[i], rate);
    if (!P[i].loc.ok || P[i].loc.avail < 1) continue;
    const uint64_t nc = w[P[i].loc.at];
    if (nc == 0 || nc > ((uint64_t)1 << 28) || (P[i].loc.avail - 1) / 7 < nc) continue;      // (empty, or the host stage's check 4)
    P[i].slot = (int)list.size(); P[i].n = nc;
    list.push_back(MemSection{w + P[i].loc.at, nc, P[i].loc.mode, P[i].loc.code_words});
    cells += nc; chunks += mem_section_chunks(nc);
  }
  const bool batch = !list.empty() && cells >= min_cells;
  // the tapes: every located pair that holds a record at all (a proof with two empty tapes has nothing to defer)
  std::vector<ManyTapeProof> TP(tr ? n : 0);
  std::vector<TapeSection> tlist;
  uint64_t records = 0, tchunks = 0;
  if (tr) for (uint32_t i = 0; i < n; i++) {
    TP[i].def = &P[i].def;
    const TapeLocated L = tape_sections_locate(proofs[i], proof_words[i], P[i].loc);
    if (!L.ok) continue;
    TapeSection S = L.sec;
    if (!S.n_wide) S.wide = nullptr;
    if (S.hash[0] == 0 && !S.wide) continue;
    TP[i].sec = S; TP[i].slot = (int)tlist.size();
    tlist.push_back(S);
    records += S.n_full + S.n_wide; tchunks += tape_section_chunks(S, 0) + tape_section_chunks(S, 1);
  }
  const bool tbatch = tr && !tlist.empty() && records >= tr->min_records;
  std::vector<int> sv(list.size(), 0);
  std::vector<uint32_t> dg(batch ? 4 * (size_t)chunks : 0);
  if (batch) {
    const int rc = st.prepare(st.self, list.data(), (uint32_t)list.size(), sv.data(), dg.data());
    if (rc) return rc < 0 ? rc : -rc;
    uint64_t chunk0 = 0;
    for (uint32_t i = 0; i < n; i++) if (P[i].slot >= 0) { P[i].verdict = sv[P[i].slot]; P[i].dg = dg.data() + 4 * chunk0; chunk0 += mem_section_chunks(P[i].n); }
  }
  std::vector<int> thv(tlist.size(), 0), twv(tlist.size(), 0);
  std::vector<uint64_t> tused(tlist.size(), 0);
  std::vector<uint32_t> tdg(tbatch ? 4 * (size_t)tchunks : 0);
  if (tbatch) {
    const int rc = tr->stage->prepare(tr->stage->self, tlist.data(), (uint32_t)tlist.size(), thv.data(), tused.data(), twv.data(), tdg.data());
    if (rc) return rc < 0 ? rc : -rc;
    uint64_t chunk0 = 0;
    for (uint32_t i = 0; i < n; i++) if (TP[i].slot >= 0) {
      ManyTapeProof& T = TP[i];
      T.hv = thv[T.slot]; T.wv = twv[T.slot]; T.used = tused[T.slot]; T.dg = tdg.data() + 4 * chunk0;
      chunk0 += tape_section_chunks(T.sec, 0) + tape_section_chunks(T.sec, 1);
    }
  } else for (ManyTapeProof& T : TP) T.slot = -1;
  for (uint32_t i = 0; i < n; i++) {
    const MemStages ms{&P[i], mm_check, mm_digests, mm_side, &P[i].def};
    TapeStages ts{nullptr, tm_hash_check, tm_wide_check, tm_digests, tm_hash_side, tm_wide_side, &P[i].def};
    if (tbatch) ts.self = &TP[i];
    const int rc = front(i, batch ? &ms : nullptr, tbatch ? &ts : nullptr);
    if (rc < 0) return rc;
    out[i] = rc;
  }
  // phase B: every proof whose front kept check 10, with the shares it left out
  std::vector<MemSideJob> jobs;
  std::vector<TapeSideJob> tjobs;
  std::vector<uint32_t> who, twho;
  for (uint32_t i = 0; i < n; i++) if (P[i].def.filled) {
    if (P[i].def.armed) { jobs.push_back(MemSideJob{(uint32_t)P[i].slot, P[i].def.lk_m.data(), P[i].def.blob.data(), P[i].def.blob.size()}); who.push_back(i); }
    if (P[i].def.tapes_armed && (TP[i].hash_batch || TP[i].wide_batch)) { tjobs.push_back(TapeSideJob{(uint32_t)TP[i].slot, P[i].def.lk_m.data(), TP[i].hash_batch, TP[i].wide_batch}); twho.push_back(i); }
  }
  std::vector<E4> share(n, bb::e_zero());
  auto add_to = [&](uint32_t i, const uint32_t* t) { E4 x; memcpy(x.c, t, 16); share[i] = bb::e_add(share[i], x); };
  if (!jobs.empty()) {
    std::vector<uint32_t> sums(4 * jobs.size(), 0);
    const int rc = st.side(st.self, list.data(), jobs.data(), (uint32_t)jobs.size(), sums.data());
    if (rc) return rc < 0 ? rc : -rc;
    for (size_t j = 0; j < jobs.size(); j++) {
      uint32_t* Tm = sums.data() + 4 * j;
      if (probe.what == 1 && probe.index == who[j]) Tm[0] = bb::add(Tm[0], bb::R1);
      add_to(who[j], Tm);
    }
  }
  if (!tjobs.empty()) {
    std::vector<uint32_t> sums(8 * tjobs.size(), 0);
    const int rc = tr->stage->sides(tr->stage->self, tlist.data(), tjobs.data(), (uint32_t)tjobs.size(), sums.data());
    if (rc) return rc < 0 ? rc : -rc;
    for (size_t j = 0; j < tjobs.size(); j++) { add_to(twho[j], sums.data() + 8 * j); add_to(twho[j], sums.data() + 8 * j + 4); }
  }
  for (uint32_t i = 0; i < n; i++) if (P[i].def.filled) {
    if (P[i].def.tapes_armed) {                                    // (a check the list did not answer for this front: the host stage kept what its side needs)
      uint32_t t[4];
      if (!TP[i].hash_batch) { host_hash_side(&TP[i].host, P[i].def.lk_m.data(), t); add_to(i, t); }
      if (!TP[i].wide_batch) { host_wide_side(&TP[i].host, P[i].def.lk_m.data(), t); add_to(i, t); }
      if (tr->probe.index == i && ((tr->probe.what == 1 && TP[i].hash_batch) || (tr->probe.what == 2 && TP[i].wide_batch))) share[i].c[0] = bb::add(share[i].c[0], bb::R1);      // (the probed share, where the list answered that check)
    }
    if (!mem_deferred_check(P[i].def, share[i].c)) out[i] = 10;
  }
  tdone.call();
  done.call();
  if (batch) { note->cells = cells; note->sections = (uint32_t)list.size(); note->deferred = (uint32_t)jobs.size(); }
  if (tbatch && tr->note) { tr->note->records = records; tr->note->sections = (uint32_t)tlist.size(); tr->note->deferred = (uint32_t)tjobs.size(); }
  return 0;
}
}  // namespace
MemManyStage host_mem_many_stage() { return MemManyStage{nullptr, host_mem_many_prepare, host_mem_many_side, nullptr}; }
TapeManyStage host_tape_many_stage() { return TapeManyStage{nullptr, host_tape_many_prepare, host_tape_many_sides, nullptr}; }
TapeLocated tape_sections_locate(const uint32_t* w, uint64_t len, const MemLocated& loc) {
  TapeLocated L;
  if (!w || !loc.ok || loc.mode != 4 || loc.avail < 1) return L;
  const uint64_t nc = w[loc.at];
  if (nc > ((uint64_t)1 << 28) || (loc.avail - 1) / 7 < nc) return L;      // (the memory stage's check 4)
  const uint64_t at = loc.at + 1 + 7 * nc;
  if (at >= len) return L;
  TapeSection& S = L.sec;
  S.hash = w + at; S.avail = len - at;
  const TapeExtent x = tape_section_walk(S.hash, S.avail, nullptr);
  S.n_full = x.n_full; S.hash_words = x.used; S.whole = x.whole;
  S.n_real = (uint64_t)w[7] | ((uint64_t)w[8] << 30); S.code_end = air::CODE_BASE + 4 * loc.code_words;
  if (S.code_end >> 32) return L;                                   // (a code size no program has: the device record holds 32 bits, the host stage takes it)
  S.wide = nullptr; S.n_wide = 0;
  if (x.whole && x.used < S.avail) {
    const uint64_t nw = S.hash[x.used];
    if (nw <= S.n_real && nw <= ((uint64_t)1 << 28) && (S.avail - x.used - 1) / 8 >= nw) { S.wide = S.hash + x.used; S.n_wide = nw; }
  }
  L.ok = true;
  return L;
}

int verify_many_with_mem_stage(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, const MemManyStage& mem,
                               uint64_t min_cells, const TapeStagesFor* tapes, const StarkQueryStage& queries, const MemManyProbe& probe, int32_t* verdicts, MemManyNote* note,
                               const TapeManyRun* tape_run) {
  std::vector<int32_t> out(n, 0);
  std::vector<StarkQueries> Q(n);
  const int frc = mem_many_fronts(proofs, proof_words, n, false, mem, min_cells, probe, tape_run, [&](uint32_t i, const MemStages* ms, const TapeStages* listed) -> int {
    const uint32_t* w = proofs[i];
    if (listed) return stark_verify_collect(w, proof_words[i], expects ? expects[i] : nullptr, true, listed, &Q[i], ms);
    const bool with_tapes = tapes && w && proof_words[i] >= 10 && w[9] == 4;
    const TapeStages* ts = with_tapes ? tapes->begin(tapes->self, i) : nullptr;
    if (with_tapes && !ts) return -ZKIR_ERR_DEVICE;
    const int rc = stark_verify_collect(w, proof_words[i], expects ? expects[i] : nullptr, true, ts, &Q[i], ms);
    return with_tapes ? tapes->end(tapes->self, rc) : rc;
  }, out, note);
  if (frc) return frc;
  std::vector<StarkQueries> list;
  std::vector<uint32_t> who;
  for (uint32_t i = 0; i < n; i++) if (!out[i]) { list.push_back(std::move(Q[i])); who.push_back(i); }
  std::vector<int> codes(list.size() + 1, 0);
  if (!list.empty()) {                                             // (no proof reached its queries: nothing is run)
    const int src = queries.run(queries.self, list.data(), (uint32_t)list.size(), codes.data());
    if (src) return src < 0 ? src : -src;
  }
  for (size_t k = 0; k < list.size(); k++) out[who[k]] = codes[k] ? codes[k] : stark_length_check(list[k]);
  memcpy(verdicts, out.data(), (size_t)n * sizeof(int32_t));
  return 0;
}

int rate_many_with_mem_stage(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, const uint32_t* min_queries,
                             const uint32_t* min_pow_bits, uint32_t n, const MemManyStage& mem, uint64_t min_cells, const TapeStagesFor* tapes, const PcsManyStage& queries,
                             const MemManyProbe& probe, int32_t* verdicts, MemManyNote* note, const TapeManyRun* tape_run) {
  std::vector<int32_t> out(n, 0);
  std::vector<PcsCollected> C(n);
  const int frc = mem_many_fronts(proofs, proof_words, n, true, mem, min_cells, probe, tape_run, [&](uint32_t i, const MemStages* ms, const TapeStages* listed) -> int {
    const uint32_t* w = proofs[i];
    const bool with_tapes = !listed && tapes && w && proof_words[i] >= 10 && w[9] == 4;
    const TapeStages* ts = listed ? listed : with_tapes ? tapes->begin(tapes->self, i) : nullptr;
    if (with_tapes && !ts) return -ZKIR_ERR_DEVICE;
    int rc = rate_verify_with_stage(w, proof_words[i], expects ? expects[i] : nullptr, min_queries ? min_queries[i] : 1u, min_pow_bits ? min_pow_bits[i] : 0u, pcs_collect_stage(&C[i]), ts, ms);
    if (with_tapes) rc = tapes->end(tapes->self, rc);
    if (!rc && !C[i].filled) { set_last_error({ZKIR_ERR_OTHER, "zkir_verify_rate_many_memory: a front accepted a proof without reaching its queries"}); return -(int)ZKIR_ERR_OTHER; }
    return rc;
  }, out, note);
  if (frc) return frc;
  std::vector<PcsCollected> list;
  std::vector<uint32_t> who;
  for (uint32_t i = 0; i < n; i++) if (!out[i]) { list.push_back(std::move(C[i])); who.push_back(i); }
  for (PcsCollected& c : list) { c.q.qs = c.qs.data(); c.q.betas_m = c.betas_m.data(); c.q.gamma_m = c.gamma_m.data(); }      // (a moved description points at its own tables)
  std::vector<int> codes(list.size() + 1, 0);
  if (!list.empty()) {
    const int src = queries.run(queries.self, list.data(), (uint32_t)list.size(), codes.data());
    if (src) return src < 0 ? src : -src;
  }
  for (size_t k = 0; k < list.size(); k++) out[who[k]] = codes[k] ? 100 + codes[k] : 0;
  memcpy(verdicts, out.data(), (size_t)n * sizeof(int32_t));
  return 0;
}

int mem_sections_stage(const char* who, const MemManyStage& st, const uint32_t* const* secs, const uint64_t* n_words, const uint32_t* modes, const uint64_t* code_words, const uint8_t* const* blobs,
                       const size_t* blob_lens, const uint32_t* alphas, const uint32_t* lambdas, uint32_t n, int32_t* verdicts, uint32_t* digests, uint32_t* sums) {
  auto refuse = [&](const std::string& why) { set_last_error({ZKIR_ERR_ARGUMENT, std::string(who) + ": " + why}); return (int)ZKIR_ERR_ARGUMENT; };
  if (!secs || !n_words || !modes || !code_words || !blobs || !blob_lens || !alphas || !lambdas || !verdicts || !digests || !sums) return refuse("null argument");
  if (n < 1 || n > 1024) return refuse("n must be 1 .. 1024");
  try {
    MemManyDone done{st};
    std::vector<MemSection> list(n);
    std::vector<uint32_t> lk((size_t)n * air::N_LK);
    for (uint32_t i = 0; i < n; i++) {
      uint64_t nc = 0;
      if (const char* why = mem_side_args(secs[i], n_words[i], blobs[i], blob_lens[i], alphas + 4 * i, lambdas + 4 * i, sums, lk.data() + (size_t)i * air::N_LK, &nc)) return refuse(why);
      if (modes[i] != 3 && modes[i] != 4) return refuse("a mode must be 3 or 4");
      list[i] = MemSection{secs[i], nc, (int)modes[i], code_words[i]};
    }
    std::vector<int> sv(n, 0);
    int rc = st.prepare(st.self, list.data(), n, sv.data(), digests);
    if (rc) return rc < 0 ? -rc : rc;
    std::vector<MemSideJob> jobs;
    uint64_t chunk0 = 0;
    for (uint32_t i = 0; i < n; i++) {                               // (a failing section has no digests: zero)
      const uint64_t nch = mem_section_chunks(list[i].n);
      verdicts[i] = sv[i];
      if (sv[i]) memset(digests + 4 * chunk0, 0, 16 * (size_t)nch); else jobs.push_back(MemSideJob{i, lk.data() + (size_t)i * air::N_LK, blobs[i], blob_lens[i]});
      chunk0 += nch;
    }
    std::vector<uint32_t> T(4 * jobs.size() + 4, 0);
    if (!jobs.empty()) { rc = st.side(st.self, list.data(), jobs.data(), (uint32_t)jobs.size(), T.data()); if (rc) return rc < 0 ? -rc : rc; }
    memset(sums, 0, 16 * (size_t)n);
    for (size_t j = 0; j < jobs.size(); j++) { E4 t; memcpy(t.c, T.data() + 4 * j, 16); t = bb::e_from_mont(t); memcpy(sums + 4 * (size_t)jobs[j].section, t.c, 16); }
  } catch (const std::exception& e) { set_last_error({ZKIR_ERR_OTHER, std::string(who) + ": " + e.what()}); return ZKIR_ERR_OTHER; }
  return ZKIR_OK;
}

int tape_sections_stage(const char* who, const TapeManyStage& st, const uint32_t* const* hash_secs, const uint64_t* hash_words, const uint32_t* const* wide_secs, const uint64_t* wide_words,
                        const uint64_t* n_real, const uint64_t* code_end, const uint32_t* alphas, const uint32_t* lambdas, uint32_t n, int32_t* hash_verdicts, int32_t* wide_verdicts,
                        uint32_t* digests, uint32_t* sums) {
  auto refuse = [&](const std::string& why) { set_last_error({ZKIR_ERR_ARGUMENT, std::string(who) + ": " + why}); return (int)ZKIR_ERR_ARGUMENT; };
  if (!hash_secs || !hash_words || !wide_secs || !wide_words || !n_real || !code_end || !alphas || !lambdas || !hash_verdicts || !wide_verdicts || !digests || !sums) return refuse("null argument");
  if (n < 1 || n > 1024) return refuse("n must be 1 .. 1024");
  try {
    std::vector<TapeSection> list(n);
    std::vector<uint32_t> lk((size_t)n * air::N_LK, 0);
    TapeManyDone done{&st};
    std::vector<uint8_t> wide_over(n, 0);                          // a count above n_real is the front's own 57: such a list does not reach the stage
    uint64_t out_chunks = 0, in_chunks = 0;
    for (uint32_t i = 0; i < n; i++) {
      if (!hash_secs[i] || !wide_secs[i] || hash_words[i] < 1 || wide_words[i] < 1) return refuse("a section must hold its count word");
      if (hash_words[i] >> 31 || wide_words[i] >> 31) return refuse("a section is too long");
      for (int k = 0; k < 4; k++) if (alphas[4 * i + k] >= bb::P || lambdas[4 * i + k] >= bb::P) return refuse("alpha and lambda must be canonical");
      if (wide_words[i] != 1 + 8 * (uint64_t)wide_secs[i][0]) return refuse("a wide section must be [n] + 8 n words");
      TapeSection& S = list[i];
      S.hash = hash_secs[i]; S.avail = hash_words[i];
      const TapeExtent x = tape_section_walk(S.hash, S.avail, nullptr);
      if (x.whole && x.used != S.avail) return refuse("words behind a hash section's last record");
      S.n_full = x.n_full; S.hash_words = x.used; S.whole = x.whole;
      S.n_real = n_real[i]; S.code_end = code_end[i];
      S.n_wide = wide_secs[i][0]; S.wide = S.n_wide ? wide_secs[i] : nullptr;
      if (S.n_wide > S.n_real) { wide_over[i] = 1; S.wide = nullptr; S.n_wide = 0; }
      uint32_t* l = lk.data() + (size_t)i * air::N_LK;
      E4 a, l1, lam = bb::e_one_m();
      memcpy(a.c, alphas + 4 * i, 16); memcpy(l1.c, lambdas + 4 * i, 16);
      a = bb::e_to_mont(a); l1 = bb::e_to_mont(l1);
      memcpy(l + air::LK_ALPHA, a.c, 16);
      for (int j = 0; j <= air::N_TUPLE; j++) { memcpy(l + air::LK_LAM + 4 * j, lam.c, 16); lam = bb::e_mul_m(lam, l1); }
      out_chunks += (hash_words[i] + 511) / 512 + (wide_words[i] + 511) / 512;
      in_chunks += tape_section_chunks(S, 0) + tape_section_chunks(S, 1);
    }
    std::vector<int> hv(n, 0), wv(n, 0);
    std::vector<uint64_t> used(n, 0);
    std::vector<uint32_t> dg(4 * (size_t)in_chunks + 4, 0);
    int rc = st.prepare(st.self, list.data(), n, hv.data(), used.data(), wv.data(), dg.data());
    if (rc) return rc < 0 ? -rc : rc;
    memset(digests, 0, 16 * (size_t)out_chunks);
    memset(sums, 0, 32 * (size_t)n);
    std::vector<TapeSideJob> jobs;
    uint64_t oc = 0, ic = 0;
    for (uint32_t i = 0; i < n; i++) {
      const TapeSection& S = list[i];
      const uint64_t c0 = tape_section_chunks(S, 0), c1 = tape_section_chunks(S, 1), o0 = (hash_words[i] + 511) / 512;
      hash_verdicts[i] = hv[i]; wide_verdicts[i] = wide_over[i] ? 57 : wv[i];
      if (!hv[i]) memcpy(digests + 4 * oc, dg.data() + 4 * ic, 16 * (size_t)c0);      // (a passing section is whole: c0 = o0)
      if (!wide_verdicts[i]) {
        if (S.wide) memcpy(digests + 4 * (oc + o0), dg.data() + 4 * (ic + c0), 16 * (size_t)c1);
        else section_digests_host(wide_secs[i], 1, digests + 4 * (oc + o0));      // (the empty wide section: its count word alone)
      }
      if (!hv[i] && !wide_verdicts[i]) jobs.push_back(TapeSideJob{i, lk.data() + (size_t)i * air::N_LK, true, S.wide != nullptr});
      oc += o0 + (wide_words[i] + 511) / 512; ic += c0 + c1;
    }
    std::vector<uint32_t> T(8 * jobs.size() + 8, 0);
    if (!jobs.empty()) { rc = st.sides(st.self, list.data(), jobs.data(), (uint32_t)jobs.size(), T.data()); if (rc) return rc < 0 ? -rc : rc; }
    for (size_t j = 0; j < jobs.size(); j++) for (int h = 0; h < 2; h++) {
      E4 t; memcpy(t.c, T.data() + 8 * j + 4 * h, 16); t = bb::e_from_mont(t); memcpy(sums + 8 * (size_t)jobs[j].section + 4 * h, t.c, 16);
    }
  } catch (const std::exception& e) { set_last_error({ZKIR_ERR_OTHER, std::string(who) + ": " + e.what()}); return ZKIR_ERR_OTHER; }
  return ZKIR_OK;
}
}  // namespace zkir

extern "C" {

int zkir_tape_sections_stage_host(const uint32_t* const* hash_secs, const uint64_t* hash_words, const uint32_t* const* wide_secs, const uint64_t* wide_words, const uint64_t* n_real,
                                  const uint64_t* code_end, const uint32_t* alphas, const uint32_t* lambdas, uint32_t n, int32_t* hash_verdicts, int32_t* wide_verdicts, uint32_t* digests,
                                  uint32_t* sums) {
  return zkir::tape_sections_stage("zkir_tape_sections_stage_host", zkir::host_tape_many_stage(), hash_secs, hash_words, wide_secs, wide_words, n_real, code_end, alphas, lambdas, n, hash_verdicts,
                                   wide_verdicts, digests, sums);
}
int zkir_mem_sections_stage_host(const uint32_t* const* secs, const uint64_t* n_words, const uint32_t* modes, const uint64_t* code_words, const uint8_t* const* blobs, const size_t* blob_lens,
                                 const uint32_t* alphas, const uint32_t* lambdas, uint32_t n, int32_t* verdicts, uint32_t* digests, uint32_t* sums) {
  return zkir::mem_sections_stage("zkir_mem_sections_stage_host", zkir::host_mem_many_stage(), secs, n_words, modes, code_words, blobs, blob_lens, alphas, lambdas, n, verdicts, digests, sums);
}
static int mem_many_host_refuse(const char* m) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, m}); return ZKIR_ERR_ARGUMENT; }
// The list entries over host_mem_many_stage: EVERY located section goes through the list stage (no threshold), so the deferral runs on a machine without a device.
// zkir_verify_memory_last: the cells that went through it, no launches, no upload (noted behind the last front: every front's clock resets the record).
int zkir_verify_many_memory_host(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts) {
  if (!proofs || !proof_words || !verdicts) return mem_many_host_refuse("zkir_verify_many_memory_host: null proofs, proof_words or verdicts");
  if (n < 1 || n > 1024) return mem_many_host_refuse("zkir_verify_many_memory_host: n must be 1 .. 1024");
  try {
    zkir::MemManyNote note;
    const int rc = zkir::verify_many_with_mem_stage(proofs, proof_words, expects, n, zkir::host_mem_many_stage(), 0, nullptr, zkir::host_stark_query_stage(), zkir::MemManyProbe{}, verdicts, &note);
    zkir::verify_note_memory(note.cells, 0, 0);
    return rc;
  } catch (const std::exception& e) { zkir::set_last_error({ZKIR_ERR_OTHER, std::string("zkir_verify_many_memory_host: ") + e.what()}); return -ZKIR_ERR_OTHER; }
}
int zkir_verify_rate_many_memory_host(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, const uint32_t* min_queries,
                                      const uint32_t* min_pow_bits, uint32_t n, int32_t* verdicts) {
  if (!proofs || !proof_words || !verdicts) return mem_many_host_refuse("zkir_verify_rate_many_memory_host: null proofs, proof_words or verdicts");
  if (n < 1 || n > 1024) return mem_many_host_refuse("zkir_verify_rate_many_memory_host: n must be 1 .. 1024");
  try {
    zkir::MemManyNote note;
    const int rc = zkir::rate_many_with_mem_stage(proofs, proof_words, expects, min_queries, min_pow_bits, n, zkir::host_mem_many_stage(), 0, nullptr, zkir::host_pcs_many_stage(), zkir::MemManyProbe{},
                                                  verdicts, &note);
    zkir::verify_note_memory(note.cells, 0, 0);
    return rc;
  } catch (const std::exception& e) { zkir::set_last_error({ZKIR_ERR_OTHER, std::string("zkir_verify_rate_many_memory_host: ") + e.what()}); return -ZKIR_ERR_OTHER; }
}
// The *_many_memory_host entries PLUS the tape list stage over host_tape_many_stage: every located pair of tapes goes through it (no threshold).  zkir_verify_tapes_last:
// the records that went through it, no launches, no upload.
int zkir_verify_many_tapes_host(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts) {
  if (!proofs || !proof_words || !verdicts) return mem_many_host_refuse("zkir_verify_many_tapes_host: null proofs, proof_words or verdicts");
  if (n < 1 || n > 1024) return mem_many_host_refuse("zkir_verify_many_tapes_host: n must be 1 .. 1024");
  try {
    zkir::MemManyNote note; zkir::TapeManyNote tnote;
    const zkir::TapeManyStage ts = zkir::host_tape_many_stage();
    const zkir::TapeManyRun run{&ts, 0, zkir::TapeManyProbe{}, &tnote};
    const int rc = zkir::verify_many_with_mem_stage(proofs, proof_words, expects, n, zkir::host_mem_many_stage(), 0, nullptr, zkir::host_stark_query_stage(), zkir::MemManyProbe{}, verdicts, &note, &run);
    zkir::verify_note_memory(note.cells, 0, 0);
    zkir::verify_note_tapes(tnote.records, 0, 0);
    return rc;
  } catch (const std::exception& e) { zkir::set_last_error({ZKIR_ERR_OTHER, std::string("zkir_verify_many_tapes_host: ") + e.what()}); return -ZKIR_ERR_OTHER; }
}
int zkir_verify_rate_many_tapes_host(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, const uint32_t* min_queries,
                                     const uint32_t* min_pow_bits, uint32_t n, int32_t* verdicts) {
  if (!proofs || !proof_words || !verdicts) return mem_many_host_refuse("zkir_verify_rate_many_tapes_host: null proofs, proof_words or verdicts");
  if (n < 1 || n > 1024) return mem_many_host_refuse("zkir_verify_rate_many_tapes_host: n must be 1 .. 1024");
  try {
    zkir::MemManyNote note; zkir::TapeManyNote tnote;
    const zkir::TapeManyStage ts = zkir::host_tape_many_stage();
    const zkir::TapeManyRun run{&ts, 0, zkir::TapeManyProbe{}, &tnote};
    const int rc = zkir::rate_many_with_mem_stage(proofs, proof_words, expects, min_queries, min_pow_bits, n, zkir::host_mem_many_stage(), 0, nullptr, zkir::host_pcs_many_stage(), zkir::MemManyProbe{},
                                                  verdicts, &note, &run);
    zkir::verify_note_memory(note.cells, 0, 0);
    zkir::verify_note_tapes(tnote.records, 0, 0);
    return rc;
  } catch (const std::exception& e) { zkir::set_last_error({ZKIR_ERR_OTHER, std::string("zkir_verify_rate_many_tapes_host: ") + e.what()}); return -ZKIR_ERR_OTHER; }
}

}  // extern "C"
