// verify_stages.h — the three stages of a mode-4 verification that are linear in the size of the proof's tapes (the hash section and the wide section), behind one
// small interface: verify.cpp fills it with its host code (zkir_verify and its siblings: host only, no HIP call), zkir_verify_device (verify_device.inl, in the prover's
// translation unit) with the device forms.  The touched cells' three stages have an interface of their own below (MemStages); the query stages follow.  Everything else a
// verifier does (header, program, constraints at zeta, FRI) is verify.cpp's alone.
//
// A stage returns a VERDICT: 0 or the failed check's number, exactly what the host code returns at that point — or a NEGATIVE value: no verdict could be formed (a device
// failure, no memory; zkir_last_error says which), which the verifier passes through unchanged.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "hashcall.h"

namespace zkir {

struct TapeStages {
  void* self;
  // hashcall::parse_section's verdict on the hash section that starts at w (avail words to the proof's end); 0: *used = the section's length
  int (*hash_check)(void* self, const uint32_t* w, size_t avail, uint64_t n_real, uint64_t code_end, size_t* used);
  // the wide tape's record checks (57): sec = [n] + 8 n words, all inside the proof, n <= n_real (both checked by the caller)
  int (*wide_check)(void* self, const uint32_t* sec, size_t n_wide, uint64_t n_real);
  // so::observe_section's chunk digests of section `which` (0 hash, 1 wide): dg = 4 words per chunk of 512
  int (*digests)(void* self, int which, const uint32_t* sw, size_t sl, uint32_t* dg);
  // the sections' shares of the lookup table side (Montgomery E4 words); lk_m: air.h LK_ALPHA and LK_LAM, Montgomery
  int (*hash_side)(void* self, const uint32_t* lk_m, uint32_t T[4]);
  int (*wide_side)(void* self, const uint32_t* lk_m, uint32_t T[4]);
};

// what the host stages keep between their calls
struct HostTapes { std::vector<hashcall::Call> hcalls; const uint32_t* wide = nullptr; size_t n_wide = 0; };
TapeStages host_tape_stages(HostTapes* h);

int verify_with_stages(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, const TapeStages& stages);
void verify_note_device_stages(uint32_t n);                      // (zkir_verify_device) how many stages of the calling thread's last verification ran on the device

// ---- the three stages of a mode-3 / mode-4 verification that are linear in the TOUCHED-CELL section ([n] + 7 n words: air::mem_cell_code names a record's fields) ----
// A verifier handed NO MemStages runs its own inline host code (zkir_verify and every entry from before this interface: literally the code they always ran); handed one, it
// skips its cell loop, observes the stage's digests, leaves the cells' 2 n denominators out of its batch inversion and adds the stage's share of the table side.  verify.cpp
// fills the interface with host functions (what the device form leaves small sections to, and what zkir_mem_section_check_host / zkir_mem_table_side_host run),
// mem_stage.inl with the device forms.  Verdicts as above.
struct MemStages {
  void* self;
  // the section that starts at sec (avail words to the proof's end): 4 (the proof ends inside it, or its count is above 2^28), else the code of the LOWEST failing cell
  // (air::mem_cell_code: 54 / 55); 0: *used = 1 + 7 n.  code_words: the program's code size in words
  int (*check)(void* self, const uint32_t* sec, size_t avail, int mode, uint64_t code_words, size_t* used);
  // so::observe_section's chunk digests of the checked section: dg = 4 words per chunk of 512
  int (*digests)(void* self, const uint32_t* sec, size_t len, uint32_t* dg);
  // the checked section's share of the table side, Montgomery E4: per cell + 1 / (alpha - fp(cell, 0, the program image's bytes)) - 1 / (alpha - fp(cell, t_last, final
  // bytes)); lk_m: air.h LK_ALPHA and LK_LAM, Montgomery; blob: the program the proof carries (the image bytes are mem_image_cell's)
  int (*side)(void* self, const uint32_t* lk_m, const uint8_t* blob, size_t blob_len, uint32_t T[4]);
};
struct HostMem { const uint32_t* sec = nullptr; size_t n = 0; };      // what the host stages keep between their calls
MemStages host_mem_stages(HostMem* h);
// the bytes of cell `addr` in the VM's initial memory (code at 0x1000, data behind it, zero elsewhere; all zero where the blob is shorter than its header or than what the
// header claims), and the part of the blob that holds them: *image_len = code + data bytes behind blob + 32, 0 under the same rule
uint64_t mem_image_cell(const uint8_t* blob, size_t blob_len, uint64_t addr);
const uint8_t* mem_image_of(const uint8_t* blob, size_t blob_len, uint64_t* image_len);
// the byte length the proof states for the program blob it carries, cut to what the proof can hold (0: a proof too short to say): no image a memory stage is handed is longer
uint64_t stark_proof_blob_bytes(const uint32_t* proof, uint64_t proof_words);
void section_chunk_digests(const uint32_t* sw, size_t sl, uint32_t* dg);      // so::observe_section's chunk digests on host threads
// zkir_mem_table_side_host / _launch's argument checks: nullptr and lk (air::N_LK Montgomery words: alpha, lambda^0 .. lambda^11 from the canonical challenges), *n = the
// section's cells — or why the call is refused.  The cells themselves (in range, strictly increasing: check 54) are the caller's to check.
const char* mem_side_args(const uint32_t* sec, uint64_t n_words, const uint8_t* blob, size_t blob_len, const uint32_t alpha[4], const uint32_t lambda[4], const uint32_t* sum,
                          uint32_t* lk, uint64_t* n);
void verify_note_memory(uint64_t cells, uint32_t launches, uint64_t uploaded_words);      // (zkir_verify_memory_device) zkir_verify_memory_last's record

// ---- the QUERY STAGE of the commitment layer's verifiers (zkir_lowdeg_verify, zkir_eval_verify, zkir_batch_eval_verify and their *_device forms) ----
// Checks 6 .. 11 of all the queries of a 'ZKLD' / 'ZKEV' / 'ZKBE' proof.  verify.cpp's fri_part_verify hands the stage what it has CHECKED (the shape: checks 1 and 3 passed,
// so the length is exactly the header's and every word is below p) and what it has DRAWN from the transcript; verify.cpp fills the stage with its host loop (no HIP call),
// pcs_verify.inl with two kernels.  The stage returns a verdict as above: 0, 6 .. 11 (first failing check, lowest query first), or a negative value.
constexpr uint32_t PCS_MAX_MATS = 4, PCS_MAX_LAYERS = 9, PCS_MAX_SEL = 8;      // (log_M <= 27, the first layer folds once, the others LOG_ARITY = 3 times: at most 9 layers)
struct PcsQueries {
  const uint32_t* w; uint64_t len;                               // the proof
  uint32_t log_M, b, n_mats, n_layers, num_queries;
  uint32_t widths[PCS_MAX_MATS], ks[PCS_MAX_LAYERS];
  uint64_t at_roots, at_lroots, at_fin, at_queries, qsize;      // word offsets: the n_mats matrix roots, the layer roots, the final layer (4 << b values), query 0; words a query
  const uint32_t* qs;                                            // the transcript's samples, each below M / 2
  const uint32_t* betas_m;                                       // n_layers Montgomery E4
  // THE LAYER-0 RULE AS DATA.  n_points = 0: the value at a row is sum_k gamma^k row[k] over matrix 0 (the low-degree proof).  Else it is sum_i (a_i - A_i) / (z_i - x),
  // x = 31 w_M^pos, A_i = the sum over the selected pairs of point i of sum_k gamma^(e0 + k) row_mat[k].  gamma_m: n_gamma Montgomery E4 powers; z_m, a_m: Montgomery E4.
  uint32_t n_points, n_sel, n_gamma;
  const uint32_t* gamma_m;
  struct Sel { uint32_t point, mat, e0; } sel[PCS_MAX_SEL];
  uint32_t z_m[2][4], a_m[2][4];
};
struct QueryStage { void* self; int (*run)(void* self, const PcsQueries& q); };
QueryStage host_query_stage();                                   // the loop of verify.cpp
// the three verifiers, by the proof's kind (0 'ZKLD', 1 'ZKEV', 2 'ZKBE'; 'ZKLD' has one root and no points): everything but the query stage is verify.cpp's host code
int pcs_verify_with_stage(int kind, const uint32_t* proof, uint64_t n_words, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals, const QueryStage& stage);
// a 'ZKSR' proof (zkir_verify_rate): verify.cpp's STARK front and constraint check on the host, the embedded evaluation proof's query stage behind `stage`; a mode-4
// proof's three tape stages behind `tapes` (NULL: the host forms), a mode-3 / mode-4 proof's memory stages behind `mem` (NULL: the verifier's inline host code)
int rate_verify_with_stage(const uint32_t* proof, uint64_t n_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits, const QueryStage& stage,
                           const TapeStages* tapes = nullptr, const MemStages* mem = nullptr);

// ---- the query stage over a LIST of proofs (zkir_verify_rate_chain, zkir_verify_rate_many_device, zkir_pcs_verify_many_device and their siblings) ----
// A PcsCollected OWNS what a PcsQueries points at except the proof (samples, gamma table, betas): pcs_collect_stage is a QueryStage that copies the description it is handed
// into `out` and answers 0, so a caller runs the host fronts of several proofs first — proof after proof, each up to the point where its queries would start — and then ONE
// run of a PcsManyStage over all it has collected: codes[i] = 0 or 6 .. 11, proof i's first failing check, lowest query first.  run returns 0, or a negative value (no verdict
// for any of them).  verify.cpp fills the stage with its host loop (no HIP call), pcs_verify_many.inl with two kernels that serve proofs whose shapes differ.
struct PcsCollected {
  PcsQueries q{};
  std::vector<uint32_t> qs, betas_m, gamma_m;
  bool filled = false;                                           // the front reached its queries (a front that fails earlier never calls the stage)
};
QueryStage pcs_collect_stage(PcsCollected* out);
struct PcsManyStage { void* self; int (*run)(void* self, const PcsCollected* list, uint32_t n, int* codes); };
PcsManyStage host_pcs_many_stage();
// zkir_verify_rate_segment: rate_verify_with_stage without check 7 (a mode >= 3 proof is never a segment: 2); states_out: NULL or 2 x 68 words (first | last), counters_out:
// NULL or the four counter words — both written as soon as the header is read, whatever the verdict
int rate_segment_verify_with_stage(const uint32_t* proof, uint64_t n_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits, const QueryStage& stage,
                                   uint32_t* states_out, uint32_t* counters_out);
// zkir_verify_rate_chain with the segments' queries in ONE run of `stage` (a chain of one mode >= 3 proof is the caller's: it is a whole run)
int rate_chain_with_stage(const uint32_t* const* proofs, const uint64_t* proof_words, uint32_t n_segments, const zkir_public_inputs* expect, uint32_t min_queries,
                          uint32_t min_pow_bits, const PcsManyStage& stage);

// ---- the QUERY STAGE of the mixed-height verifier (zkir_mixed_eval_verify and zkir_mixed_eval_verify_device: a 'ZKMH' proof) ----
// Checks 6 .. 11 of all the queries, handed over as above: after checks 1 .. 5, 12 and 13 and the sampling.  The proof has ONE FRI and one layer-0 rule per GROUP: g[h] is a
// PcsQueries of which only the rule counts (log_M = log M_h, n_mats, widths, n_points, n_sel, sel with e0 counted from the proof's first exponent, z_m, a_m, and the gamma
// table all groups share); group h's first matrix is matrix first_mat[h] of the proof's roots at at_roots.  A query holds q, group 0's records at q and q + M_0/2, each lower
// group's records at q mod M_h, then the layers; the layer of size M_h is the fold of the layer before it plus F_h (g[h]'s rule at row q mod M_h).
// The mixed schedule (fri_mixed_schedule) is longer than the single-height one: over every pair and triple of heights and every b it has at most 10 layers
// (log_ns = (26, 3), b = 1: 1,3,3,3,3,3,3,3,1,1), so this path has its own bounds; the hash jobs of one query are at most 2*4 (group 0) + 2*4 (two lower groups) + 10.
constexpr uint32_t MIXED_MAX_GROUPS = 3, MIXED_MAX_LAYERS = 10, MIXED_MAX_SLOTS = 2 * PCS_MAX_MATS + (MIXED_MAX_GROUPS - 1) * PCS_MAX_MATS + MIXED_MAX_LAYERS;      // 26
struct MixedQueries {
  const uint32_t* w; uint64_t len;                               // the proof
  uint32_t n_groups, b, n_layers, num_queries;
  PcsQueries g[MIXED_MAX_GROUPS];
  uint32_t first_mat[MIXED_MAX_GROUPS];
  uint32_t ks[MIXED_MAX_LAYERS];
  uint64_t at_roots, at_lroots, at_fin, at_queries, qsize;      // as in PcsQueries; at_roots: the first of all the groups' roots
  const uint32_t* qs;                                            // the transcript's samples, each below M_0 / 2
  const uint32_t* betas_m;                                       // n_layers Montgomery E4
};
struct MixedQueryStage { void* self; int (*run)(void* self, const MixedQueries& q); };
MixedQueryStage host_mixed_query_stage();                        // the loop of verify.cpp
int mixed_eval_verify_with_stage(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals, const MixedQueryStage& stage);

// ---- the QUERY STAGE of the STARK verifier (zkir_verify and its siblings; zkir_verify_on_device, zkir_verify_many_on_device, zkir_verify_chain_on_device) ----
// Checks 20 .. 27 (and 4: a query cut by the proof's end) of all the queries of a ZKIR-STARK proof, handed over after check 11: the header, the word range (every word from
// word 2 on is below p) and the whole transcript are verify.cpp's host code.  A STARK query is the commitment layer's at b = 1 — three matrices (main WM, aux WA, quotient 4)
// under the three roots at at_roots, opened at q and q + N, then the FRI layers — and its layer-0 value (A - a0) / (x - zeta) + (B - b0) / (x - zeta w) is PcsQueries' rule
// with z = (zeta, zeta w), a = (a0, b0) and the selections (0, main, 0), (0, aux, WM), (0, quot, 2 WT), (1, main, WT), (1, aux, WT + WM), WT = WM + WA.
// The proof's LENGTH is not checked before the queries: query t lies at at_queries + t qsize and may run past len (codes 20 / 4).  Check 30 stays with the caller.
// The stage takes a LIST (a chain's segments, a service's proofs): codes[i] = 0 or proof i's first failing check, lowest query first, in the order 20, 4, 21 (row q, then
// q + N), 27, 22, per layer j 23 then 24 (j = 0) / 25 (j > 0), 26.  run returns 0, or a negative value (no verdict for any of them).
// A StarkQueries OWNS what it points to except the proof: a caller collects several before it runs the stage.
struct StarkQueries {
  const uint32_t* w = nullptr; uint64_t len = 0;                 // the proof (borrowed)
  uint32_t log_n = 0, mode = 0, WM = 0, WA = 0, num_queries = 0, n_layers = 0;
  uint32_t ks[PCS_MAX_LAYERS] = {0};
  uint64_t at_roots = 0, at_lroots = 0, at_fin = 0, at_queries = 0, qsize = 0;      // word offsets: the trace, aux and quotient roots (12 words), the layer roots, the final layer (8 values), query 0
  std::vector<uint32_t> qs;                                      // the transcript's samples, each below N
  std::vector<uint32_t> betas_m, gamma_m;                        // n_layers and 2 WT + 4 Montgomery E4
  uint32_t zeta_m[4] = {0}, zeta_w_m[4] = {0}, a0_m[4] = {0}, b0_m[4] = {0};
};
struct StarkQueryStage { void* self; int (*run)(void* self, const StarkQueries* list, uint32_t n, int* codes); };
StarkQueryStage host_stark_query_stage();                        // the loop of verify.cpp: host threads, ZKIR_VERIFY_THREADS
// verify_impl up to check 11 (whole runs: check 7 included; a segment: whole_run = false, its boundary states and counters out): 0 = *out is filled and the queries are the
// caller's (then check 30: stark_length_check), else the failed check.  stages: nullable (the host tape stages); mem: nullable (the inline host code).
// out == NULL: the whole verification, queries and check 30 included (zkir_verify's verdict).
int stark_verify_collect(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, bool whole_run, const TapeStages* stages, StarkQueries* out,
                         const MemStages* mem = nullptr);
int stark_host_queries_from(const StarkQueries& q, uint32_t first);      // the host loop over queries first .. num_queries - 1 (the device stage: the queries a short proof cuts)
void verify_note_queries(uint64_t hash_jobs, uint64_t value_jobs, uint32_t launches, uint64_t uploaded_words);      // (the *_on_device entries) zkir_verify_queries_last's record
inline int stark_length_check(const StarkQueries& q) { return q.at_queries + (uint64_t)q.num_queries * q.qsize != q.len ? 30 : 0; }
// zkir_verify_chain with the segments' queries in ONE run of `stage` (a chain of one mode >= 3 proof is the caller's: it is a whole run)
int verify_chain_with_stage(const uint32_t* const* proofs, const uint64_t* proof_words, uint32_t n_segments, const zkir_public_inputs* expect, const StarkQueryStage& stage);

}  // namespace zkir
