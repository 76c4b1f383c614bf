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

struct MemDeferred;
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
  // (the list form below: TapeManyStage) NULL for every stage from before it: the sides run where they always ran.  Else, where defer->tapes_armed is set when the front
  // reaches the table side, the front calls NEITHER side: it forms T without the tapes' shares, keeps check 10 in *defer and goes on as if that check held.  May be the
  // record MemStages::defer points at (a proof defers its cells, its tapes or both; two DIFFERENT armed records: the tapes' one is ignored)
  MemDeferred* defer = nullptr;
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
struct MemDeferred;
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
  // (the list form below) NULL for every stage from before it: side runs where it always ran.  Else, where defer->armed is set when the front reaches the table side, the
  // front does NOT call side: it forms T without the cells' share, keeps check 10 in *defer and goes on as if that check held
  MemDeferred* defer = nullptr;
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
void verify_note_tapes(uint64_t records, uint32_t launches, uint64_t uploaded_words);      // (the *_many_tapes_* entries) zkir_verify_tapes_last's record
void verify_note_memory(uint64_t cells, uint32_t launches, uint64_t uploaded_words);      // (zkir_verify_memory_device) zkir_verify_memory_last's record

// ---- the memory stages over a LIST of proofs (zkir_verify_many_memory_device, zkir_verify_rate_many_memory_device and their *_host forms) ----
// check and digests depend on the proof's words alone, so a list stage answers them for every proof BEFORE any front runs (prepare).  side needs the lookup challenges,
// which the transcript yields only behind the digests — but its result enters LK_TN alone, which nothing but check 10 reads and no challenge, grinding or sample depends
// on.  So a front whose check was answered by the list DEFERS check 10: it keeps in a MemDeferred, BY VALUE, what the check reads, and goes on as if it held (check 11,
// the sampling, the collecting query stage).  After the last front ONE side call serves every proof that deferred; the caller completes LK_TN = (T + T_mem) / N and
// evaluates the kept check (mem_deferred_check).  A proof whose deferred check fails has verdict 10 whatever its front answered afterwards (every check before 10 had
// passed, 10 precedes all later ones); every other proof keeps its front's verdict.
struct MemDeferred {
  bool armed = false;                                            // (the check callback) this proof's table side is deferred
  bool tapes_armed = false;                                      // (a list entry's tape callbacks) the hash and wide tapes' shares are deferred
  bool filled = false;                                           // (the front) check 10 was reached: everything below is set
  int mode = 0, log_n = 0, WM = 0; uint64_t n_real = 0;
  std::vector<uint32_t> ev;                                      // Montgomery E4 words: main | aux at zeta, the same at zeta w, the quotient's four
  std::vector<uint32_t> lk_m;                                    // air.h LK_*; LK_TN is not final
  std::vector<uint32_t> states;                                  // the boundary states, first | last, canonical
  uint32_t cnt[4] = {0, 0, 0, 0}, alpha_m[4] = {0, 0, 0, 0}, zeta_m[4] = {0, 0, 0, 0};
  uint32_t T_m[4] = {0, 0, 0, 0};                                // the table side WITHOUT the cells' share, Montgomery E4
  std::vector<uint8_t> blob;                                     // the program the proof carries (the side's image bytes)
};
bool mem_deferred_check(const MemDeferred& d, const uint32_t T_mem[4]);      // check 10 with LK_TN = (T + T_mem) / N
// A LOCATED section: sec[0] = n <= 2^28 and 1 + 7 n words lie at sec inside the proof (the list entries send no empty one).  Its chunk digests are 4 mem_section_chunks(n) words.
struct MemSection { const uint32_t* sec; uint64_t n; int mode; uint64_t code_words; };
inline uint64_t mem_section_chunks(uint64_t n) { return (1 + 7 * n + 511) / 512; }
struct MemSideJob { uint32_t section; const uint32_t* lk_m; const uint8_t* blob; size_t blob_len; };      // section: an index into the list prepare was handed
struct MemManyStage {
  void* self;
  // per section MemStages::check's verdict (0 / 54 / 55) and, where it is 0, MemStages::digests' words at digests + 4 (the chunks of the sections before it)
  int (*prepare)(void* self, const MemSection* list, uint32_t n, int* verdicts, uint32_t* digests);
  // per job MemStages::side's sum (sums + 4 job); list: what prepare was handed, every job's section had verdict 0 and its words are below p
  int (*side)(void* self, const MemSection* list, const MemSideJob* jobs, uint32_t n_jobs, uint32_t* sums);
  void (*done)(void* self);                                      // nullable: the stage keeps nothing of the list from here on (called once, before the query stage)
};
MemManyStage host_mem_many_stage();                              // loops over the host stage functions
// Where a proof's touched-cell section starts, by the front's own rules (magic, mode, header, the blob's length word, the code size in blob bytes 16 .. 19, the I/O
// section): at = its word offset, avail = the words behind it.  A ROUTING AID ONLY: the list entries compare what the front hands their check callback with this and
// fall back to the host stage on any difference, so a wrong answer can choose the slower route and nothing else.
struct MemLocated { bool ok = false; uint64_t at = 0, avail = 0; int mode = 0; uint64_t code_words = 0; };
MemLocated mem_section_locate(const uint32_t* proof, uint64_t proof_words, bool rate);
// a mode-4 proof's tape stages for front i (NULL: the host forms): begin before the front, end(rc) behind it (what it answers is the front's result)
struct TapeStagesFor { void* self; const TapeStages* (*begin)(void* self, uint32_t i); int (*end)(void* self, int rc); };
struct MemManyProbe { uint32_t what = 0, index = 0; };           // (zkir_verify_many_memory_probe) what = 1: + 1 on proof index's T_mem before its deferred check
struct MemManyNote { uint64_t cells = 0; uint32_t sections = 0, deferred = 0; };      // what went through the list stage (all zero: the batch stayed with the inline host code)
// zkir_mem_sections_stage_host / _launch: the list stage on its own over n whole sections ([n_i] + 7 n_i words each, n_i = 0 included) with their modes, code sizes, blobs and
// canonical challenges: per section the verdict, the chunk digests (zero where the verdict is not 0) and the canonical sum (likewise)
int mem_sections_stage(const char* who, const MemManyStage& st, const uint32_t* const* secs, const uint64_t* n_words, const uint32_t* modes, const uint64_t* code_words, const uint8_t* const* blobs,
                       const size_t* blob_lens, const uint32_t* alphas, const uint32_t* lambdas, uint32_t n, int32_t* verdicts, uint32_t* digests, uint32_t* sums);

// ---- a mode-4 proof's TAPE stages over a LIST of proofs (zkir_verify_many_tapes_device, zkir_verify_rate_many_tapes_device and their *_host forms) ----
// The same key as above.  hash_check, wide_check and both sections' digests depend on the proof's words alone (plus n_real and the code's end from the header and the blob),
// and so do the bytes every hash call wrote: a list stage answers them for every proof BEFORE any front runs (prepare).  hash_side and wide_side need the lookup challenges,
// but their sums enter T, then LK_TN, which check 10 alone reads: a front whose tape checks were answered by the list DEFERS check 10 (TapeStages::defer, tapes_armed) and
// goes on; after the last front ONE sides call serves every proof that deferred, and mem_deferred_check is handed the sum of ALL the deferred shares (cells + hash + wide).
//
// A LOCATED pair of tapes.  hash: the hash section's start, avail: the words from there to the proof's end (>= 1).  The records are placed by hashcall::n_cells_of of their
// own fields, never by a count word: n_full records of hash[0] lie in the proof whole and take hash_words words with the count word; whole: the walk placed all hash[0] of
// them.  wide: NULL, or the wide section ([n_wide] + 8 n_wide words) at hash + hash_words, where the hash section is whole, n_wide <= n_real and those words lie in the proof.
struct TapeSection {
  const uint32_t* hash; uint64_t avail;
  uint64_t n_full, hash_words; bool whole;
  const uint32_t* wide; uint64_t n_wide;
  uint64_t n_real, code_end;
};
// hash_tape_walk's rule (tape_table.inl) without the device's needs.  prefix: NULL, or min(w[0], avail / 8) + 1 entries: how many cells the records before record k hold.
// header_only: record n_full's eight header words lie in the buffer, its cells do not.
struct TapeExtent { uint64_t n_full = 0, cells = 0, used = 1; bool whole = false, header_only = false; };
inline TapeExtent tape_section_walk(const uint32_t* w, uint64_t avail, uint64_t* prefix) {
  TapeExtent t;
  const uint64_t nh = w[0];
  uint64_t q = 1;
  t.whole = true;
  for (uint64_t k = 0; k < nh; k++) {
    if (q + 8 > avail) { t.whole = false; break; }
    const uint32_t* c = w + q;
    if (prefix) prefix[k] = t.cells;
    const uint64_t n = hashcall::n_cells_of((uint64_t)c[1] | ((uint64_t)c[2] << 20), c[3], (uint64_t)c[4] | ((uint64_t)c[5] << 20));
    if (q + 8 + 5 * n > avail) { t.whole = false; t.header_only = true; break; }
    q += 8 + 5 * n; t.cells += n; t.n_full++;
  }
  if (prefix && t.whole) prefix[nh] = t.cells;
  t.used = q;
  return t;
}
// a section's chunk digests in prepare's answer: the hash section's (only where it is whole: hash_words is its length if its check passes), then the wide section's
inline uint64_t tape_section_chunks(const TapeSection& S, int which) { return which ? (S.wide ? (1 + 8 * S.n_wide + 511) / 512 : 0) : (S.whole ? (S.hash_words + 511) / 512 : 0); }
// Where a mode-4 proof's tapes lie: mem_section_locate's result (loc), then 1 + 7 n words of touched cells.  ok = false: not mode 4, or the proof ends before the hash
// section's count word.  A ROUTING AID ONLY, as mem_section_locate is: the list entries compare what the front hands their callbacks with this (pointer, available words,
// n_real, code_end, n_wide) and fall back to the host stage on any difference.
struct TapeLocated { bool ok = false; TapeSection sec{}; };
TapeLocated tape_sections_locate(const uint32_t* proof, uint64_t proof_words, const MemLocated& loc);
struct TapeSideJob { uint32_t section; const uint32_t* lk_m; bool hash, wide; };      // section: an index into the list prepare was handed; which of the two sums are wanted
struct TapeManyStage {
  void* self;
  // per section TapeStages::hash_check's verdict and *used (used[i], where the verdict is 0), TapeStages::wide_check's verdict (wide_verdicts[i]; 0 where wide is NULL) and
  // TapeStages::digests' words of both sections at digests + 4 (the chunks of the sections before it: tape_section_chunks(S, 0) + tape_section_chunks(S, 1) each)
  int (*prepare)(void* self, const TapeSection* list, uint32_t n, int* hash_verdicts, uint64_t* used, int* wide_verdicts, uint32_t* digests);
  // per job TapeStages::hash_side's sum at sums + 8 job and wide_side's at sums + 8 job + 4 (zero where not wanted); list: what prepare was handed, a wanted side's check
  // had verdict 0 and the proof's words are below p
  int (*sides)(void* self, const TapeSection* list, const TapeSideJob* jobs, uint32_t n_jobs, uint32_t* sums);
  void (*done)(void* self);                                      // nullable, as MemManyStage::done
};
TapeManyStage host_tape_many_stage();                            // loops over the host stage functions
struct TapeManyProbe { uint32_t what = 0, index = 0; };          // (zkir_verify_many_tapes_probe) what = 1: + 1 on proof index's hash share, 2: on its wide share, before its deferred check
struct TapeManyNote { uint64_t records = 0; uint32_t sections = 0, deferred = 0; };      // what went through the tape list stage (all zero: every proof kept its own tape stages)
// the tape list stage of a many-proof call: the located tapes go through `stage` where their calls plus wide records reach min_records (and there is one at all)
struct TapeManyRun { const TapeManyStage* stage; uint64_t min_records; TapeManyProbe probe; TapeManyNote* note; };
// zkir_tape_sections_stage_host / _launch: the list stage on its own over n whole hash sections (hash_words[i] words each: [0] included) and wide sections ([n] + 8 n
// words) with their n_real, code_end and canonical challenges: per section both verdicts, the chunk digests (hash: ceil(hash_words / 512), then wide: ceil(wide_words / 512);
// zero where the verdict is not 0) and the two canonical sums (sums + 8 i, + 4; zero unless BOTH verdicts are 0)
int tape_sections_stage(const char* who, const TapeManyStage& st, const uint32_t* const* hash_secs, const uint64_t* hash_words, const uint32_t* const* wide_secs, const uint64_t* wide_words,
                        const uint64_t* n_real, const uint64_t* code_end, const uint32_t* alphas, const uint32_t* lambdas, uint32_t n, int32_t* hash_verdicts, int32_t* wide_verdicts,
                        uint32_t* digests, uint32_t* sums);
struct PcsManyStage;
struct StarkQueryStage;
// zkir_verify / zkir_verify_rate of n proofs (modes mixed), the memory stages through `mem` where the located sections' total cells reach min_cells, the queries through ONE
// run of `queries`.  Host only: whatever touches a device is behind the three interfaces.  0, or a negative value (no verdict for any of them).
// tape_run: NULL (every mode-4 front has its own tape stages: `tapes`), or the tape list stage around the same pass of fronts.  Where the tape batch goes through it, a
// mode-4 proof it does not serve (not located, no record) runs the host tape stages; where it does not (below min_records), every front keeps `tapes`.
int verify_many_with_mem_stage(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, const MemManyStage& mem,
                               uint64_t min_cells, const TapeStagesFor* tapes, const StarkQueryStage& queries, const MemManyProbe& probe, int32_t* verdicts, MemManyNote* note,
                               const TapeManyRun* tape_run = nullptr);
int rate_many_with_mem_stage(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, const uint32_t* min_queries,
                             const uint32_t* min_pow_bits, uint32_t n, const MemManyStage& mem, uint64_t min_cells, const TapeStagesFor* tapes, const PcsManyStage& queries,
                             const MemManyProbe& probe, int32_t* verdicts, MemManyNote* note, const TapeManyRun* tape_run = nullptr);

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
