/* zkir_amd_experimental.h — measurement probes and kernel experiments exported by libzkir_amd.so that are NOT part of the drop-in boundary (include/zkir_amd.h):
 * nothing in the reference has a counterpart, no caller of the boundary needs them, and they may change or disappear.  Used by bench.py (the peaks) and scripts/ (the experiments). */
#ifndef ZKIR_AMD_EXPERIMENTAL_H
#define ZKIR_AMD_EXPERIMENTAL_H
#include "zkir_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* diagnostic: measured peak rate (per second) of independent Montgomery multiplications on the current device — the integer-ALU
 * roofline the Poseidon2 kernels are priced against (they are ALU-bound, not HBM- or MFMA-bound) */
double zkir_modmul_peak_per_s(void* hip_stream);
/* diagnostic: achieved HBM bandwidth (GB/s, read + write bytes) of a 16-byte-per-lane grid-stride device-to-device copy of `bytes` bytes (rounded down to 16 KiB; two scratch
 * buffers are allocated and freed): the measured copy peak the HBM-bound stages are held against next to the nominal 8 TB/s (MI355X_MICROARCH.md: ~6.3 TB/s for this copy) */
double zkir_hbm_copy_peak_gbs(uint64_t bytes, void* hip_stream);
/* EXPERIMENT (profiles/HISTORY.md, round 4): zkir_main_trace_launch + zkir_lde_launch (default VM mode) with the first two blocks of the main trace never written: the
 * extension's first inverse pass generates them from the trace.  m = scratch for the main-trace matrix (as zkir_main_trace_launch's out), out = the LDE.
 * Same output as the two calls; ZKIR_ERR_ARGUMENT where it does not apply (padded log2 rows < 20 or = 21).  Measured in profiles/r04*_fused01*. */
int zkir_commit_fused01_launch(const zkir_stark_ctx* ctx, const zkir_trace_columns* trace, uint64_t n_real, uint32_t* m, uint32_t width, uint32_t* out, void* hip_stream);
/* EXPERIMENT: one strided NTT pass (stage 0 of the inverse transform over 2^log_n rows, or stage 11 of the forward one over 2^(log_n + 1)) with tile geometry `variant`
 * (ntt.hip: strided_variant_run lists them) over `width` columns: for timing the tilings side by side (scripts/time_ntt_tiles.py); the data is left partially transformed. */
int zkir_ntt_strided_variant_launch(const zkir_stark_ctx* ctx, uint32_t* data, uint32_t width, int variant, int forward, void* hip_stream);

/* EXPERIMENT (round 6; profiles/r06_overlap_variants.txt): zkir_lde_launch + zkir_merkle_commit_launch of a canonical matrix with the leaf sponge absorbed block-group-wise on
 * the context's second stream while the next group of `group` B8 blocks is extended on `hip_stream` (a 12-word sponge state per leaf travels through HBM between groups).
 * in / out as zkir_lde_launch, tree as zkir_merkle_commit_launch; same output as the two calls. */
int zkir_commit_overlapped_launch(const zkir_stark_ctx* ctx, uint32_t* in, uint32_t width, uint32_t* out, uint32_t* tree, uint32_t group, void* hip_stream);

/* MEASUREMENT: zkir_lowdeg_prove with the device time (ms, HIP events) of its four stages: combine | FRI commit phase | grinding | query section. */
int zkir_lowdeg_prove_stages(zkir_stark_ctx* ctx, const uint32_t* lde_mat, uint32_t width, const uint32_t* tree, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host,
                             uint64_t cap_words, uint64_t* n_words, float stage_ms[4], void* hip_stream);
/* TEST / MEASUREMENT: the combine kernel of zkir_lowdeg_prove alone for a GIVEN canonical gamma: cw[t M + j] = coordinate t of sum_k gamma^k col_k(row j), M = N << log_blowup
 * rows of the context.  gpow_scratch: DEVICE buffer of 32 ceil(width / 8) words for the gamma powers, uploaded with a synchronous copy. */
int zkir_lowdeg_combine_launch(const zkir_stark_ctx* ctx, const uint32_t* lde_mat, uint32_t width, const uint32_t gamma[4], uint32_t* gpow_scratch, uint32_t* cw, void* hip_stream);

/* MEASUREMENT: zkir_eval_prove with the device time (ms, HIP events) of its six stages: weights | evaluations | quotient | FRI commit phase | grinding | query section. */
int zkir_eval_prove_stages(zkir_stark_ctx* ctx, const uint32_t* lde_mat, uint32_t width, const uint32_t* tree, const uint32_t* points, uint32_t n_points, uint32_t num_queries,
                           uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words, float stage_ms[6], void* hip_stream);
/* TEST / MEASUREMENT: the evaluations of zkir_eval_prove alone (weights, dot and sum kernels) for GIVEN points (HOST, canonical, as zkir_eval_prove takes them):
 * evals = n_points x width canonical E4 words on the DEVICE, point-major.  scratch: DEVICE buffer of zkir_eval_at_scratch_words(log_n, width, n_points) words. */
uint64_t zkir_eval_at_scratch_words(uint32_t log_n, uint32_t width, uint32_t n_points);
int zkir_eval_at_launch(const zkir_stark_ctx* ctx, const uint32_t* lde_mat, uint32_t width, const uint32_t* points, uint32_t n_points, uint32_t* scratch, uint32_t* evals, void* hip_stream);
/* TEST / MEASUREMENT: the codeword of zkir_eval_prove alone (inverse table and quotient kernel) for GIVEN gamma, points and evaluations (HOST, canonical):
 * cw[t M + j] = coordinate t of F at row j, M = N << log_blowup.  scratch: DEVICE buffer of zkir_eval_quotient_scratch_words(log_n + log_blowup, width, n_points) words;
 * the gamma table is uploaded with a synchronous copy. */
uint64_t zkir_eval_quotient_scratch_words(uint32_t log_m, uint32_t width, uint32_t n_points);
int zkir_eval_quotient_launch(const zkir_stark_ctx* ctx, const uint32_t* lde_mat, uint32_t width, const uint32_t gamma[4], const uint32_t* points, uint32_t n_points,
                              const uint32_t* evals, uint32_t* scratch, uint32_t* cw, void* hip_stream);

/* TEST: the main, aux and quotient LDE matrices of the context's last zkir_prove_rate proof, copied to the HOST from where they still lie in its workspace: B8 layout
 * ([blocks][M][8] words, M = N << log_blowup), canonical; the quotient's one block holds its 4 columns and 4 zero columns.  A NULL buffer is skipped; widths (may be NULL)
 * gets the three widths, *rows (may be NULL) gets M.  ZKIR_ERR_ARGUMENT once any other proof has used the context's workspace (or before the first). */
int zkir_prove_rate_last_matrices(const zkir_stark_ctx* ctx, uint32_t* main_host, uint32_t* aux_host, uint32_t* quotient_host, uint32_t widths[3], uint64_t* rows);

/* MEASUREMENT: zkir_batch_eval_prove with the device time (ms, HIP events) of its six stages: weights | evaluations | quotient | FRI commit phase | grinding | query section. */
int zkir_batch_eval_prove_stages(zkir_stark_ctx* ctx, uint32_t n_mats, const uint32_t* const* lde_mats, const uint32_t* widths, const uint32_t* const* trees, const uint32_t* masks,
                                 const uint32_t* points, uint32_t n_points, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words,
                                 float stage_ms[6], void* hip_stream);
/* TEST / MEASUREMENT: the codeword of zkir_batch_eval_prove alone (inverse table and batch_quotient_kernel) for GIVEN gamma, points and evaluations (HOST, canonical; evals in
 * the proof's exponent order, 4 words each): cw[t M + j] = coordinate t of F at row j.  scratch: DEVICE buffer of zkir_batch_eval_quotient_scratch_words words; the gamma
 * table is uploaded with a synchronous copy. */
uint64_t zkir_batch_eval_quotient_scratch_words(uint32_t log_m, uint32_t n_mats, const uint32_t* widths, uint32_t n_points);
int zkir_batch_eval_quotient_launch(const zkir_stark_ctx* ctx, uint32_t n_mats, const uint32_t* const* lde_mats, const uint32_t* widths, const uint32_t* masks, const uint32_t gamma[4],
                                    const uint32_t* points, uint32_t n_points, const uint32_t* evals, uint32_t* scratch, uint32_t* cw, void* hip_stream);

/* MEASUREMENT: zkir_mixed_eval_prove with the device time (ms, HIP events) of its six stages, each over all the groups: weights | evaluations | quotients | FRI commit phase |
 * grinding | query section. */
int zkir_mixed_eval_prove_stages(zkir_stark_ctx* const* ctxs, uint32_t n_groups, const uint32_t* n_mats, const uint32_t* const* lde_mats, const uint32_t* widths,
                                 const uint32_t* const* trees, const uint32_t* masks, const uint32_t* points, const uint32_t* n_points, uint32_t num_queries, uint32_t pow_bits,
                                 uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words, float stage_ms[6], void* hip_stream);
/* TEST / MEASUREMENT: the FRI fold kernel alone.  layer: DEVICE, the 2^log_m values of a layer of the context's FRI, layer[t m + j] = coordinate t of value j, canonical
 * (k <= log_m <= log_n + log_blowup; the layer's coset shift is 31^(2^(log_n + log_blowup - log_m))).  It is folded k (1 .. 3) times with beta (HOST, canonical E4), beta^2,
 * beta^4 into out[t g + i], g = m >> k.  addend: NULL, or DEVICE 4 g words added by index (out = fold + addend: the add form zkir_mixed_eval_prove uses at a layer of a lower
 * group's size).  Synchronises the stream. */
int zkir_fri_fold_launch(const zkir_stark_ctx* ctx, const uint32_t* layer, uint32_t log_m, uint32_t k, const uint32_t beta[4], const uint32_t* addend, uint32_t* out, void* hip_stream);

/* DIAGNOSTIC: what the calling thread's last zkir_lowdeg_verify_device / zkir_eval_verify_device / zkir_batch_eval_verify_device call launched: hash_jobs = num_queries x
 * (2 n_mats + n_layers) leaf-and-path jobs, value_jobs = num_queries x (2 + n_layers) (two layer-0 values and one fold a layer); (0, 0) when the call returned before its
 * query stage (verdicts 1 - 5, 12, 13).  After zkir_mixed_eval_verify_device: hash_jobs = num_queries x (2 n_mats_0 + the lower groups' n_mats + n_layers), value_jobs =
 * num_queries x (2 + (n_groups - 1) + n_layers) (one more wave per lower group: its F_h).  Either pointer may be NULL. */
int zkir_pcs_verify_last_jobs(uint64_t* hash_jobs, uint64_t* value_jobs);
/* MEASUREMENT: with ZKIR_PCS_VERIFY_TIMES set in the environment the device query stage synchronises after its upload and after its kernels; this reports the host clocks
 * (ms) of the calling thread's last such call: upload | kernels | download.  Zeros without the variable or before the stage. */
int zkir_pcs_verify_last_stage_ms(double ms[3]);
/* MEASUREMENT: the same for the STARK verifier's device query stage (zkir_verify_on_device, zkir_verify_many_on_device, zkir_verify_chain_on_device), under
 * ZKIR_VERIFY_QUERIES_TIMES: upload | kernels | download of the calling thread's last stage run. */
int zkir_verify_queries_last_stage_ms(double ms[3]);
/* TEST HOOK: the STARK verifier's query stage on PERTURBED DRAWS.  The roots are in the transcript, so a proof mutated by one word fails a hash check (21 / 22 / 23 / 27) or
 * grinding before it can reach checks 24, 25 or 26; perturbing what the VERIFIER drew reaches them with an honest proof.  Runs zkir_verify's host part (no expectation; a
 * failing one is returned as it is), perturbs, then runs the host form of the stage (device = 0: no HIP call) or the device form, then check 30.  what: 0 nothing, 1 a0 + 1,
 * 2 b0 + 1, 3 zeta + 1, 4 betas[index] + 1, 5 qs[index] ^= 1.  Returns the verdict; negative: -ZKIR_ERR_ARGUMENT (no such what / layer / query) or a device failure. */
int zkir_stark_query_stage_probe(const uint32_t* proof, uint64_t proof_words, uint32_t what, uint32_t index, int device, void* hip_stream);
/* THE MEMORY STAGES OVER A LIST OF PROOFS (zkir_verify_many_memory_device, zkir_verify_rate_many_memory_device; csrc/verify_stages.h: MemManyStage).
 * _host: the same orchestration (section locator, phase A, deferring fronts, phase B, resolution, one query stage) over the HOST list stage and the host query stage, no HIP
 * call; EVERY located section goes through the list stage (no threshold).  zkir_verify_memory_last reports the cells that did, no launches, no upload. */
int zkir_verify_many_memory_host(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts);
int zkir_verify_rate_many_memory_host(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, const uint32_t* min_queries,
                                      const uint32_t* min_pow_bits, uint32_t n, int32_t* verdicts);
/* The list stage on its own: n = 1 .. 1024 whole sections (secs[i]: [n_i] + 7 n_i = n_words[i] words, n_i = 0 included), modes[i] 3 / 4, code_words[i], the program blobs
 * and per section four canonical words of alpha and lambda (alphas, lambdas: 4 n words).  verdicts[i] = 0 / 54 / 55 as zkir_mem_section_check_*; digests: 4 words per
 * chunk of 512, section after section (ceil(n_words[i] / 512) chunks each; zero where the verdict is not 0); sums: 4 canonical words per section as
 * zkir_mem_table_side_* (zero where the verdict is not 0).  _launch: three launches for all sections (mem_stage_many.inl); _host: verify.cpp's code. */
int zkir_mem_sections_stage_host(const uint32_t* const* secs, const uint64_t* n_words, const uint32_t* modes, const uint64_t* code_words, const uint8_t* const* blobs, const size_t* blob_lens,
                                 const uint32_t* alphas, const uint32_t* lambdas, uint32_t n, int32_t* verdicts, uint32_t* digests, uint32_t* sums);
int zkir_mem_sections_stage_launch(const uint32_t* const* secs, const uint64_t* n_words, const uint32_t* modes, const uint64_t* code_words, const uint8_t* const* blobs, const size_t* blob_lens,
                                   const uint32_t* alphas, const uint32_t* lambdas, uint32_t n, int32_t* verdicts, uint32_t* digests, uint32_t* sums, void* hip_stream);
/* TEST HOOK: zkir_verify_many_memory_host (device = 0) / _device (device != 0, with every section on the device whatever the threshold) with a PERTURBED share.  An honest
 * proof's cells cannot make check 10 fail alone where grinding precedes it; what = 1 adds one to proof `index`'s T_mem before its deferred check, so that proof answers 10
 * if (and only if) its front deferred — whatever it answered afterwards.  what = 0: nothing. */
int zkir_verify_many_memory_probe(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts, uint32_t what,
                                  uint32_t index, int device, void* hip_stream);
/* THE TAPE STAGES OVER A LIST OF PROOFS (zkir_verify_many_tapes_device, zkir_verify_rate_many_tapes_device; csrc/verify_stages.h: TapeManyStage).
 * _host: the whole deferral (both locators, phase A, deferring fronts, phase B, resolution, one query stage) over the HOST list stages, no HIP call; every located section and
 * every located pair of tapes that holds a record goes through them.  zkir_verify_tapes_last reports the records that did, no launches, no upload. */
int zkir_verify_many_tapes_host(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts);
int zkir_verify_rate_many_tapes_host(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, const uint32_t* min_queries,
                                     const uint32_t* min_pow_bits, uint32_t n, int32_t* verdicts);
/* The list stage on its own: n = 1 .. 1024 pairs of whole sections.  hash_secs[i]: a hash section of hash_words[i] words ([0] included; words behind its last record are
 * refused, a section that ENDS inside a record is a verdict: 4); wide_secs[i]: [n_i] + 8 n_i = wide_words[i] words; n_real[i], code_end[i] (below 2^32) and per pair four
 * canonical words of alpha and lambda.  hash_verdicts[i] = 0 / 4 / 55 / 56 as zkir_hash_tape_check_*, wide_verdicts[i] = 0 / 57; digests: 4 words per chunk of 512, per
 * pair ceil(hash_words[i] / 512) chunks then ceil(wide_words[i] / 512) (zero where that section's verdict is not 0); sums: per pair 4 canonical words of the hash calls'
 * share as zkir_tape_table_side_*, then 4 of the wide records' (zero unless BOTH verdicts are 0).  _launch: at most 8 launches for all pairs (tape_stage_many.inl;
 * zkir_verify_tapes_last reports them); _host: verify.cpp's code. */
int zkir_tape_sections_stage_host(const uint32_t* const* hash_secs, const uint64_t* hash_words, const uint32_t* const* wide_secs, const uint64_t* wide_words, const uint64_t* n_real,
                                  const uint64_t* code_end, const uint32_t* alphas, const uint32_t* lambdas, uint32_t n, int32_t* hash_verdicts, int32_t* wide_verdicts, uint32_t* digests,
                                  uint32_t* sums);
int zkir_tape_sections_stage_launch(const uint32_t* const* hash_secs, const uint64_t* hash_words, const uint32_t* const* wide_secs, const uint64_t* wide_words, const uint64_t* n_real,
                                    const uint64_t* code_end, const uint32_t* alphas, const uint32_t* lambdas, uint32_t n, int32_t* hash_verdicts, int32_t* wide_verdicts, uint32_t* digests,
                                    uint32_t* sums, void* hip_stream);
/* TEST HOOK: zkir_verify_many_tapes_host (device = 0) / _device (device != 0, every batch on the device whatever the thresholds) with a PERTURBED share: what = 1 adds one to
 * proof `index`'s hash share, what = 2 to its wide share, before its deferred check — so that proof answers 10 if (and only if) the batch answered that tape's check for its
 * front.  what = 0: nothing. */
int zkir_verify_many_tapes_probe(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts, uint32_t what,
                                 uint32_t index, int device, void* hip_stream);
/* TEST HOOKS, host builds of the leaf sponge's pieces (poseidon2.h, round 28).  _scaled_quads: n states of twelve RAW input words of permute_scaled (anything inside its
 * documented input range, below 1.96 p); full[12 i ..] = its raw output words, quads[12 i + 4 Q + j] = word j of the quad permute_scaled_quad<Q> defines.
 * _sponge_full_blocks: the rate-8 sponge over n_words = 8, 16, .. words as leaf_hash_kernel runs it; form 0: the constants every kernel uses (canonical words), 1: the
 * constants derived from the input factor 1 (canonical words), 2: from the input factor R (words in Montgomery form); digest: four canonical words. */
void zkir_poseidon2_scaled_quads(const uint32_t* in, uint64_t n, uint32_t* full, uint32_t* quads);
int zkir_poseidon2_sponge_full_blocks(const uint32_t* words, uint32_t n_words, uint32_t form, uint32_t digest[4]);

#ifdef __cplusplus
}
#endif
#endif
