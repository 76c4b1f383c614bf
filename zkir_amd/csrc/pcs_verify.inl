// pcs_verify.inl — zkir_lowdeg_verify_device, zkir_eval_verify_device, zkir_batch_eval_verify_device, zkir_verify_rate_device (include/zkir_amd.h): the verifiers of the
// commitment layer with their QUERY STAGE (verify_stages.h: checks 6 .. 11 of all queries) on the device.  Included by stark.hip at file scope, after query_stage.inl: the
// stage is a BATCH OF ONE over that file's record, kernel pair and runner (one staged upload, two launches, one download, one synchronisation on the caller's stream),
// and its untrusted-input contract is stated there.
//
// Everything before the stage — shape, expectations, word range (checks 1 and 3: the proof's length is EXACTLY what its header states and every word is below p), the whole
// transcript, the final-degree check, grinding, the sampling — is verify.cpp's host code, run first and unchanged.  The host picks the verdict from the flags in the order
// the host loop returns it (pcs_resolve).
namespace {

// A 'ZKLD' / 'ZKEV' / 'ZKBE' proof's description as a job of the shared stage: the bounds everything below is indexed within, the record (every offset from the checked
// header, counted from the proof's first word), the whole proof as the span to upload.  The job borrows the description's samples, gamma table and betas.
int pcs_query_job(const zkir::PcsQueries& Q, const char* who, QueryJob& J) {
  const char* const bad = "a query description is not a checked proof's";
  const uint32_t nl = Q.n_layers, nq = Q.num_queries, n_fin = 4u << Q.b;
  if (!Q.w || !Q.qs || !Q.betas_m || !Q.gamma_m || nl < 1 || nl > zkir::PCS_MAX_LAYERS || Q.n_mats < 1 || Q.n_mats > zkir::PCS_MAX_MATS || nq < 1 || nq > 128 || Q.b < 1 || Q.b > 3 || Q.log_M < 2 ||
      Q.log_M > 27 || Q.n_points > 2 || Q.n_sel > zkir::PCS_MAX_SEL || Q.len >> 31 || Q.at_roots + 4 * (uint64_t)Q.n_mats > Q.len || Q.at_lroots + 4 * (uint64_t)nl > Q.len ||
      Q.at_fin + 4 * (uint64_t)n_fin > Q.at_queries || Q.at_queries > Q.len) return query_refuse(who, bad);
  QueryShape& sh = J.sh;
  QueryMat mats[zkir::PCS_MAX_MATS];
  for (uint32_t m = 0; m < Q.n_mats; m++) {
    if (Q.widths[m] < 1 || Q.widths[m] > 512) return query_refuse(who, bad);
    mats[m] = QueryMat{Q.widths[m], Q.log_M, (uint32_t)Q.at_roots + 4 * m, 2, 0};
  }
  if (const char* why = query_layout(Q.log_M, Q.b, Q.ks, nl, (uint32_t)Q.at_lroots, mats, Q.n_mats, Q.qsize, QuerySlots{sh.leaf_off, sh.leaf_words, sh.depth, sh.root_at, sh.idx_add}, J.ltab, &sh.lay0_off))
    return query_refuse(who, why);
  if (Q.at_queries + (uint64_t)nq * Q.qsize != Q.len) return query_refuse(who, "the query section is not the header's");
  sh.at_queries = (uint32_t)Q.at_queries; sh.qsize = (uint32_t)Q.qsize; sh.at_fin = (uint32_t)Q.at_fin;
  sh.n_layers = nl; sh.n_slots = 2 * Q.n_mats + nl; sh.log_M = Q.log_M; sh.fin_mask = n_fin - 1u; sh.n_points = Q.n_points;
  for (uint32_t m = 0; m < Q.n_mats; m++) { sh.widths[m] = Q.widths[m]; sh.rec_off[m] = mats[m].rec_off; }
  // the layer-0 rule as data (n_points = 0: one selected pair, the plain sum over matrix 0); every selection stays inside the gamma table
  if (Q.n_points == 0) { sh.n_sel = 1; if (Q.n_gamma < Q.widths[0]) return query_refuse(who, bad); }
  else {
    sh.n_sel = Q.n_sel;
    for (uint32_t k = 0; k < Q.n_sel; k++) {
      if (Q.sel[k].point >= Q.n_points || Q.sel[k].mat >= Q.n_mats || (uint64_t)Q.sel[k].e0 + Q.widths[Q.sel[k].mat] > Q.n_gamma) return query_refuse(who, bad);
      sh.sel_point[k] = Q.sel[k].point; sh.sel_mat[k] = Q.sel[k].mat; sh.sel_e0[k] = Q.sel[k].e0;
    }
    memcpy(sh.z_m, Q.z_m, sizeof sh.z_m); memcpy(sh.a_m, Q.a_m, sizeof sh.a_m);
    sh.wM_m = bb::to_mont(bb::root_of_unity((int)Q.log_M));
  }
  J.qs = Q.qs; J.n_qs = nq; J.gamma_m = Q.gamma_m; J.n_gamma = Q.n_gamma; J.betas_m = Q.betas_m;
  J.words = Q.w; J.n_words = Q.len; J.n_full = nq;
  return 0;
}

// The verdict of checks 7 .. 11 from the flags, with check 6 from the proof's own index words: for t rising — 6; 7 for matrix 0 row q, matrix 0 row q + M/2, matrix 1 ...;
// 8; per layer j: 9 (j), then 10 (j) for j > 0; 11.  Exactly the order in which verify.cpp's loop returns.
int pcs_resolve(const zkir::PcsQueries& Q, const uint32_t* fh, const uint32_t* f8, const uint32_t* ff) {
  const uint32_t n_slots = 2 * Q.n_mats + Q.n_layers;
  for (uint32_t t = 0; t < Q.num_queries; t++) {
    if (Q.w[Q.at_queries + (uint64_t)t * Q.qsize] != Q.qs[t]) return 6;
    const uint32_t* h = fh + (size_t)t * n_slots;
    for (uint32_t sl = 0; sl < 2 * Q.n_mats; sl++) if (h[sl]) return 7;
    if (f8[2 * t] | f8[2 * t + 1]) return 8;
    for (uint32_t j = 0; j < Q.n_layers; j++) {
      if (h[2 * Q.n_mats + j]) return 9;
      if (j > 0 && ff[(size_t)t * Q.n_layers + j - 1]) return 10;
    }
    if (ff[(size_t)t * Q.n_layers + Q.n_layers - 1]) return 11;
  }
  return 0;
}

thread_local uint64_t pcs_last_jobs[2] = {0, 0};                 // what the calling thread's last *_verify_device call launched (zkir_pcs_verify_last_jobs)

// ZKIR_PCS_VERIFY_TIMES (measurements: scripts/time_pcs_verify.py): the stage synchronises after the upload and after the kernels and keeps host clocks of its parts
thread_local double pcs_last_ms[3] = {0, 0, 0};                  // upload, kernels, download

// The device form of the query stage: a batch of one.  It leaves zkir_verify_queries_last's record alone.
struct PcsDeviceStage {
  hipStream_t s;
  bool held = false;                                             // the caller holds the device state's mutex already (zkir_verify_rate_device on a mode-4 proof: the tape stages ran under it)
  int run(const zkir::PcsQueries& Q) {
    QueryJob J{};
    const int jrc = pcs_query_job(Q, "zkir_*_verify_device", J);
    if (jrc) return jrc;
    QueryRun R{s, held, "zkir_*_verify_device", "ZKIR_PCS_VERIFY_TIMES", pcs_last_ms};
    const int rc = R.run(&J, 1);
    pcs_last_jobs[0] = R.hash_jobs; pcs_last_jobs[1] = R.value_jobs;
    return rc ? rc : pcs_resolve(Q, J.fh, J.f0, J.ff);
  }
};
int pcs_device_run(void* p, const zkir::PcsQueries& Q) { return guarded([&] { return static_cast<PcsDeviceStage*>(p)->run(Q); }); }

int pcs_verify_device(int kind, const uint32_t* proof, uint64_t n_words, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals, void* stream) {
  pcs_last_jobs[0] = pcs_last_jobs[1] = 0;
  pcs_last_ms[0] = pcs_last_ms[1] = pcs_last_ms[2] = 0;
  PcsDeviceStage st{(hipStream_t)stream};
  return guarded([&] { return zkir::pcs_verify_with_stage(kind, proof, n_words, expect_roots, expect_points, expect_evals, zkir::QueryStage{&st, pcs_device_run}); });
}

}  // namespace

extern "C" {

int zkir_lowdeg_verify_device(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_root, void* stream) { return pcs_verify_device(0, proof, n_words, expect_root, nullptr, nullptr, stream); }
int zkir_eval_verify_device(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_root, const uint32_t* expect_points, const uint32_t* expect_evals, void* stream) {
  return pcs_verify_device(1, proof, n_words, expect_root, expect_points, expect_evals, stream);
}
int zkir_batch_eval_verify_device(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals, void* stream) {
  return pcs_verify_device(2, proof, n_words, expect_roots, expect_points, expect_evals, stream);
}

// zkir_verify_rate with the embedded evaluation proof's query stage on the device: the same function, the same verdict for every input
int zkir_verify_rate_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits, void* stream) {
  pcs_last_jobs[0] = pcs_last_jobs[1] = 0;
  pcs_last_ms[0] = pcs_last_ms[1] = pcs_last_ms[2] = 0;
  PcsDeviceStage st{(hipStream_t)stream};
  // modes 0 - 3 have no tapes (and a proof too short to name its mode has no verdict that depends on them): the host front, the query stage on the device
  if (!proof || proof_words < 10 || proof[9] != 4) return guarded([&] { return zkir::rate_verify_with_stage(proof, proof_words, expect, min_queries, min_pow_bits, zkir::QueryStage{&st, pcs_device_run}); });
  // mode 4: the three tape stages on the device as in zkir_verify_device (verify_device.inl), under the device state's mutex for the whole call
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_verify_rate_device: no current HIP device"}); return -ZKIR_ERR_DEVICE; }
  VerifyDevice* Vp = nullptr;
  const int src = guarded([&] { Vp = &verify_device(dev); return 0; });
  if (src) return src;
  std::lock_guard<std::mutex> lock(Vp->mu);
  Vp->pin.reset();
  DeviceTapes dt(*Vp, (hipStream_t)stream);
  const zkir::TapeStages tapes{&dt, dt_hash_check, dt_wide_check, dt_digests, dt_hash_side, dt_wide_side};
  st.held = true;
  const int rc = guarded([&] { return zkir::rate_verify_with_stage(proof, proof_words, expect, min_queries, min_pow_bits, zkir::QueryStage{&st, pcs_device_run}, &tapes); });
  if (dt.stages_run) (void)hipStreamSynchronize((hipStream_t)stream);      // (a verdict reached before a stage's own synchronisation: nothing of this call stays in flight)
  zkir::verify_note_device_stages(dt.stages_run);
  return rc;
}

// zkir_verify_rate_device with a mode-3 / mode-4 proof's memory stages (mem_stage.inl) on the device too, under the device state's mutex for the whole call
int zkir_verify_rate_memory_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits, void* stream) {
  if (!has_memory_section(proof, proof_words)) return zkir_verify_rate_device(proof, proof_words, expect, min_queries, min_pow_bits, stream);
  pcs_last_jobs[0] = pcs_last_jobs[1] = 0;
  pcs_last_ms[0] = pcs_last_ms[1] = pcs_last_ms[2] = 0;
  PcsDeviceStage st{(hipStream_t)stream};
  st.held = true;
  MemRunNote note;
  const int rc = with_memory_stages(proof, proof_words, stream, "zkir_verify_rate_memory_device", [&](const zkir::TapeStages* tapes, const zkir::MemStages* mem) {
    return zkir::rate_verify_with_stage(proof, proof_words, expect, min_queries, min_pow_bits, zkir::QueryStage{&st, pcs_device_run}, tapes, mem);
  }, &note);
  zkir::verify_note_device_stages(note.stages_run);
  zkir::verify_note_memory(note.cells, note.launches, note.uploaded_words);
  return rc;
}

int zkir_pcs_verify_last_jobs(uint64_t* hash_jobs, uint64_t* value_jobs) {
  if (hash_jobs) *hash_jobs = pcs_last_jobs[0];
  if (value_jobs) *value_jobs = pcs_last_jobs[1];
  return ZKIR_OK;
}
int zkir_pcs_verify_last_stage_ms(double ms[3]) {
  if (!ms) return ZKIR_ERR_ARGUMENT;
  for (int k = 0; k < 3; k++) ms[k] = pcs_last_ms[k];
  return ZKIR_OK;
}

}  // extern "C"
