// pcs_verify_many.inl — the commitment layer's QUERY STAGE (verify_stages.h: checks 6 .. 11 of all queries) for a LIST of proofs whose shapes differ, and the entries over it
// (include/zkir_amd.h): zkir_verify_rate_segment_device, zkir_verify_rate_chain_device, zkir_verify_rate_many_device, zkir_pcs_verify_many_device.  Included by stark.hip at
// file scope, after query_stage.inl (the record, the kernel pair, the runner and the untrusted-input contract) and pcs_verify.inl (pcs_query_job, pcs_resolve).
//
// Everything before the stage is verify.cpp's host code, run first, proof after proof, with a COLLECTING stage (verify_stages.h: PcsCollected) in place of the queries: the
// shape, the expectations, the word range, the whole transcript, the final-degree check, grinding, the sampling — for a 'ZKSR' proof the whole STARK front and the
// constraints at zeta before that.  One stage run then serves n 'ZKLD' / 'ZKEV' / 'ZKBE' proofs that may differ in log_M, the rate b (so the final layer's size and the
// schedule), the number of matrices (1 .. 4) and their widths, the points (0 .. 2), the selections (<= 8) and the number of queries; nothing is launched for an empty
// list.  Only the 'ZKLD' / 'ZKEV' / 'ZKBE' words go up: of a 'ZKSR' proof the embedded evaluation proof, never the program, the cells or the tapes in front of it.
namespace {

// The device form of the list stage.
struct PcsManyDeviceStage {
  hipStream_t s;
  uint64_t hash_jobs = 0, value_jobs = 0, uploaded_words = 0; uint32_t launches = 0;      // what the run launched (zkir_verify_queries_last)
  int run(const zkir::PcsCollected* list, uint32_t n, int* codes) {
    if (!n) return 0;
    const char* const who = "zkir_*_many_device";
    std::vector<QueryJob> jobs(n);
    for (uint32_t i = 0; i < n; i++) {
      const zkir::PcsCollected& C = list[i];
      if (!C.filled || C.qs.size() != C.q.num_queries || C.betas_m.size() != 4 * (size_t)C.q.n_layers || C.gamma_m.size() != 4 * (size_t)C.q.n_gamma) return query_refuse(who, "a query description is not a checked proof's");
      const int jrc = pcs_query_job(C.q, who, jobs[i]);
      if (jrc) return jrc;
      jobs[i].qs = C.qs.data(); jobs[i].gamma_m = C.gamma_m.data(); jobs[i].betas_m = C.betas_m.data();      // (what the description owns)
    }
    QueryRun R{s, false, who, nullptr, nullptr};
    const int rc = R.run(jobs.data(), n);
    hash_jobs = R.hash_jobs; value_jobs = R.value_jobs; launches = R.launches; uploaded_words = R.uploaded_words;
    if (rc) return rc;
    for (uint32_t i = 0; i < n; i++) codes[i] = pcs_resolve(list[i].q, jobs[i].fh, jobs[i].f0, jobs[i].ff);
    return 0;
  }
  void note() const { zkir::verify_note_queries(hash_jobs, value_jobs, launches, uploaded_words); }
};
int pcs_many_device_run(void* p, const zkir::PcsCollected* list, uint32_t n, int* codes) { return guarded([&] { return static_cast<PcsManyDeviceStage*>(p)->run(list, n, codes); }); }

int pcs_many_refuse(const char* m) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, m}); return ZKIR_ERR_ARGUMENT; }

// What zkir_verify_rate_many_device and zkir_pcs_verify_many_device share: front(i, stage) runs proof i's host front with the collecting stage and answers its verdict so far
// (negative: no verdict for the call); then one stage run over the proofs that reached their queries; `lift` turns a query code into the entry's (100 + c for a 'ZKSR' proof).
template <typename Front>
int pcs_many_verify(uint32_t n, int32_t* verdicts, void* stream, int lift, Front front) {
  return guarded([&]() -> int {
    std::vector<int32_t> out(n, 0);
    std::vector<zkir::PcsCollected> list(n);
    std::vector<uint32_t> who;
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; i++) {
      list[k] = zkir::PcsCollected{};
      const int rc = front(i, zkir::pcs_collect_stage(&list[k]));
      if (rc < 0) return rc;
      out[i] = rc;
      if (!rc && !list[k].filled) { zkir::set_last_error({ZKIR_ERR_OTHER, "zkir_*_many_device: a front accepted a proof without reaching its queries"}); return -(int)ZKIR_ERR_OTHER; }
      if (!rc) { who.push_back(i); k++; }
    }
    PcsManyDeviceStage st{(hipStream_t)stream};
    std::vector<int> codes((size_t)k + 1, 0);
    if (k) { const int src = st.run(list.data(), k, codes.data()); if (src) return src; }      // (no proof reached its queries: nothing is launched)
    st.note();
    for (uint32_t j = 0; j < k; j++) out[who[j]] = codes[j] ? lift + codes[j] : 0;
    memcpy(verdicts, out.data(), (size_t)n * sizeof(int32_t));
    return 0;
  });
}

}  // namespace

extern "C" {

int zkir_verify_rate_segment_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits, uint32_t first_state[68],
                                    uint32_t last_state[68], void* stream) {
  uint32_t st[2 * 68];
  int32_t verdict = 0;
  const int rc = pcs_many_verify(1, &verdict, stream, 100, [&](uint32_t, const zkir::QueryStage& collect) {
    return zkir::rate_segment_verify_with_stage(proof, proof_words, expect, min_queries, min_pow_bits, collect, st, nullptr);
  });
  zkir::verify_note_device_stages(0);
  if (rc) return rc > 0 ? -rc : rc;                              // (a batch of one has no argument of its own to refuse: whatever fails here is no verdict)
  if (verdict == 0) { if (first_state) memcpy(first_state, st, sizeof st / 2); if (last_state) memcpy(last_state, st + 68, sizeof st / 2); }
  return verdict;
}

int zkir_verify_rate_chain_device(const uint32_t* const* proofs, const uint64_t* proof_words, uint32_t n_segments, const zkir_public_inputs* expect, uint32_t min_queries,
                                  uint32_t min_pow_bits, void* stream) {
  if (proofs && proof_words && n_segments == 1 && proofs[0] && proof_words[0] > 9 && proofs[0][9] >= 3) return zkir_verify_rate_device(proofs[0], proof_words[0], expect, min_queries, min_pow_bits, stream);      // a whole run by itself
  PcsManyDeviceStage st{(hipStream_t)stream};
  const int rc = guarded([&] { return zkir::rate_chain_with_stage(proofs, proof_words, n_segments, expect, min_queries, min_pow_bits, zkir::PcsManyStage{&st, pcs_many_device_run}); });
  zkir::verify_note_device_stages(0);
  if (rc >= 0) st.note();
  return rc;
}

int zkir_verify_rate_many_device(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, const uint32_t* min_queries,
                                 const uint32_t* min_pow_bits, uint32_t n, int32_t* verdicts, void* stream) {
  if (!proofs || !proof_words || !verdicts) return pcs_many_refuse("zkir_verify_rate_many_device: null proofs, proof_words or verdicts");
  if (n < 1 || n > 1024) return pcs_many_refuse("zkir_verify_rate_many_device: n must be 1 .. 1024");
  uint32_t stages_total = 0;
  const int rc = pcs_many_verify(n, verdicts, stream, 100, [&](uint32_t i, const zkir::QueryStage& collect) -> int {
    const uint32_t* w = proofs[i]; const uint64_t len = proof_words[i];
    const zkir_public_inputs* expect = expects ? expects[i] : nullptr;
    const uint32_t mq = min_queries ? min_queries[i] : 1u, mb = min_pow_bits ? min_pow_bits[i] : 0u;
    if (!w || len < 10 || w[9] != 4) return zkir::rate_verify_with_stage(w, len, expect, mq, mb, collect);
    // mode 4: the three tape stages on the device as in zkir_verify_rate_device, under the device state's mutex for this proof's front (a description owns its draws, so
    // the staging the tape stages leave behind is free for the next proof and for the shared query stage)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { zkir::set_last_error({ZKIR_ERR_DEVICE, "zkir_verify_rate_many_device: no current HIP device"}); return -ZKIR_ERR_DEVICE; }
    VerifyDevice& V = verify_device(dev);
    std::lock_guard<std::mutex> lock(V.mu);
    V.pin.reset();
    DeviceTapes dt(V, (hipStream_t)stream);
    const zkir::TapeStages tapes{&dt, dt_hash_check, dt_wide_check, dt_digests, dt_hash_side, dt_wide_side};
    const int frc = zkir::rate_verify_with_stage(w, len, expect, mq, mb, collect, &tapes);
    if (dt.stages_run) (void)hipStreamSynchronize((hipStream_t)stream);      // (a verdict reached before a stage's own synchronisation: nothing of this proof stays in flight)
    stages_total += dt.stages_run;
    return frc;
  });
  zkir::verify_note_device_stages(stages_total);
  return rc;
}

// zkir_verify_rate_many_device with the memory sections of all mode-3 / mode-4 proofs as ONE device batch (mem_stage_many.inl; the orchestration is verify.cpp's
// zkir::rate_many_with_mem_stage)
int zkir_verify_rate_many_memory_device(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, const uint32_t* min_queries,
                                        const uint32_t* min_pow_bits, uint32_t n, int32_t* verdicts, void* stream) {
  if (!proofs || !proof_words || !verdicts) return pcs_many_refuse("zkir_verify_rate_many_memory_device: null proofs, proof_words or verdicts");
  if (n < 1 || n > 1024) return pcs_many_refuse("zkir_verify_rate_many_memory_device: n must be 1 .. 1024");
  return guarded([&]() -> int {
    zkir::MemManyNote note;
    MemManyDevice md{(hipStream_t)stream, "zkir_verify_rate_many_memory_device"};
    PcsManyDeviceStage st{(hipStream_t)stream};
    const zkir::TapeStagesFor tapes = md.tapes_for();
    const int rc = zkir::rate_many_with_mem_stage(proofs, proof_words, expects, min_queries, min_pow_bits, n, md.stage(), verify_device_min_cells(), &tapes,
                                                  zkir::PcsManyStage{&st, pcs_many_device_run}, zkir::MemManyProbe{}, verdicts, &note);
    zkir::verify_note_device_stages(md.tape_stages + md.launches);
    if (rc) return rc;
    st.note();
    zkir::verify_note_memory(note.cells, md.launches, md.uploaded_words);
    return 0;
  });
}

// zkir_verify_rate_many_memory_device PLUS the tape list stage (tape_stage_many.inl), as zkir_verify_many_tapes_device
int zkir_verify_rate_many_tapes_device(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, const uint32_t* min_queries,
                                       const uint32_t* min_pow_bits, uint32_t n, int32_t* verdicts, void* stream) {
  if (!proofs || !proof_words || !verdicts) return pcs_many_refuse("zkir_verify_rate_many_tapes_device: null proofs, proof_words or verdicts");
  if (n < 1 || n > 1024) return pcs_many_refuse("zkir_verify_rate_many_tapes_device: n must be 1 .. 1024");
  return guarded([&]() -> int {
    zkir::MemManyNote note; zkir::TapeManyNote tnote;
    MemManyDevice md{(hipStream_t)stream, "zkir_verify_rate_many_tapes_device"};
    TapeManyDevice td{md};
    PcsManyDeviceStage st{(hipStream_t)stream};
    const zkir::TapeStagesFor tapes = md.tapes_for();
    const zkir::TapeManyStage ts = td.stage();
    const zkir::TapeManyRun run{&ts, verify_device_min_records(), zkir::TapeManyProbe{}, &tnote};
    const int rc = zkir::rate_many_with_mem_stage(proofs, proof_words, expects, min_queries, min_pow_bits, n, md.stage(), verify_device_min_cells(), &tapes,
                                                  zkir::PcsManyStage{&st, pcs_many_device_run}, zkir::MemManyProbe{}, verdicts, &note, &run);
    zkir::verify_note_device_stages(md.tape_stages + md.launches + td.launches);
    if (rc) return rc;
    st.note();
    zkir::verify_note_memory(note.cells, md.launches, md.uploaded_words);
    zkir::verify_note_tapes(tnote.records, td.launches, td.uploaded_words);
    return 0;
  });
}

int zkir_pcs_verify_many_device(const uint32_t* kinds, const uint32_t* const* proofs, const uint64_t* proof_words, const uint32_t* const* expect_roots, const uint32_t* const* expect_points,
                                const uint32_t* const* expect_evals, uint32_t n, int32_t* verdicts, void* stream) {
  if (!kinds || !proofs || !proof_words || !verdicts) return pcs_many_refuse("zkir_pcs_verify_many_device: null kinds, proofs, proof_words or verdicts");
  if (n < 1 || n > 1024) return pcs_many_refuse("zkir_pcs_verify_many_device: n must be 1 .. 1024");
  for (uint32_t i = 0; i < n; i++) if (kinds[i] > 2) return pcs_many_refuse("zkir_pcs_verify_many_device: a kind must be 0 ('ZKLD'), 1 ('ZKEV') or 2 ('ZKBE')");
  const int rc = pcs_many_verify(n, verdicts, stream, 0, [&](uint32_t i, const zkir::QueryStage& collect) {
    return zkir::pcs_verify_with_stage((int)kinds[i], proofs[i], proof_words[i], expect_roots ? expect_roots[i] : nullptr, expect_points ? expect_points[i] : nullptr,
                                       expect_evals ? expect_evals[i] : nullptr, collect);
  });
  zkir::verify_note_device_stages(0);
  return rc;
}

}  // extern "C"
