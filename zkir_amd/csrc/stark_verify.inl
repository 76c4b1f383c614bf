// stark_verify.inl — zkir_verify_on_device, zkir_verify_many_on_device, zkir_verify_chain_on_device (include/zkir_amd.h) and zkir_stark_query_stage_probe
// (zkir_amd_experimental.h): the product's own verifier with its QUERY STAGE (verify_stages.h: StarkQueries, checks 20 .. 27 of all queries) on the device, for ONE proof,
// for MANY independent proofs, or for the segments of a CHAIN — always one batch.  Included by stark.hip at file scope, after query_stage.inl: a STARK proof is a job of
// that file's record, kernel pair and runner — three matrices (main, aux, quotient) at b = 1, the layer-0 rule with n_points = 2, z = (zeta, zeta w), a = (a0, b0) and five
// selections — and its untrusted-input contract is stated there.
//
// Everything before the stage — header, program, cells, tapes (a mode-4 proof's through verify_device.inl's tape stages), the whole transcript, the constraints at zeta,
// the final layer's degree, grinding, the sampling — is verify.cpp's host code, run first, proof after proof.  One stage run then serves n proofs whose shapes differ
// (mode, so the widths; log_n, so depths and schedule; the number of queries), and the host picks each proof's verdict in the order the host loop returns it
// (stark_resolve).
//
// WHAT IS THIS STAGE'S OWN.  The word-range scan (every word from word 2 on is below p) and the header checks (the mode fixes WM / WA, log_n <= 26, at most 128 queries)
// come first, but the proof's LENGTH is not checked before the queries: the device takes only the n_full = min(num_queries, (len - at_queries) / qsize) queries that lie
// wholly inside the proof, the host loop the rest (the cut one decides), merged in query order.  Only the words from the trace root to the end of the last whole query are
// uploaded — never the program, the cells or the tapes in front of them — and the record's offsets are counted from the trace root.
namespace {

// One proof's verdict from its flags (fh: n_full n_slots hash flags, f24: 2 n_full, ff: n_full n_layers), with check 20 from the proof's own index words, in the host loop's
// order: for t rising — 20; 21 (main at q, at q + N); 27 (aux); 22 (quotient); per layer j: 23, then 24 (j = 0) or 25 (j > 0); 26.
int stark_resolve(const zkir::StarkQueries& Q, uint32_t n_full, const uint32_t* fh, const uint32_t* f24, const uint32_t* ff) {
  const uint32_t nl = Q.n_layers, n_slots = 6 + nl;
  for (uint32_t t = 0; t < n_full; t++) {
    if (Q.w[Q.at_queries + (uint64_t)t * Q.qsize] != Q.qs[t]) return 20;
    const uint32_t* h = fh + (size_t)t * n_slots;
    if (h[0] | h[1]) return 21;
    if (h[2] | h[3]) return 27;
    if (h[4] | h[5]) return 22;
    for (uint32_t j = 0; j < nl; j++) {
      if (h[6 + j]) return 23;
      if (j == 0 ? (f24[2 * t] | f24[2 * t + 1]) : ff[(size_t)t * nl + j - 1]) return j == 0 ? 24 : 25;
    }
    if (ff[(size_t)t * nl + nl - 1]) return 26;
  }
  return 0;
}

// ZKIR_VERIFY_QUERIES_TIMES (measurements: scripts/time_verify.py --queries): the stage synchronises after the upload and after the kernels and keeps host clocks of its parts
thread_local double stark_last_ms[3] = {0, 0, 0};               // upload, kernels, download

// The device form of the STARK query stage.
struct StarkDeviceStage {
  hipStream_t s;
  uint64_t hash_jobs = 0, value_jobs = 0, uploaded_words = 0; uint32_t launches = 0;      // what the run launched (zkir_verify_queries_last)
  int run(const zkir::StarkQueries* list, uint32_t n, int* codes) {
    if (!n) return 0;
    const char* const who = "zkir_verify_*_on_device";
    std::vector<QueryJob> jobs(n);
    for (uint32_t i = 0; i < n; i++) {
      const zkir::StarkQueries& Q = list[i];
      QueryJob& J = jobs[i];
      QueryShape& sh = J.sh;
      const uint32_t nl = Q.n_layers, WT = Q.WM + Q.WA, log_M = Q.log_n + 1;
      if (nl < 1 || nl > zkir::PCS_MAX_LAYERS || Q.num_queries > 128 || Q.log_n > 26 || Q.at_queries > Q.len || Q.at_roots >= Q.at_queries || Q.qs.size() != Q.num_queries || Q.betas_m.size() != 4 * (size_t)nl ||
          Q.gamma_m.size() != 4 * (2 * (size_t)WT + 4) || !Q.qsize) return query_refuse(who, "a query description is not a checked proof's");
      if (Q.at_lroots < Q.at_roots + 12 || Q.at_fin != Q.at_lroots + 4 * (uint64_t)nl || Q.at_queries != Q.at_fin + 4 * 8 + 1) return query_refuse(who, "the query section is not the header's");
      QueryMat mats[3] = {{Q.WM, log_M, 0, 2, 0}, {Q.WA, log_M, 4, 2, 0}, {4, log_M, 8, 2, 0}};      // main, aux, quotient under the three roots
      if (const char* why = query_layout(log_M, 1, Q.ks, nl, (uint32_t)(Q.at_lroots - Q.at_roots), mats, 3, Q.qsize, QuerySlots{sh.leaf_off, sh.leaf_words, sh.depth, sh.root_at, sh.idx_add}, J.ltab, &sh.lay0_off))
        return query_refuse(who, why);
      sh.at_queries = (uint32_t)(Q.at_queries - Q.at_roots); sh.qsize = (uint32_t)Q.qsize; sh.at_fin = (uint32_t)(Q.at_fin - Q.at_roots);
      sh.n_layers = nl; sh.n_slots = 6 + nl; sh.log_M = log_M; sh.fin_mask = (4u << 1) - 1u; sh.wM_m = bb::to_mont(bb::root_of_unity((int)log_M));
      for (uint32_t m = 0; m < 3; m++) { sh.widths[m] = mats[m].width; sh.rec_off[m] = mats[m].rec_off; }
      // the rule as data: A = main | aux | quotient at gamma^0.., B = main | aux at gamma^WT..
      const uint32_t sp[5] = {0, 0, 0, 1, 1}, sm[5] = {0, 1, 2, 0, 1}, se[5] = {0, Q.WM, 2 * WT, WT, WT + Q.WM};
      sh.n_points = 2; sh.n_sel = 5;
      for (int k = 0; k < 5; k++) { sh.sel_point[k] = sp[k]; sh.sel_mat[k] = sm[k]; sh.sel_e0[k] = se[k]; }
      memcpy(sh.z_m[0], Q.zeta_m, 16); memcpy(sh.z_m[1], Q.zeta_w_m, 16); memcpy(sh.a_m[0], Q.a0_m, 16); memcpy(sh.a_m[1], Q.b0_m, 16);
      J.qs = Q.qs.data(); J.n_qs = Q.num_queries; J.gamma_m = Q.gamma_m.data(); J.n_gamma = 2 * WT + 4; J.betas_m = Q.betas_m.data();
      J.n_full = (uint32_t)std::min<uint64_t>(Q.num_queries, (Q.len - Q.at_queries) / Q.qsize);
      J.words = Q.w + Q.at_roots; J.n_words = J.n_full ? (Q.at_queries - Q.at_roots) + (uint64_t)J.n_full * Q.qsize : 0;      // (a proof without a whole query sends nothing)
    }
    QueryRun R{s, false, who, "ZKIR_VERIFY_QUERIES_TIMES", stark_last_ms};
    const int rc = R.run(jobs.data(), n);
    hash_jobs = R.hash_jobs; value_jobs = R.value_jobs; launches = R.launches; uploaded_words = R.uploaded_words;
    if (rc) return rc;
    // the whole queries' codes from the flags; behind them the queries a short proof cuts: the host loop's codes (query order)
    for (uint32_t i = 0; i < n; i++) {
      codes[i] = jobs[i].n_full ? stark_resolve(list[i], jobs[i].n_full, jobs[i].fh, jobs[i].f0, jobs[i].ff) : 0;
      if (!codes[i] && jobs[i].n_full < list[i].num_queries) codes[i] = zkir::stark_host_queries_from(list[i], jobs[i].n_full);
    }
    return 0;
  }
  void note() const { zkir::verify_note_queries(hash_jobs, value_jobs, launches, uploaded_words); }
};
int stark_device_run(void* p, const zkir::StarkQueries* list, uint32_t n, int* codes) { return guarded([&] { return static_cast<StarkDeviceStage*>(p)->run(list, n, codes); }); }

int stark_refuse(const char* m) { zkir::set_last_error({ZKIR_ERR_ARGUMENT, m}); return ZKIR_ERR_ARGUMENT; }

}  // namespace

extern "C" {

int zkir_verify_on_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, void* stream) {
  stark_last_ms[0] = stark_last_ms[1] = stark_last_ms[2] = 0;
  return guarded([&]() -> int {
    zkir::StarkQueries Q;
    uint32_t stages_run = 0;
    const int rc = verify_device_part(proof, proof_words, expect, stream, &Q, &stages_run);
    zkir::verify_note_device_stages(stages_run);
    if (rc) return rc;
    StarkDeviceStage st{(hipStream_t)stream};
    int code = 0;
    const int src = st.run(&Q, 1, &code);
    if (src) return src;
    st.note();
    return code ? code : zkir::stark_length_check(Q);
  });
}

// zkir_verify's verdict with the memory section's three stages (mem_stage.inl) and a mode-4 proof's tape stages on the device; queries != 0: the query stage too.
int zkir_verify_memory_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, int queries, void* stream) {
  // modes 0 - 2 have no memory section (and a proof too short to name its mode has no verdict that depends on one): the existing entries
  if (!has_memory_section(proof, proof_words)) return queries ? zkir_verify_on_device(proof, proof_words, expect, stream) : zkir_verify_device(proof, proof_words, expect, stream);
  stark_last_ms[0] = stark_last_ms[1] = stark_last_ms[2] = 0;
  return guarded([&]() -> int {
    zkir::StarkQueries Q;
    MemRunNote note;
    const int rc = with_memory_stages(proof, proof_words, stream, "zkir_verify_memory_device", [&](const zkir::TapeStages* tapes, const zkir::MemStages* mem) {
      return zkir::stark_verify_collect(proof, proof_words, expect, true, tapes, queries ? &Q : nullptr, mem);
    }, &note);
    zkir::verify_note_device_stages(note.stages_run);
    zkir::verify_note_memory(note.cells, note.launches, note.uploaded_words);
    if (rc || !queries) return rc;
    StarkDeviceStage st{(hipStream_t)stream};
    int code = 0;
    const int src = st.run(&Q, 1, &code);
    if (src) return src;
    st.note();
    return code ? code : zkir::stark_length_check(Q);
  });
}

int zkir_verify_many_on_device(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts, void* stream) {
  stark_last_ms[0] = stark_last_ms[1] = stark_last_ms[2] = 0;
  if (!proofs || !proof_words || !verdicts) return stark_refuse("zkir_verify_many_on_device: null proofs, proof_words or verdicts");
  if (n < 1 || n > 1024) return stark_refuse("zkir_verify_many_on_device: n must be 1 .. 1024");
  return guarded([&]() -> int {
    std::vector<int32_t> out(n, 0);
    std::vector<zkir::StarkQueries> list;
    std::vector<uint32_t> who;
    uint32_t stages_total = 0;
    for (uint32_t i = 0; i < n; i++) {                           // the host parts, proof after proof (a mode-4 proof's tapes through the device tape stages, which reset the
      zkir::StarkQueries Q;                                      //  per-device staging: a description owns its draws)
      uint32_t stages_run = 0;
      const int rc = verify_device_part(proofs[i], proof_words[i], expects ? expects[i] : nullptr, stream, &Q, &stages_run);
      stages_total += stages_run;
      if (rc < 0) return rc;
      out[i] = rc;
      if (!rc) { list.push_back(std::move(Q)); who.push_back(i); }
    }
    zkir::verify_note_device_stages(stages_total);
    StarkDeviceStage st{(hipStream_t)stream};
    std::vector<int> codes(list.size() + 1, 0);
    if (!list.empty()) {                                         // (no proof reached its queries: nothing is launched)
      const int src = st.run(list.data(), (uint32_t)list.size(), codes.data());
      if (src) return src;
    }
    st.note();
    for (size_t k = 0; k < list.size(); k++) out[who[k]] = codes[k] ? codes[k] : zkir::stark_length_check(list[k]);
    memcpy(verdicts, out.data(), (size_t)n * sizeof(int32_t));
    return 0;
  });
}

// zkir_verify_many_on_device with the memory sections of all mode-3 / mode-4 proofs as ONE device batch (mem_stage_many.inl; the orchestration is verify.cpp's
// zkir::verify_many_with_mem_stage).  device = 0: the host list stage and the host query stage (the probe's host form).
static int verify_many_memory_run(const char* who, const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts,
                                  const zkir::MemManyProbe& probe, int device, uint64_t min_cells, void* stream) {
  stark_last_ms[0] = stark_last_ms[1] = stark_last_ms[2] = 0;
  if (!proofs || !proof_words || !verdicts) return stark_refuse((std::string(who) + ": null proofs, proof_words or verdicts").c_str());
  if (n < 1 || n > 1024) return stark_refuse((std::string(who) + ": n must be 1 .. 1024").c_str());
  return guarded([&]() -> int {
    zkir::MemManyNote note;
    if (!device) {
      const int rc = zkir::verify_many_with_mem_stage(proofs, proof_words, expects, n, zkir::host_mem_many_stage(), 0, nullptr, zkir::host_stark_query_stage(), probe, verdicts, &note);
      zkir::verify_note_memory(note.cells, 0, 0);
      return rc;
    }
    MemManyDevice md{(hipStream_t)stream, who};
    StarkDeviceStage st{(hipStream_t)stream};
    const zkir::TapeStagesFor tapes = md.tapes_for();
    const int rc = zkir::verify_many_with_mem_stage(proofs, proof_words, expects, n, md.stage(), min_cells, &tapes, zkir::StarkQueryStage{&st, stark_device_run}, probe, verdicts, &note);
    zkir::verify_note_device_stages(md.tape_stages + md.launches);
    if (rc) return rc;
    st.note();
    zkir::verify_note_memory(note.cells, md.launches, md.uploaded_words);
    return 0;
  });
}
int zkir_verify_many_memory_device(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts, void* stream) {
  return verify_many_memory_run("zkir_verify_many_memory_device", proofs, proof_words, expects, n, verdicts, zkir::MemManyProbe{}, 1, verify_device_min_cells(), stream);
}
int zkir_verify_many_memory_probe(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts, uint32_t what,
                                  uint32_t index, int device, void* stream) {
  if (what > 1 || index >= n) return stark_refuse("zkir_verify_many_memory_probe: what must be 0 or 1 and index below n");
  return verify_many_memory_run("zkir_verify_many_memory_probe", proofs, proof_words, expects, n, verdicts, zkir::MemManyProbe{what, index}, device, 0, stream);
}

// zkir_verify_many_memory_device PLUS the tape list stage (tape_stage_many.inl): the hash and wide tapes of all mode-4 proofs as ONE device batch beside the memory batch,
// around one pass of fronts and one query stage.  device = 0: the host list stages and the host query stage (the probe's host form).
static int verify_many_tapes_run(const char* who, const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts,
                                 const zkir::TapeManyProbe& probe, int device, uint64_t min_cells, uint64_t min_records, void* stream) {
  stark_last_ms[0] = stark_last_ms[1] = stark_last_ms[2] = 0;
  if (!proofs || !proof_words || !verdicts) return stark_refuse((std::string(who) + ": null proofs, proof_words or verdicts").c_str());
  if (n < 1 || n > 1024) return stark_refuse((std::string(who) + ": n must be 1 .. 1024").c_str());
  return guarded([&]() -> int {
    zkir::MemManyNote note; zkir::TapeManyNote tnote;
    if (!device) {
      const zkir::TapeManyStage hs = zkir::host_tape_many_stage();
      const zkir::TapeManyRun run{&hs, 0, probe, &tnote};
      const int rc = zkir::verify_many_with_mem_stage(proofs, proof_words, expects, n, zkir::host_mem_many_stage(), 0, nullptr, zkir::host_stark_query_stage(), zkir::MemManyProbe{}, verdicts, &note, &run);
      zkir::verify_note_memory(note.cells, 0, 0);
      zkir::verify_note_tapes(tnote.records, 0, 0);
      return rc;
    }
    MemManyDevice md{(hipStream_t)stream, who};
    TapeManyDevice td{md};
    StarkDeviceStage st{(hipStream_t)stream};
    const zkir::TapeStagesFor tapes = md.tapes_for();
    const zkir::TapeManyStage ts = td.stage();
    const zkir::TapeManyRun run{&ts, min_records, probe, &tnote};
    const int rc = zkir::verify_many_with_mem_stage(proofs, proof_words, expects, n, md.stage(), min_cells, &tapes, zkir::StarkQueryStage{&st, stark_device_run}, zkir::MemManyProbe{}, verdicts, &note, &run);
    zkir::verify_note_device_stages(md.tape_stages + md.launches + td.launches);
    if (rc) return rc;
    st.note();
    zkir::verify_note_memory(note.cells, md.launches, md.uploaded_words);
    zkir::verify_note_tapes(tnote.records, td.launches, td.uploaded_words);
    return 0;
  });
}
int zkir_verify_many_tapes_device(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts, void* stream) {
  return verify_many_tapes_run("zkir_verify_many_tapes_device", proofs, proof_words, expects, n, verdicts, zkir::TapeManyProbe{}, 1, verify_device_min_cells(), verify_device_min_records(), stream);
}
int zkir_verify_many_tapes_probe(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts, uint32_t what,
                                 uint32_t index, int device, void* stream) {
  if (what > 2 || index >= n) return stark_refuse("zkir_verify_many_tapes_probe: what must be 0 .. 2 and index below n");
  return verify_many_tapes_run("zkir_verify_many_tapes_probe", proofs, proof_words, expects, n, verdicts, zkir::TapeManyProbe{what, index}, device, 0, 0, stream);
}

int zkir_verify_chain_on_device(const uint32_t* const* proofs, const uint64_t* proof_words, uint32_t n_segments, const zkir_public_inputs* expect, void* stream) {
  if (proofs && proof_words && n_segments == 1 && proofs[0] && proof_words[0] > 9 && proofs[0][9] >= 3) return zkir_verify_on_device(proofs[0], proof_words[0], expect, stream);      // a whole run by itself
  stark_last_ms[0] = stark_last_ms[1] = stark_last_ms[2] = 0;
  StarkDeviceStage st{(hipStream_t)stream};
  const int rc = guarded([&] { return zkir::verify_chain_with_stage(proofs, proof_words, n_segments, expect, zkir::StarkQueryStage{&st, stark_device_run}); });
  zkir::verify_note_device_stages(0);
  if (rc >= 0) st.note();
  return rc;
}

int zkir_verify_queries_last_stage_ms(double ms[3]) {
  if (!ms) return ZKIR_ERR_ARGUMENT;
  for (int k = 0; k < 3; k++) ms[k] = stark_last_ms[k];
  return ZKIR_OK;
}

int zkir_stark_query_stage_probe(const uint32_t* proof, uint64_t proof_words, uint32_t what, uint32_t index, int device, void* stream) {
  return guarded([&]() -> int {
    zkir::StarkQueries Q;
    const int rc = zkir::stark_verify_collect(proof, proof_words, nullptr, true, nullptr, &Q);
    if (rc) return rc;
    auto bump = [](uint32_t* e) { e[0] = bb::add(e[0], bb::R1); };      // + 1 on a Montgomery E4
    switch (what) {
      case 0: break;
      case 1: bump(Q.a0_m); break;
      case 2: bump(Q.b0_m); break;
      case 3: bump(Q.zeta_m); break;
      case 4: if (index >= Q.n_layers) return -stark_refuse("zkir_stark_query_stage_probe: no such layer"); bump(Q.betas_m.data() + 4 * (size_t)index); break;
      case 5: if (index >= Q.num_queries) return -stark_refuse("zkir_stark_query_stage_probe: no such query"); Q.qs[index] ^= 1u; break;
      default: return -stark_refuse("zkir_stark_query_stage_probe: what must be 0 .. 5");
    }
    int code = 0;
    if (device) {
      StarkDeviceStage st{(hipStream_t)stream};
      const int src = st.run(&Q, 1, &code);
      if (src) return src;
      st.note();
    } else {
      const zkir::StarkQueryStage hs = zkir::host_stark_query_stage();
      const int src = hs.run(hs.self, &Q, 1, &code);
      if (src) return src;
    }
    return code ? code : zkir::stark_length_check(Q);
  });
}

}  // extern "C"
