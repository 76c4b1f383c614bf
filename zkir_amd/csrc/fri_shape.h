// fri_shape.h — the shape of the one FRI every proof here runs: which layers are committed, how large the final layer is, how many words a query's layers take.
// Host only (no HIP): the provers (stark.hip) and the verifiers (verify.cpp) both read it, so neither side can fold a layer the other does not expect.
//
// A codeword of M = 2^(log_n + b) values (b = log_blowup: 1 for a STARK proof, 1 .. 3 for the commitment layer's proofs) is folded down to 4 << b values of a word of
// degree < 4.  Specs: oracle/stark_oracle.cpp (so::fri_schedule, b = 1), tests/lowdeg_ref.py (any b).
#pragma once

#include <cstdint>
#include <vector>

#include "air.h"

namespace zkir {

// the STARK proof states LOG_FINAL as a header word; it is this file's final layer at b = 1
static_assert(air::LOG_FINAL == 2 + 1, "a STARK proof's final layer is fri_final_size(1) values");

// values of the final layer
constexpr uint32_t fri_final_size(int b) { return 4u << b; }

// Folds per committed layer: the codeword is folded once (its leaves are the pairs (q, q + M/2) the matrix openings determine), later layers LOG_ARITY times (8-to-1: three
// binary folds with beta, beta^2, beta^4), the last one as needed to land on the final layer.  A commitment costs ~log2(leaves) SEQUENTIAL Poseidon2 levels (~10 us each
// once a level is small), so committing every third fold cuts the latency-bound part of FRI from ~200 levels to ~80 at 2^20 rows.
inline std::vector<int> fri_schedule(int log_n, int b) {
  std::vector<int> ks;
  const int log_fin = 2 + b;
  for (int log_m = log_n + b; log_m > log_fin;) {
    const int k = ks.empty() ? 1 : (air::LOG_ARITY < log_m - log_fin ? air::LOG_ARITY : log_m - log_fin);
    ks.push_back(k); log_m -= k;
  }
  return ks;
}

// The schedule of a proof over codewords of several heights ('ZKMH', mixed_eval.inl): log_ns[0] > log_ns[1] > .. at one b.  fri_schedule's rule with one more cap: a step never
// jumps over the size M_h = 2^(log_ns[h] + b) of a lower codeword, so every M_h (h >= 1) is the size of a committed layer — the layer F_h is added to before it is hashed.
// ks[0] stays 1.  One height gives fri_schedule(log_ns[0], b).  Spec: tests/mixed_eval_ref.py.
inline std::vector<int> fri_mixed_schedule(const uint32_t* log_ns, uint32_t n_groups, int b) {
  std::vector<int> ks;
  const int log_fin = 2 + b;
  for (int log_m = (int)log_ns[0] + b; log_m > log_fin;) {
    int k = ks.empty() ? 1 : (air::LOG_ARITY < log_m - log_fin ? air::LOG_ARITY : log_m - log_fin);
    for (uint32_t h = 1; h < n_groups; h++) {
      const int lower = (int)log_ns[h] + b;
      if (lower < log_m && log_m - lower < k) k = log_m - lower;
    }
    ks.push_back(k); log_m -= k;
  }
  return ks;
}

// words of one query's FRI layers: per layer its 2^k values (4 words each) and the path of its leaf (4 words a level, depth = log2 of the layer's leaves)
inline uint64_t fri_query_words(uint32_t log_M, const std::vector<int>& ks) {
  uint64_t words = 0;
  int log_m = (int)log_M;
  for (int k : ks) { words += 4 * ((uint64_t)1 << k) + 4 * (uint64_t)(log_m - k); log_m -= k; }
  return words;
}

}  // namespace zkir
