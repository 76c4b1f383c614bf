// verify_stages.h — the three stages of a mode-4 verification that are linear in the size of the proof's tapes (the hash section and the wide section), behind one
// small interface: verify.cpp fills it with its host code (zkir_verify and its siblings: host only, no HIP call), zkir_verify_device (verify_device.inl, in the prover's
// translation unit) with the device forms.  Everything else a verifier does (header, program, touched cells, constraints at zeta, FRI, queries) is verify.cpp's alone.
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

}  // namespace zkir
