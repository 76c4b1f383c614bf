// host_san_driver.cpp — the host entry points that read untrusted bytes (verify.cpp, interp.cpp, hashes.cpp and the host parts of hashcall.h, verify_stages.h, host.h), called on a
// corpus of honest and malformed inputs from a stand-alone program that is built with AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_host_sanitized.py builds it,
// writes the corpus and compares every verdict with the oracle's).  No HIP, no torch, no Python: the three host objects and this file.
//
// What the library defines in its HIP translation units is stated here: pinned memory is malloc memory, the last error is kept for printing, zkir_padded_log_n is restated
// (the test holds it against the library's).  The three tape entry points zkir_hash_tape_check_host / zkir_tape_table_side_host / zkir_hash_tape_new_bytes_host and
// zkir_interpret live in those units too, so their own bodies are NOT run here.  What runs in their place, with the wrappers' argument checks restated:
//   zkir_interpret                  zkir::interpret (interp.cpp), the function it forwards to;
//   zkir_hash_tape_check_host       hashcall::parse_section (hashcall.h), the function it forwards to;
//   zkir_hash_tape_new_bytes_host   hashcall::parse_section and hashcall::new_bytes, call after call in one loop: the wrapper's offsets table and its threaded memcpy into
//                                   the caller's array are not sanitized (its refusal of a null array is restated, as the other wrappers' checks are);
//   zkir_tape_table_side_host       not its body at all.  The wrapper sums with hash_table_side_host / wide_table_side_host of tape_table.inl (a HIP translation unit) over the
//                                   caller's new_bytes; the driver runs the verifier's host tape stages of verify.cpp / verify_stages.h (hash_check, wide_check, hash_side,
//                                   wide_side, digests), which read the same untrusted sections, work out new_bytes themselves and form the same sum by other code.  They
//                                   are what a proof's tapes reach in zkir_verify, hence the code at the trust boundary; tape_table.inl's host sums are held to the same
//                                   reference by tests/test_tape_table_side.py, which loads the library and so runs unsanitized.
//
// Corpus file (little-endian): 'ZKSC', n_bases, bases, n_cases, cases.  A base = [elem size u32][count u64][data].  A case = [kind u32][n_args u32][args u64..][n_bufs u32][bufs];
// a buf = [elem size u32][base u32 or 0xFFFFFFFF][take u64][n_patches u64][(position u64, value u64)..][n_inline u64][inline data]: the first `take` elements of the base,
// patched, then the inline elements.  Every buffer is handed to the entry point in a heap block of EXACTLY its length (element `count` is a redzone); a zero-length buffer is a
// valid pointer with length 0.  One verdict line per case on stdout: "<case index> <verdict>", then " | <the last error message>" where the entry point left one.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/zkir_amd.h"
#include "../../zkir_amd/csrc/air.h"
#include "../../zkir_amd/csrc/babybear.h"
#include "../../zkir_amd/csrc/hashcall.h"
#include "../../zkir_amd/csrc/host.h"
#include "../../zkir_amd/csrc/verify_stages.h"

// ---- what the HIP translation units define ----
static std::string g_last_error;
namespace zkir {
void* pinned_alloc(size_t bytes) { return malloc(bytes); }
void pinned_free(void* p) { free(p); }
void set_last_error(const Status& st) { g_last_error = st.msg; }
}  // namespace zkir
extern "C" uint32_t zkir_padded_log_n(uint64_t n_real) { uint32_t k = 3; while (((uint64_t)1 << k) < n_real) k++; return k; }

namespace {

[[noreturn]] void die(const char* what) { fprintf(stderr, "host_san_driver: %s\n", what); exit(2); }

struct Reader {
  const uint8_t* p; size_t n, at = 0;
  void need(size_t k) { if (k > n - at) die("the corpus file is cut short"); }
  uint32_t u32() { need(4); uint32_t v; memcpy(&v, p + at, 4); at += 4; return v; }
  uint64_t u64() { need(8); uint64_t v; memcpy(&v, p + at, 8); at += 8; return v; }
  const uint8_t* bytes(size_t k) { need(k); const uint8_t* q = p + at; at += k; return q; }
};

struct Base { uint32_t elem; uint64_t count; const uint8_t* data; };

// a heap block of exactly `count` elements
struct Block {
  void* p = nullptr; uint32_t elem = 1; uint64_t count = 0;
  Block() = default;
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
  Block(Block&& o) noexcept : p(o.p), elem(o.elem), count(o.count) { o.p = nullptr; }
  ~Block() { free(p); }
  const uint32_t* w() const { return (const uint32_t*)p; }
  const uint64_t* q() const { return (const uint64_t*)p; }
  const uint8_t* b() const { return (const uint8_t*)p; }
};

Block read_buf(Reader& r, const std::vector<Base>& bases) {
  Block out;
  out.elem = r.u32();
  if (out.elem != 1 && out.elem != 4 && out.elem != 8) die("element size");
  const uint32_t base = r.u32();
  const uint64_t take = r.u64(), n_patch = r.u64();
  if (base != 0xFFFFFFFFu && (base >= bases.size() || bases[base].elem != out.elem || take > bases[base].count)) die("base reference");
  if (base == 0xFFFFFFFFu && take) die("take without a base");
  const size_t patches_at = r.at;
  r.bytes((size_t)n_patch * 16);
  const uint64_t n_inline = r.u64();
  const uint8_t* inl = r.bytes((size_t)n_inline * out.elem);
  out.count = take + n_inline;
  const size_t nbytes = (size_t)out.count * out.elem;
  out.p = malloc(nbytes);                                           // (0 bytes: a valid pointer, nothing behind it)
  if (!out.p) die("out of memory");
  uint8_t* d = (uint8_t*)out.p;
  if (take) memcpy(d, bases[base].data, (size_t)take * out.elem);
  if (n_inline) memcpy(d + (size_t)take * out.elem, inl, (size_t)n_inline * out.elem);
  Reader pr{r.p, r.n, patches_at};
  for (uint64_t k = 0; k < n_patch; k++) {
    const uint64_t pos = pr.u64(), val = pr.u64();
    if (pos >= out.count) die("patch position");
    memcpy(d + (size_t)pos * out.elem, &val, out.elem);             // (little-endian host)
  }
  return out;
}

uint32_t crc32_of(const void* data, size_t n) {
  static uint32_t table[256];
  static bool made = false;
  if (!made) { for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1; table[i] = c; } made = true; }
  uint32_t c = 0xFFFFFFFFu;
  const uint8_t* b = (const uint8_t*)data;
  for (size_t i = 0; i < n; i++) c = table[(c ^ b[i]) & 0xFF] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

// a verifier's `expect` from twelve u64 words: n_real, entry point, mode, fri parameters, program digest, io digest
zkir_public_inputs expect_of(const Block& b) {
  if (b.elem != 8 || b.count != 12) die("expect block");
  zkir_public_inputs e;
  memset(&e, 0, sizeof e);
  e.n_real = b.q()[0]; e.entry_point = b.q()[1]; e.deferred = (uint32_t)b.q()[2]; e.fri_params = (uint32_t)b.q()[3];
  for (int k = 0; k < 4; k++) { e.program_digest[k] = (uint32_t)b.q()[4 + k]; e.io_digest[k] = (uint32_t)b.q()[8 + k]; }
  return e;
}

enum Kind : uint32_t { VERIFY = 0, VERIFY_SEGMENT, VERIFY_CHAIN, VERIFY_IO, VERIFY_CHAIN_IO, LOWDEG, MERKLE, HASH_CHECK, TAPE_SIDE, NEW_BYTES, CALL_CELLS, DIGEST_BYTES, INTERPRET, PADDED_LOG_N };

// zkir_tape_table_side_host's argument checks, then — in place of its body, see the head comment — the verifier's host tape stages (verify_stages.h) on the two sections:
// "refused <check>" or the sum's four canonical words and the checksum of the sections' chunk digests
void tape_side(const Block& hash, const Block& wide, const Block& alpha, const Block& lambda) {
  static const uint32_t no_calls[1] = {0u};
  const uint32_t* hw = hash.w(); uint64_t nh = hash.count;
  if (!nh) { hw = no_calls; nh = 1; }
  for (int k = 0; k < 4; k++) if (alpha.w()[k] >= bb::P || lambda.w()[k] >= bb::P) { printf("refused challenge"); return; }
  if (wide.count && wide.count != 1 + 8 * (uint64_t)wide.w()[0]) { printf("refused wide"); return; }
  zkir::HostTapes tapes;
  const zkir::TapeStages S = zkir::host_tape_stages(&tapes);
  size_t used = 0;
  const int hrc = S.hash_check(S.self, hw, (size_t)nh, ~0ull, 0, &used);
  if (hrc || used != nh) { printf("refused %d", hrc ? hrc : 4); return; }
  const uint32_t n_wide = wide.count ? wide.w()[0] : 0;
  const uint32_t* ww = wide.count ? wide.w() : no_calls;
  const int wrc = S.wide_check(S.self, ww, n_wide, ~0ull);
  if (wrc) { printf("refused %d", wrc); return; }
  uint32_t lk[air::N_LK] = {0};
  bb::E4 lam = bb::e_one_m();
  const bb::E4 l1 = bb::e_to_mont(bb::E4{{lambda.w()[0], lambda.w()[1], lambda.w()[2], lambda.w()[3]}});
  for (int k = 0; k < 4; k++) lk[air::LK_ALPHA + k] = bb::to_mont(alpha.w()[k]);
  for (int j = 0; j <= air::N_TUPLE; j++) { for (int k = 0; k < 4; k++) lk[air::LK_LAM + 4 * j + k] = lam.c[k]; lam = bb::e_mul_m(lam, l1); }
  bb::E4 Th = bb::e_zero(), Tw = bb::e_zero();
  if (S.hash_side(S.self, lk, Th.c) || S.wide_side(S.self, lk, Tw.c)) { printf("refused side"); return; }
  const bb::E4 T = bb::e_from_mont(bb::e_add(Th, Tw));
  std::vector<uint32_t> dg(4 * ((nh + 511) / 512) + 4 * (((size_t)1 + 8 * n_wide + 511) / 512));
  S.digests(S.self, 0, hw, (size_t)nh, dg.data());
  S.digests(S.self, 1, ww, (size_t)1 + 8 * n_wide, dg.data() + 4 * ((nh + 511) / 512));
  printf("sum %u %u %u %u digests %08x", T.c[0], T.c[1], T.c[2], T.c[3], crc32_of(dg.data(), dg.size() * 4));
}

// zkir_hash_tape_new_bytes_host's parser and per-call function, call after call (not its threaded copy into the caller's array): every touched cell's bytes after its call
// (no_out: the caller hands a null array; the wrapper's refusal of that, where the section has cells, is restated)
void new_bytes(const Block& hash, bool no_out) {
  static const uint32_t no_calls[1] = {0u};
  const uint32_t* hw = hash.w(); uint64_t nh = hash.count;
  if (!nh) { hw = no_calls; nh = 1; }
  std::vector<hashcall::Call> calls;
  size_t used = 0;
  const int hrc = hashcall::parse_section(hw, (size_t)nh, ~0ull, 0, calls, &used);
  if (hrc || used != nh) { printf("refused %d", hrc ? hrc : 4); return; }
  size_t cells = 0;
  for (const hashcall::Call& c : calls) cells += c.cells.size();
  if (cells && no_out) { printf("refused null"); return; }
  std::vector<uint64_t> all, nb;
  for (const hashcall::Call& c : calls) { hashcall::new_bytes(c, nb); all.insert(all.end(), nb.begin(), nb.end()); }
  printf("cells %zu crc %08x", all.size(), crc32_of(all.data(), all.size() * 8));
}

// zkir_interpret's host function under one configuration, and (traced runs) the memory witness of the asked mode on its log
void interpret(const Block& blob, const Block& inputs, const std::vector<uint64_t>& a) {
  if (a.size() != 5) die("interpret arguments");
  zkir_vm_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.max_cycles = a[0]; cfg.enable_range_checking = (uint8_t)a[1]; cfg.enable_execution_trace = (uint8_t)a[2]; cfg.enable_deferred_model = (uint8_t)a[3];
  zkir_delta_log* log = new zkir_delta_log();
  zkir::Status st;
  try { st = zkir::interpret(blob.b(), (size_t)blob.count, inputs.q(), (size_t)inputs.count, cfg, 0, *log); } catch (const std::bad_alloc&) { st = {ZKIR_ERR_OTHER, "out of host memory"}; }
  if (!st.ok()) { printf("error %d", st.code); delete log; return; }
  printf("halt %d %" PRIu64 " cycles %" PRIu64 " outputs %zu %08x", log->halt_kind, log->halt_kind == ZKIR_HALT_EXIT ? log->halt_code : 0, log->cycles, log->outputs.size(),
         crc32_of(log->outputs.data(), log->outputs.size() * 8));
  if (a[4]) {
    zkir_memcheck_witness* w = nullptr;
    const int rc = zkir_memcheck_witness_of_mode(log, blob.b(), (size_t)blob.count, (uint32_t)a[4], &w);
    if (rc) printf(" witness refused");
    else printf(" witness cells %" PRIu64 " accesses %" PRIu64 " calls %" PRIu64, zkir_memcheck_witness_n_cells(w), zkir_memcheck_witness_n_accesses(w), zkir_memcheck_witness_n_hash_calls(w));
    zkir_memcheck_witness_free(w);
  }
  delete log;
}

void run_case(uint32_t kind, const std::vector<uint64_t>& a, const std::vector<Block>& b) {
  auto want = [&](size_t n_args, size_t n_bufs) { if (a.size() != n_args || b.size() < n_bufs) die("case shape"); };
  switch (kind) {
    case VERIFY: case VERIFY_SEGMENT: {                             // args: has_expect | bufs: proof [expect]
      want(1, 1 + (size_t)a[0]);
      zkir_public_inputs e; if (a[0]) e = expect_of(b[1]);
      if (kind == VERIFY) { printf("rc %d", zkir_verify(b[0].w(), b[0].count, a[0] ? &e : nullptr)); break; }
      uint32_t first[68], last[68];
      const int rc = zkir_verify_segment(b[0].w(), b[0].count, a[0] ? &e : nullptr, first, last);
      if (rc) printf("rc %d", rc); else printf("rc 0 states %08x %08x", crc32_of(first, sizeof first), crc32_of(last, sizeof last));
      break;
    }
    case VERIFY_CHAIN: case VERIFY_CHAIN_IO: {                      // args: has_expect, n [halt kind, halt code] | bufs: n proofs [expect] [inputs outputs]
      want(kind == VERIFY_CHAIN ? 2 : 4, (size_t)a[1] + (size_t)a[0] + (kind == VERIFY_CHAIN ? 0 : 2));
      const size_t n = (size_t)a[1];
      std::vector<const uint32_t*> ptrs(n); std::vector<uint64_t> lens(n);
      for (size_t i = 0; i < n; i++) { if (b[i].elem != 4) die("proof block"); ptrs[i] = b[i].w(); lens[i] = b[i].count; }
      zkir_public_inputs e; if (a[0]) e = expect_of(b[n]);
      if (kind == VERIFY_CHAIN) { printf("rc %d", zkir_verify_chain(ptrs.data(), lens.data(), (uint32_t)n, a[0] ? &e : nullptr)); break; }
      const Block& in = b[n + (size_t)a[0]]; const Block& out = b[n + (size_t)a[0] + 1];
      printf("rc %d", zkir_verify_chain_io(ptrs.data(), lens.data(), (uint32_t)n, a[0] ? &e : nullptr, in.q(), (size_t)in.count, out.q(), (size_t)out.count, (int)a[2], a[3]));
      break;
    }
    case VERIFY_IO: {                                               // args: has_expect, halt kind, halt code | bufs: proof [expect] inputs outputs
      want(3, 3 + (size_t)a[0]);
      zkir_public_inputs e; if (a[0]) e = expect_of(b[1]);
      const Block& in = b[1 + (size_t)a[0]]; const Block& out = b[2 + (size_t)a[0]];
      printf("rc %d", zkir_verify_io(b[0].w(), b[0].count, a[0] ? &e : nullptr, in.q(), (size_t)in.count, out.q(), (size_t)out.count, (int)a[1], a[2]));
      break;
    }
    case LOWDEG: {                                                  // args: has_root | bufs: proof [root]
      want(1, 1 + (size_t)a[0]);
      if (a[0] && b[1].count != 4) die("root block");
      printf("rc %d", zkir_lowdeg_verify(b[0].w(), b[0].count, a[0] ? b[1].w() : nullptr));
      break;
    }
    case MERKLE: {                                                  // args: width, n_leaves, flags | bufs: root, indices, openings (n_idx records of the form's length)
      want(3, 3);
      const uint64_t n_idx = b[1].count;
      uint32_t* verdicts = (uint32_t*)malloc((size_t)n_idx * 4);
      uint32_t summary[2] = {0, 0};
      const int rc = zkir_merkle_verify_host(b[0].w(), (uint32_t)a[0], a[1], b[1].q(), n_idx, b[2].w(), (uint32_t)a[2], verdicts, summary);
      if (rc) printf("error %d", rc);
      else { printf("summary %u %u verdicts", summary[0], summary[1]); for (uint64_t i = 0; i < n_idx; i++) printf(" %u", verdicts[i]); }
      free(verdicts);
      break;
    }
    case HASH_CHECK: {                                              // zkir_hash_tape_check_host | args: n_real, code_end | bufs: the section
      want(2, 1);
      zkir::HostTapes tapes;
      const zkir::TapeStages S = zkir::host_tape_stages(&tapes);
      size_t used = 0;
      const int code = S.hash_check(S.self, b[0].w(), (size_t)b[0].count, a[0], a[1], &used);
      if (code) printf("code %d", code); else printf("code 0 used %zu", used);
      break;
    }
    case TAPE_SIDE: want(0, 4); tape_side(b[0], b[1], b[2], b[3]); break;
    case NEW_BYTES: want(1, 1); new_bytes(b[0], a[0] != 0); break;
    case CALL_CELLS: {                                              // args: in_ptr, len, out_ptr, kind, cell
      want(5, 0);
      uint64_t rank = 0;
      const uint64_t n = zkir_hash_call_cells_host(a[0], a[1], a[2], (uint32_t)a[3], a[4], &rank);
      printf("cells %" PRIu64 " rank %" PRIu64 "", n, rank);
      break;
    }
    case DIGEST_BYTES: {
      want(0, 1);
      uint32_t dg[4];
      zkir_digest_bytes(b[0].b(), (size_t)b[0].count, dg);
      printf("digest %u %u %u %u", dg[0], dg[1], dg[2], dg[3]);
      break;
    }
    case INTERPRET: want(5, 2); interpret(b[0], b[1], a); break;
    case PADDED_LOG_N: {
      want(0, 1);
      printf("log_n");
      for (uint64_t i = 0; i < b[0].count; i++) printf(" %u", zkir_padded_log_n(b[0].q()[i]));
      break;
    }
    default: die("unknown case kind");
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: host_san_driver <corpus file>");
  FILE* f = fopen(argv[1], "rb");
  if (!f) die("cannot open the corpus file");
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> file((size_t)size);
  if (size && fread(file.data(), 1, (size_t)size, f) != (size_t)size) die("cannot read the corpus file");
  fclose(f);
  Reader r{file.data(), file.size()};
  if (r.u32() != 0x43534B5Au) die("not a corpus file");
  std::vector<Base> bases(r.u32());
  for (Base& b : bases) { b.elem = r.u32(); b.count = r.u64(); b.data = r.bytes((size_t)b.count * b.elem); }
  const uint32_t n_cases = r.u32();
  for (uint32_t i = 0; i < n_cases; i++) {
    const uint32_t kind = r.u32();
    std::vector<uint64_t> args(r.u32());
    for (uint64_t& x : args) x = r.u64();
    std::vector<Block> bufs;
    const uint32_t n_bufs = r.u32();
    for (uint32_t k = 0; k < n_bufs; k++) bufs.push_back(read_buf(r, bases));
    printf("%u ", i);
    g_last_error.clear();
    run_case(kind, args, bufs);
    if (!g_last_error.empty()) printf(" | %s", g_last_error.c_str());      // (what the entry point left in the last error: for the reader, not compared)
    printf("\n");
    fflush(stdout);
  }
  if (r.at != r.n) die("trailing bytes in the corpus file");
  return 0;
}
