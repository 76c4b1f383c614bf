// rate_chain_san_driver.cpp — zkir_verify_rate_segment and zkir_verify_rate_chain (verify.cpp) called on a corpus of honest and malformed 'ZKSR' segment proofs and chains
// from a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_rate_chain_sanitized.py builds it, writes the corpus and compares every
// verdict with tests/rate_chain_ref.py's).  No HIP, no torch, no Python: the host objects and this file.  What the library defines in its HIP translation units is stated
// here, as in host_san_driver.cpp.
//
// Corpus file: host_san_driver.cpp's format ('ZKSC', bases, cases; a buffer = a base's prefix + patches + inline elements).  Every proof is handed to the verifier in a heap
// block of EXACTLY its length.  An expectation is 13 words: n_real (2 words, low first), entry point (2 words), mode, program digest (4), io digest (4).
//   kind 0  zkir_verify_rate_segment: args = [min_queries, min_pow_bits, 1 if an expectation follows], bufs = proof [expect]; "<case> rc <code>", on acceptance followed by
//           " states <h>", h = the fold h <- 31 h + w (mod 2^32) over the 136 state words handed out
//   kind 1  zkir_verify_rate_chain: args = [min_queries, min_pow_bits, 1 if an expectation follows, n_segments], bufs = the segments in order [expect]; "<case> rc <code>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/zkir_amd.h"
#include "../../zkir_amd/csrc/host.h"

static std::string g_last_error;
namespace zkir {
void* pinned_alloc(size_t bytes) { return malloc(bytes); }
void pinned_free(void* p) { free(p); }
void set_last_error(const Status& st) { g_last_error = st.msg; }
}  // namespace zkir
extern "C" uint32_t zkir_padded_log_n(uint64_t n_real) { uint32_t k = 3; while (((uint64_t)1 << k) < n_real) k++; return k; }

namespace {

[[noreturn]] void die(const char* what) { fprintf(stderr, "rate_chain_san_driver: %s\n", what); exit(2); }

struct Reader {
  const uint8_t* p; size_t n, at = 0;
  void need(size_t k) { if (k > n - at) die("the corpus file is cut short"); }
  uint32_t u32() { need(4); uint32_t v; memcpy(&v, p + at, 4); at += 4; return v; }
  uint64_t u64() { need(8); uint64_t v; memcpy(&v, p + at, 8); at += 8; return v; }
  const uint8_t* bytes(size_t k) { need(k); const uint8_t* q = p + at; at += k; return q; }
};

struct Base { uint64_t count; const uint8_t* data; };

// a heap block of exactly `count` words
struct Block {
  uint32_t* p = nullptr; uint64_t count = 0;
  Block() = default;
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
  Block(Block&& o) noexcept : p(o.p), count(o.count) { o.p = nullptr; }
  ~Block() { free(p); }
};

Block read_buf(Reader& r, const std::vector<Base>& bases) {
  Block out;
  if (r.u32() != 4) die("element size");
  const uint32_t base = r.u32();
  const uint64_t take = r.u64(), n_patch = r.u64();
  if (base != 0xFFFFFFFFu && (base >= bases.size() || take > bases[base].count)) die("base reference");
  if (base == 0xFFFFFFFFu && take) die("take without a base");
  const size_t patches_at = r.at;
  r.bytes((size_t)n_patch * 16);
  const uint64_t n_inline = r.u64();
  const uint8_t* inl = r.bytes((size_t)n_inline * 4);
  out.count = take + n_inline;
  out.p = (uint32_t*)malloc((size_t)out.count * 4);                 // (0 bytes: a valid pointer, nothing behind it)
  if (!out.p) die("out of memory");
  if (take) memcpy(out.p, bases[base].data, (size_t)take * 4);
  if (n_inline) memcpy(out.p + take, inl, (size_t)n_inline * 4);
  Reader pr{r.p, r.n, patches_at};
  for (uint64_t k = 0; k < n_patch; k++) {
    const uint64_t pos = pr.u64(), val = pr.u64();
    if (pos >= out.count) die("patch position");
    out.p[pos] = (uint32_t)val;
  }
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: rate_chain_san_driver CORPUS");
  FILE* f = fopen(argv[1], "rb");
  if (!f) die("cannot open the corpus");
  std::vector<uint8_t> file;
  uint8_t chunk[1 << 16];
  for (size_t k; (k = fread(chunk, 1, sizeof chunk, f)) > 0;) file.insert(file.end(), chunk, chunk + k);
  fclose(f);
  Reader r{file.data(), file.size()};
  if (r.u32() != 0x43534B5Au) die("magic");
  std::vector<Base> bases(r.u32());
  for (Base& b : bases) { if (r.u32() != 4) die("base element size"); b.count = r.u64(); b.data = r.bytes((size_t)b.count * 4); }
  const uint32_t n_cases = r.u32();
  auto expectation = [](const Block& b, zkir_public_inputs* expect) {
    if (b.count != 13) die("expectation size");
    memset(expect, 0, sizeof *expect);
    const uint32_t* e = b.p;
    expect->n_real = (uint64_t)e[0] | ((uint64_t)e[1] << 32); expect->entry_point = (uint64_t)e[2] | ((uint64_t)e[3] << 32); expect->deferred = e[4];
    memcpy(expect->program_digest, e + 5, 16); memcpy(expect->io_digest, e + 9, 16);
  };
  for (uint32_t i = 0; i < n_cases; i++) {
    const uint32_t kind = r.u32(), n_args = r.u32();
    if (kind > 1 || n_args != 3 + kind) die("case kind or argument count");
    const uint64_t min_queries = r.u64(), min_pow_bits = r.u64(), has_expect = r.u64(), n_segments = kind ? r.u64() : 1;
    const uint32_t n_bufs = r.u32();
    std::vector<Block> b;
    for (uint32_t k = 0; k < n_bufs; k++) b.push_back(read_buf(r, bases));
    if (n_bufs != n_segments + (has_expect ? 1u : 0u)) die("buffer count");
    zkir_public_inputs expect;
    if (has_expect) expectation(b[n_bufs - 1], &expect);
    if (kind == 0) {
      uint32_t st[136];
      memset(st, 0xA5, sizeof st);
      const int rc = zkir_verify_rate_segment(b[0].p, b[0].count, has_expect ? &expect : nullptr, (uint32_t)min_queries, (uint32_t)min_pow_bits, st, st + 68);
      if (rc) { printf("%u rc %d\n", i, rc); continue; }
      uint32_t h = 0;
      for (uint32_t w : st) h = 31u * h + w;
      printf("%u rc 0 states %u\n", i, h);
    } else {
      std::vector<const uint32_t*> ptrs; std::vector<uint64_t> lens;
      for (uint64_t k = 0; k < n_segments; k++) { ptrs.push_back(b[k].p); lens.push_back(b[k].count); }
      printf("%u rc %d\n", i, zkir_verify_rate_chain(ptrs.data(), lens.data(), (uint32_t)n_segments, has_expect ? &expect : nullptr, (uint32_t)min_queries, (uint32_t)min_pow_bits));
    }
  }
  return 0;
}
