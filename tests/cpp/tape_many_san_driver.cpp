// tape_many_san_driver.cpp — the host code of a mode-4 proof's tape stages over a LIST of proofs (verify.cpp: the tape locator, zkir_tape_sections_stage_host, and the
// deferring orchestration behind zkir_verify_many_tapes_host / zkir_verify_rate_many_tapes_host) called on batches of well-formed, mutated and truncated sections and
// proofs from a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_tape_many_sanitized.py builds it, writes the corpus and
// compares every line with the single-proof host verifier's verdicts and the Python reference).  No HIP, no torch, no Python: the host objects and this file.  What the
// library defines in its HIP translation units is stated here, as in host_san_driver.cpp.
//
// Corpus file: host_san_driver.cpp's format ('ZKSC', bases, cases; a buffer = a base's prefix + patches + inline elements of 1 or 4 bytes).  Every buffer — every proof
// and section of a batch — is handed over in a heap block of EXACTLY its length.  Case kinds, one line "<case index> rc <code> .." each:
//   0  zkir_tape_sections_stage_host      args: per pair n_real, code_end | bufs: per pair the hash section, the wide section, alpha, lambda
//                                          -> rc <zkir code> hv <verdicts> wv <verdicts> s <eight words per pair> d <every digest word>
//   1  zkir_verify_many_tapes_host        args: none                          | bufs: the proofs   -> rc <zkir code> v <verdicts> records <zkir_verify_tapes_last's>
//   2  zkir_verify_rate_many_tapes_host   args: per proof min_queries, min_pow_bits | bufs: the proofs   -> likewise
//   3  zkir::mem_section_locate + zkir::tape_sections_locate   args: rate (0 / 1) | bufs: one proof
//                                          -> rc 0 ok <0 / 1> [at <the hash section's offset> words <hash_words> whole <0 / 1> wide <the wide section's offset, -1: none> n <n_wide>]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/zkir_amd.h"
#include "../../include/zkir_amd_experimental.h"
#include "../../zkir_amd/csrc/host.h"
#include "../../zkir_amd/csrc/verify_stages.h"

static std::string g_last_error;
namespace zkir {
void* pinned_alloc(size_t bytes) { return malloc(bytes); }
void pinned_free(void* p) { free(p); }
void set_last_error(const Status& st) { g_last_error = st.msg; }
}  // namespace zkir
extern "C" uint32_t zkir_padded_log_n(uint64_t n_real) { uint32_t k = 3; while (((uint64_t)1 << k) < n_real) k++; return k; }

namespace {

[[noreturn]] void die(const char* what) { fprintf(stderr, "tape_many_san_driver: %s\n", what); exit(2); }

struct Reader {
  const uint8_t* p; size_t n, at = 0;
  void need(size_t k) { if (k > n - at) die("the corpus file is cut short"); }
  uint32_t u32() { need(4); uint32_t v; memcpy(&v, p + at, 4); at += 4; return v; }
  uint64_t u64() { need(8); uint64_t v; memcpy(&v, p + at, 8); at += 8; return v; }
  const uint8_t* bytes(size_t k) { need(k); const uint8_t* q = p + at; at += k; return q; }
};

struct Base { uint32_t elem; uint64_t count; const uint8_t* data; };

// a heap block of exactly `count` elements of `elem` bytes
struct Block {
  uint8_t* p = nullptr; uint64_t count = 0; uint32_t elem = 4;
  Block() = default;
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
  Block(Block&& o) noexcept : p(o.p), count(o.count), elem(o.elem) { o.p = nullptr; }
  ~Block() { free(p); }
  const uint32_t* words() const { if (elem != 4) die("a word buffer was expected"); return (const uint32_t*)p; }
};

Block read_buf(Reader& r, const std::vector<Base>& bases) {
  Block out;
  out.elem = r.u32();
  if (out.elem != 1 && out.elem != 4) die("element size");
  const uint32_t base = r.u32();
  const uint64_t take = r.u64(), n_patch = r.u64();
  if (base != 0xFFFFFFFFu && (base >= bases.size() || take > bases[base].count || bases[base].elem != out.elem)) die("base reference");
  if (base == 0xFFFFFFFFu && take) die("take without a base");
  const size_t patches_at = r.at;
  r.bytes((size_t)n_patch * 16);
  const uint64_t n_inline = r.u64();
  const uint8_t* inl = r.bytes((size_t)n_inline * out.elem);
  out.count = take + n_inline;
  out.p = (uint8_t*)malloc((size_t)out.count * out.elem);           // (0 bytes: a valid pointer, nothing behind it)
  if (!out.p) die("out of memory");
  if (take) memcpy(out.p, bases[base].data, (size_t)take * out.elem);
  if (n_inline) memcpy(out.p + take * out.elem, inl, (size_t)n_inline * out.elem);
  Reader pr{r.p, r.n, patches_at};
  for (uint64_t k = 0; k < n_patch; k++) {
    const uint64_t pos = pr.u64(), val = pr.u64();
    if (pos >= out.count) die("patch position");
    if (out.elem == 4) { const uint32_t v = (uint32_t)val; memcpy(out.p + 4 * pos, &v, 4); } else out.p[pos] = (uint8_t)val;
  }
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: tape_many_san_driver CORPUS");
  FILE* f = fopen(argv[1], "rb");
  if (!f) die("cannot open the corpus");
  std::vector<uint8_t> file;
  uint8_t chunk[1 << 16];
  for (size_t k; (k = fread(chunk, 1, sizeof chunk, f)) > 0;) file.insert(file.end(), chunk, chunk + k);
  fclose(f);
  Reader r{file.data(), file.size()};
  if (r.u32() != 0x43534B5Au) die("magic");
  std::vector<Base> bases(r.u32());
  for (Base& b : bases) { b.elem = r.u32(); if (b.elem != 1 && b.elem != 4) die("base element size"); b.count = r.u64(); b.data = r.bytes((size_t)b.count * b.elem); }
  const uint32_t n_cases = r.u32();
  for (uint32_t i = 0; i < n_cases; i++) {
    const uint32_t kind = r.u32(), n_args = r.u32();
    std::vector<uint64_t> args(n_args);
    for (uint64_t& x : args) x = r.u64();
    const uint32_t n_bufs = r.u32();
    std::vector<Block> b;
    for (uint32_t k = 0; k < n_bufs; k++) b.push_back(read_buf(r, bases));
    if (kind == 0) {
      const uint32_t n = n_bufs / 4;
      if (n_bufs != 4 * n || n_args != 2 * n) die("stage case");
      std::vector<const uint32_t*> hs(n), ws(n); std::vector<uint64_t> hw(n), ww(n), n_real(n), code_end(n); std::vector<uint32_t> al(4 * (size_t)n), la(4 * (size_t)n);
      size_t chunks = 0;
      for (uint32_t k = 0; k < n; k++) {
        if (b[4 * k + 2].count != 4 || b[4 * k + 3].count != 4) die("stage case buffers");
        hs[k] = b[4 * k].words(); hw[k] = b[4 * k].count; ws[k] = b[4 * k + 1].words(); ww[k] = b[4 * k + 1].count; n_real[k] = args[2 * k]; code_end[k] = args[2 * k + 1];
        memcpy(&al[4 * (size_t)k], b[4 * k + 2].words(), 16); memcpy(&la[4 * (size_t)k], b[4 * k + 3].words(), 16);
        chunks += (size_t)((hw[k] + 511) / 512 + (ww[k] + 511) / 512);
      }
      // (the outputs in heap blocks of exactly their lengths too)
      int32_t* hv = (int32_t*)malloc(4 * (size_t)n); int32_t* wv = (int32_t*)malloc(4 * (size_t)n); uint32_t* dg = (uint32_t*)malloc(16 * chunks); uint32_t* sums = (uint32_t*)malloc(32 * (size_t)n);
      if ((n && (!hv || !wv || !sums)) || (chunks && !dg)) die("out of memory");
      if (n) { memset(hv, 0xFF, 4 * (size_t)n); memset(wv, 0xFF, 4 * (size_t)n); memset(sums, 0xFF, 32 * (size_t)n); }
      if (chunks) memset(dg, 0xFF, 16 * chunks);
      const int rc = zkir_tape_sections_stage_host(hs.data(), hw.data(), ws.data(), ww.data(), n_real.data(), code_end.data(), al.data(), la.data(), n, hv, wv, dg, sums);
      printf("%u rc %d", i, rc);
      if (rc == 0) {
        printf(" hv"); for (uint32_t k = 0; k < n; k++) printf(" %d", hv[k]);
        printf(" wv"); for (uint32_t k = 0; k < n; k++) printf(" %d", wv[k]);
        printf(" s"); for (uint32_t k = 0; k < 8 * n; k++) printf(" %u", sums[k]);
        printf(" d"); for (size_t k = 0; k < 4 * chunks; k++) printf(" %u", dg[k]);
      }
      printf("\n");
      free(hv); free(wv); free(dg); free(sums);
    } else if (kind == 3) {
      if (n_bufs != 1 || n_args != 1) die("locate case");
      const zkir::MemLocated ml = zkir::mem_section_locate(b[0].words(), b[0].count, args[0] != 0);
      const zkir::TapeLocated tl = zkir::tape_sections_locate(b[0].words(), b[0].count, ml);
      printf("%u rc 0 ok %d", i, tl.ok ? 1 : 0);
      if (tl.ok) printf(" at %lld words %llu whole %d wide %lld n %llu", (long long)(tl.sec.hash - b[0].words()), (unsigned long long)tl.sec.hash_words, tl.sec.whole ? 1 : 0,
                        tl.sec.wide ? (long long)(tl.sec.wide - b[0].words()) : -1ll, (unsigned long long)tl.sec.n_wide);
      printf("\n");
    } else if (kind == 1 || kind == 2) {
      const uint32_t n = n_bufs;
      if (n_args != (kind == 2 ? 2 * n : 0)) die("verify case");
      std::vector<const uint32_t*> proofs(n); std::vector<uint64_t> lens(n); std::vector<uint32_t> mq(n), mb(n);
      for (uint32_t k = 0; k < n; k++) { proofs[k] = b[k].words(); lens[k] = b[k].count; if (kind == 2) { mq[k] = (uint32_t)args[2 * k]; mb[k] = (uint32_t)args[2 * k + 1]; } }
      int32_t* v = (int32_t*)malloc(4 * (size_t)n);
      if (n && !v) die("out of memory");
      if (n) memset(v, 0xFF, 4 * (size_t)n);
      const int rc = kind == 1 ? zkir_verify_many_tapes_host(proofs.data(), lens.data(), nullptr, n, v)
                               : zkir_verify_rate_many_tapes_host(proofs.data(), lens.data(), nullptr, mq.data(), mb.data(), n, v);
      uint64_t cells = 0;
      zkir_verify_tapes_last(&cells, nullptr, nullptr);
      printf("%u rc %d", i, rc);
      if (rc == 0) { printf(" v"); for (uint32_t k = 0; k < n; k++) printf(" %d", v[k]); printf(" records %llu", (unsigned long long)cells); }
      printf("\n");
      free(v);
    } else die("case kind");
  }
  return 0;
}
