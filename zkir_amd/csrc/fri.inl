// fri.inl — the ONE device-side FRI prover (included by stark.hip at file scope, ahead of its two callers): zkir_prove (stark_prove.inl: a STARK proof's DEEP codeword,
// log_M = log_n + 1) and the commitment layer's provers (lowdeg.inl, eval_open.inl: a combination of committed columns at any rate the context serves, log_M = log_n + b).
//
// What is here: the kernels of the FRI phase (leaf hashes, folds, the transcript step on the device, query gathering, grinding), the prover's host transcript, what a proof in
// the context's arena needs on the host side (ProofRun: pinned staging, stage events; the arena itself), and the three steps both callers run — fri_commit, fri_grind,
// fri_query_jobs.  The shape (schedule, final layer, words of a query) is fri_shape.h's, shared with the verifiers (verify.cpp).
namespace {

using bb::E4;

// ---- FRI: leaf i of a layer of size m folded k times = (c[i + t g])_{t < 2^k}, g = m >> k: 4 * 2^k base elements absorbed
// eight at a time (two extension values per permutation), as so::hash_elems does ------------------------------------------------
__global__ __launch_bounds__(NT) void fri_leaf_hash_kernel(const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ c, uint64_t m, uint32_t k, uint32_t* __restrict__ digests) {
  const uint64_t g = m >> k, i = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= g) return;
  uint32_t s[p2::T];
#pragma unroll
  for (int t = 0; t < p2::T; t++) s[t] = 0;
  const uint32_t in_scale = cp->in_scale, carry = cp->carry, ko = cp->out_scale;
  for (uint32_t u = 0; u < (1u << k); u += 2) {
#pragma unroll
    for (int t = 0; t < 4; t++) { s[t] = bb::mont_mul_lazy(c[(uint64_t)t * m + i + u * g], in_scale); s[4 + t] = bb::mont_mul_lazy(c[(uint64_t)t * m + i + (u + 1) * g], in_scale); }
#pragma unroll
    for (int t = p2::RATE; t < p2::T; t++) s[t] = bb::mont_mul_lazy(s[t], carry);
    p2::permute_scaled(s, *cp);
  }
  reinterpret_cast<uint4*>(digests)[i] = make_uint4(bb::mont_mul(s[0], ko), bb::mont_mul(s[1], ko), bb::mont_mul(s[2], ko), bb::mont_mul(s[3], ko));
}

// the same leaf hash with one permutation per quad of lanes (p2::permute_quad): small layers are latency-bound
__global__ __launch_bounds__(NT) void fri_leaf_hash_quad_kernel(const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ c, uint64_t m, uint32_t k, uint32_t* __restrict__ digests) {
  const uint64_t g = m >> k, t = (uint64_t)blockIdx.x * NT + threadIdx.x, i = t >> 2;
  const int l = (int)(t & 3);
  if (i >= g) return;                                                         // whole quads leave together
  uint32_t s[3] = {0, 0, 0};
  const uint32_t k_in = cp->in_scale, carry = cp->carry;
  for (uint32_t u = 0; u < (1u << k); u += 2) {
    s[0] = bb::mont_mul_lazy(c[(uint64_t)l * m + i + u * g], k_in); s[1] = bb::mont_mul_lazy(c[(uint64_t)l * m + i + (u + 1) * g], k_in);
    s[2] = bb::mont_mul_lazy(s[2], carry);                                     // the capacity words stay: output factor -> input factor
    p2::permute_quad_scaled(s, l, *cp);
  }
  digests[4 * i + l] = bb::mont_mul(s[0], cp->out_scale);
}

// .. and with one permutation per ROW of 16 lanes (p2::permute_row16_scaled: the shortest chain) for the smallest layers, whose few leaves wait for each other's 2^k / 2 permutations
__global__ __launch_bounds__(NT) void fri_leaf_hash_row16_kernel(const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ c, uint64_t m, uint32_t k, uint32_t* __restrict__ digests) {
  const uint64_t g = m >> k, t = (uint64_t)blockIdx.x * NT + threadIdx.x, i = t >> 4;
  const int l = (int)(t & 15);
  if (i >= g) return;                                                         // whole rows leave together
  uint32_t s = 0;
  const uint32_t k_in = cp->in_scale, carry = cp->carry;
  for (uint32_t u = 0; u < (1u << k); u += 2) {                               // words 0-3: the coordinates of value u, 4-7: of value u + 1, 8-11: the capacity (stays: output factor -> input factor)
    if (l < 4) s = bb::mont_mul_lazy(c[(uint64_t)l * m + i + u * g], k_in);
    else if (l < 8) s = bb::mont_mul_lazy(c[(uint64_t)(l - 4) * m + i + (u + 1) * g], k_in);
    else s = bb::mont_mul_lazy(s, carry);
    s = p2::permute_row16_scaled(s, l, *cp);
  }
  if (l < 4) digests[4 * i + l] = bb::mont_mul(s, cp->out_scale);
}

// one binary fold of a layer of m values: c'[i] = (c[i] + c[i+h])/2 + beta (c[i] - c[i+h]) / (2 x_i),  x_i = shift * w_m^i,  h = m / 2;
// w_m^-i = w_2N^-(i << (log_2n - log_m)), and w^-k = -w^(N-k) for 0 < k < N (w^N = -1): the table holds w^k for k < N = 2^(log_2n - 1)
// The K binary folds between two committed layers in ONE launch (round 4: three launches and two intermediate layers before): output i of the last fold depends on the 2^K
// values c[i + u g], g = m >> K, and fold f pairs v[u] with v[u + 2^(K-f-1)] — exactly the pairs (j, j + h_f) of a binary fold of the size-(m >> f) layer, the same field operations in
// the same order on every value, so the layer is the one the chain of binary folds leaves.
// beta_m: the layer's challenge and its squares, beta^(2^f) (Montgomery), written by fri_transcript_kernel on the device (round 5: no host round trip between the layers)
// ADD (a proof over codewords of several heights, mixed_eval.inl): the layer the folds leave has the size of a lower codeword, which is added to it by index before the
// layer is hashed — out[t g + i] = fold + addend[t g + i], one bb::add per coordinate.  Without ADD the addend is not read and the kernel is what it was.
struct FoldParams { uint32_t half_shift_inv_m[3]; };
template <int K, bool ADD = false>
__global__ __launch_bounds__(NT) void fri_fold_k_kernel(const uint32_t* __restrict__ c, uint32_t log_m, uint32_t log_2n, const uint32_t* __restrict__ tw_fwd, FoldParams fp, const E4* __restrict__ beta_m, uint32_t* __restrict__ out,
                                                        const uint32_t* __restrict__ addend) {
  const uint64_t m = 1ull << log_m, g = m >> K, i = (uint64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= g) return;
  E4 v[1 << K];
#pragma unroll
  for (int u = 0; u < (1 << K); u++)
#pragma unroll
    for (int t = 0; t < 4; t++) v[u].c[t] = c[(uint64_t)t * m + i + (uint64_t)u * g];
  const uint32_t N = 1u << (log_2n - 1);
  constexpr uint32_t HALF_M = (uint32_t)(((uint64_t)((bb::P + 1) / 2) * bb::R1) % bb::P);
#pragma unroll
  for (int f = 0; f < K; f++) {
    const int cnt = 1 << (K - f - 1);
#pragma unroll
    for (int u = 0; u < cnt; u++) {
      const uint64_t j = i + (uint64_t)u * g;                                  // position in the half of the size-(m >> f) domain
      const uint32_t k = (uint32_t)(j << (log_2n - (log_m - f)));
      const uint32_t winv = k == 0 ? bb::R1 : bb::neg(tw_fwd[N - k]);
      const uint32_t inv2x = bb::mont_mul(winv, fp.half_shift_inv_m[f]);
      const E4 a = v[u], b = v[u + cnt];
      const E4 sum = bb::e_mul_fm(bb::e_add(a, b), HALF_M);
      const E4 dif = bb::e_mul_fm(bb::e_sub(a, b), inv2x);
      const E4 prod = bb::e_from_mont(bb::e_mul_m(bb::e_to_mont(dif), beta_m[f]));
      v[u] = bb::e_add(sum, prod);
    }
  }
#pragma unroll
  for (int t = 0; t < 4; t++) out[(uint64_t)t * g + i] = ADD ? bb::add(v[0].c[t], addend[(uint64_t)t * g + i]) : v[0].c[t];
}
// the one launch of the K folds of a layer of 2^log_m values into `out` (addend: null, or the codeword of out's size that is added to it)
void fri_launch_fold(int k, const uint32_t* layer, uint32_t log_m, uint32_t log_2n, const uint32_t* tw_fwd, const FoldParams& fp, const E4* beta_m, uint32_t* out, const uint32_t* addend, hipStream_t s) {
  const dim3 grid(grid_for((1ull << log_m) >> k)), block(NT);
  if (!addend) {
    if (k == 1) hipLaunchKernelGGL(fri_fold_k_kernel<1>, grid, block, 0, s, layer, log_m, log_2n, tw_fwd, fp, beta_m, out, (const uint32_t*)nullptr);
    else if (k == 2) hipLaunchKernelGGL(fri_fold_k_kernel<2>, grid, block, 0, s, layer, log_m, log_2n, tw_fwd, fp, beta_m, out, (const uint32_t*)nullptr);
    else hipLaunchKernelGGL(fri_fold_k_kernel<3>, grid, block, 0, s, layer, log_m, log_2n, tw_fwd, fp, beta_m, out, (const uint32_t*)nullptr);
  } else if (k == 1) hipLaunchKernelGGL((fri_fold_k_kernel<1, true>), grid, block, 0, s, layer, log_m, log_2n, tw_fwd, fp, beta_m, out, addend);
  else if (k == 2) hipLaunchKernelGGL((fri_fold_k_kernel<2, true>), grid, block, 0, s, layer, log_m, log_2n, tw_fwd, fp, beta_m, out, addend);
  else hipLaunchKernelGGL((fri_fold_k_kernel<3, true>), grid, block, 0, s, layer, log_m, log_2n, tw_fwd, fp, beta_m, out, addend);
}

// ---- the Fiat-Shamir step of one FRI layer ON THE DEVICE: observe the layer's root, sample beta -------------------------------------------
// Challenger (below; so::Challenger) at this point of the transcript: nothing pending, so  observe(root[0..4)); sample_ext()  is ONE duplex — state words 0..3 overwritten
// with the root, one permutation, beta = (st[7], st[6], st[5], st[4]) (sample() pops from the back of the eight rate words).  One row of lanes runs it
// (p2::permute_row16_scaled: one row of 16 lanes, lane l holds word l) on the challenger state the host uploaded (Montgomery words, as Challenger::st), leaves the state for the next
// layer, and writes  out[0..4) = the root, out[4..16) = beta, beta^2, beta^4 (Montgomery: what fri_fold_k_kernel multiplies by).  The host replays the same steps from
// the roots once the whole commit phase is enqueued (the proof needs them anyway) and refuses to go on if its betas are not the device's.
__global__ void fri_transcript_kernel(const p2::Consts* __restrict__ cp, uint32_t* __restrict__ st, const uint32_t* __restrict__ root, uint32_t* __restrict__ out) {
  __shared__ uint32_t w[p2::T];
  const int l = (int)(threadIdx.x & 15);                                      // one row of 16 lanes (p2::permute_row16_scaled): lane l < 12 holds state word l
  const uint32_t k_in = bb::from_mont(cp->in_scale), ko_m = bb::to_mont(cp->out_scale);
  const uint32_t r = l < 4 ? root[l] : 0u;
  const uint32_t xm = l < 4 ? bb::to_mont(r) : l < p2::T ? st[l] : 0u;          // words 0-3 overwritten with the root, the rest of the state stays
  uint32_t s = p2::permute_row16_scaled(bb::mont_mul_lazy(xm, k_in), l, *cp);
  if (l < p2::T) { const uint32_t v = bb::mont_mul(s, ko_m); st[l] = v; w[l] = v; }
  if (l < 4) out[l] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    E4 beta{{w[7], w[6], w[5], w[4]}};
    E4* bo = reinterpret_cast<E4*>(out + 4);
    for (int f = 0; f < 3; f++) { bo[f] = beta; beta = bb::e_mul_m(beta, beta); }
  }
}

// ---- query gathering -------------------------------------------------------------------------------------------------------------
// A job (one workgroup of 64 lanes) is one of three shapes (round 5: ~750 jobs a proof instead of ~15,000 one-line copies — building and uploading that list was 90 us of host time with the GPU idle):
//   kind 0: `count` words src[k * stride] -> dst[k]                                    (a FRI leaf: the four coordinates of a value, one column apart)
//   kind 1: `count` ROW PIECES of `width` words, src[b * stride + w] -> dst[b * width + w]  (a matrix row: 8 words out of each B8 block; the quotient's 4)
//   kind 2: a MERKLE PATH — tree = src, `stride` = its number of leaves, `count` = the leaf index: the sibling digest (4 words) of every level, leaf level first
// mont: the source words rest in Montgomery form (rows of the LDE matrices) and enter the proof canonical
struct GatherJob { const uint32_t* src; uint64_t stride; uint32_t count; uint32_t dst; uint32_t mont; uint32_t kind_width; };   // kind_width = kind | width << 8
__global__ void gather_kernel(const GatherJob* __restrict__ jobs, uint32_t n_jobs, uint32_t* __restrict__ dst) {
  const uint32_t jb = blockIdx.x;
  if (jb >= n_jobs) return;
  const GatherJob g = jobs[jb];
  const uint32_t kind = g.kind_width & 0xFF, width = g.kind_width >> 8;
  if (kind == 0) {
    for (uint32_t k = threadIdx.x; k < g.count; k += blockDim.x) { const uint32_t v = g.src[(uint64_t)k * g.stride]; dst[g.dst + k] = g.mont ? bb::from_mont(v) : v; }
  } else if (kind == 1) {
    for (uint32_t k = threadIdx.x; k < g.count * width; k += blockDim.x) { const uint32_t v = g.src[(uint64_t)(k / width) * g.stride + k % width]; dst[g.dst + k] = g.mont ? bb::from_mont(v) : v; }
  } else {
    uint32_t depth = 0;
    for (uint64_t q = g.stride; q > 1; q >>= 1) depth++;
    for (uint32_t k = threadIdx.x; k < 4 * depth; k += blockDim.x) {
      const uint32_t lvl = k >> 2;                                             // level `lvl` starts 4 * (n + n/2 + .. ) = 4 * (2 n - (2 n >> lvl)) words into the tree
      const uint64_t n = g.stride, at = 4 * (2 * n - ((2 * n) >> lvl)), sib = ((uint64_t)g.count >> lvl) ^ 1;
      dst[g.dst + k] = g.src[at + 4 * sib + (k & 3)];
    }
  }
}

// ---- proof-of-work grinding: one candidate nonce per lane; the smallest hit wins (deterministic) ------------------------------
__global__ __launch_bounds__(NT) void pow_grind_kernel(const p2::Consts* __restrict__ cp, const uint32_t* __restrict__ state_m, uint32_t base, uint32_t pow_bits, uint32_t* __restrict__ best) {
  const uint32_t nonce = base + blockIdx.x * NT + threadIdx.x;
  if (nonce >= bb::P) return;
  uint32_t s[p2::T];
  const uint32_t k_in = bb::from_mont(cp->in_scale);                          // Montgomery words R v -> input words F_IN v of the throughput formulation (a fifth fewer instructions)
#pragma unroll
  for (int i = 1; i < p2::T; i++) s[i] = bb::mont_mul_lazy(state_m[i], k_in);
  s[0] = bb::mont_mul_lazy(nonce, cp->in_scale);                              // overwrite-absorb of the single pending element (canonical)
  p2::permute_scaled(s, *cp);
  if ((bb::mont_mul(s[p2::RATE - 1], cp->out_scale) & ((1u << pow_bits) - 1)) == 0) atomicMin(best, nonce);   // sample() takes the last rate element
}

// ---- host-side duplex challenger (Montgomery state; canonical in/out) -------------------------------------------------------
struct Challenger {
  const p2::Consts& c;
  uint32_t st[p2::T];
  std::vector<uint32_t> in, out;
  explicit Challenger(const p2::Consts& cc) : c(cc) { for (auto& v : st) v = 0; }
  // (round 5) the permutation in the hash kernels' formulation (p2::permute_scaled: a quarter fewer host instructions — a proof's transcript is ~330 permutations, all of
  // them on the critical path with the GPU idle); the state stays what it was: Montgomery words R v, canonical range
  void duplex() {
    for (size_t i = 0; i < in.size(); i++) st[i] = bb::to_mont(in[i]);
    in.clear();
    const uint32_t k_in = bb::from_mont(c.in_scale), ko_m = bb::to_mont(c.out_scale);
    uint32_t s[p2::T];
    for (int i = 0; i < p2::T; i++) s[i] = bb::mont_mul_lazy(st[i], k_in);
    p2::permute_scaled(s, c);
    for (int i = 0; i < p2::T; i++) st[i] = bb::mont_mul(s[i], ko_m);
    out.clear();
    for (int i = 0; i < p2::RATE; i++) out.push_back(bb::from_mont(st[i]));
  }
  void observe(uint32_t x) { out.clear(); in.push_back(x); if ((int)in.size() == p2::RATE) duplex(); }
  void observe_n(const uint32_t* x, size_t n) { for (size_t i = 0; i < n; i++) observe(x[i]); }
  uint32_t sample() { if (!in.empty() || out.empty()) duplex(); const uint32_t v = out.back(); out.pop_back(); return v; }
  E4 sample_ext() { E4 e; for (int i = 0; i < 4; i++) e.c[i] = sample(); return e; }
  uint32_t sample_bits(int b) { return sample() & ((1u << b) - 1); }
  void flush() { if (!in.empty()) duplex(); out.clear(); }                    // so::Challenger::flush
  bool check_pow(uint32_t nonce, int pow_bits) { flush(); observe(nonce); return (sample() & ((1u << pow_bits) - 1)) == 0; }
};

#define HIP_OK(expr)                                                                                         \
  do { hipError_t _e = (expr); if (_e != hipSuccess) { zkir::set_last_error({ZKIR_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)}); return ZKIR_ERR_DEVICE; } } while (0)

// Bump allocation out of the context's persistent workspace (emptied by arena_reserve at the start of every proof; the context's mutex is held).
struct Arena {
  const zkir_stark_ctx* c;
  template <typename T> hipError_t take(T** out, size_t count) {
    const size_t need = (count * sizeof(T) + 255) & ~(size_t)255;
    if (c->arena_off + need > c->arena_size) return hipErrorOutOfMemory;
    *out = (T*)(c->arena + c->arena_off);
    c->arena_off += need;
    return hipSuccess;
  }
};
struct StageEvents {             // RAII: released on every return path
  hipEvent_t ev[10]; bool on = false;
  hipError_t create() { for (auto& e : ev) { const hipError_t r = hipEventCreate(&e); if (r != hipSuccess) return r; } on = true; return hipSuccess; }
  ~StageEvents() { if (on) for (auto& e : ev) (void)hipEventDestroy(e); }
};

// ---- what a proof in the context's arena needs on the host side: pinned staging for uploads and downloads, stage events (every prover here) ---------------------------------
// The context is const to its callers (zkir_prove takes a const one): what a proof changes in it — the arena, the pinned staging, the mutex — is `mutable` there.
// Every host block of unbounded size crosses through pinned staging (host.h).  Small results the host waits for (roots, boundary states, partial sums ..) do too: a copy into
// a pageable block is served synchronously, one host round trip per copy (the kernel timeline showed 13-29 us between consecutive 16-byte copies); d2h stages them and
// sync_d2h hands them to their destinations after the ONE synchronisation that follows them.
struct ProofRun {
  const zkir_stark_ctx* c; hipStream_t s; const char* who; bool timed;
  Arena ar; zkir::HostPin& pin; StageEvents se;
  struct Staged { void* dst; const void* src; size_t n; };
  std::vector<Staged> staged;
  ProofRun(const zkir_stark_ctx* ctx, hipStream_t stream, const char* name, bool want_times) : c(ctx), s(stream), who(name), timed(want_times), ar{ctx}, pin(ctx->pin) { pin.reset(); }
  int fail(int code, const std::string& why) const { zkir::set_last_error({code, std::string(who) + ": " + why}); return code; }
  hipError_t h2d(void* dst, const void* src, size_t bytes) {
    void* p = pin.take(bytes);
    if (!p) return hipErrorOutOfMemory;
    memcpy(p, src, bytes);
    return hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, s);
  }
  hipError_t d2h(void* dst, const void* dsrc, size_t bytes) {
    void* h = pin.take(bytes);
    if (!h) return hipErrorOutOfMemory;
    staged.push_back({dst, h, bytes});
    return hipMemcpyAsync(h, dsrc, bytes, hipMemcpyDeviceToHost, s);
  }
  hipError_t sync_d2h() {
    const hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess) for (const Staged& x : staged) memcpy(x.dst, x.src, x.n);
    staged.clear();
    return e;
  }
  void mark(int i) { if (timed) (void)hipEventRecord(se.ev[i], s); }
  void times(float* stage_ms, int n) { (void)hipEventSynchronize(se.ev[n]); for (int i = 0; i < n; i++) (void)hipEventElapsedTime(&stage_ms[i], se.ev[i], se.ev[i + 1]); }
};

inline size_t arena_al(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// the context's arena holds at least `want` bytes, and is empty
int arena_reserve(const zkir_stark_ctx* c, size_t want) {
  if (c->arena_size < want) {
    if (c->arena) (void)hipFree(c->arena);
    c->arena = nullptr; c->arena_size = 0;
    HIP_OK(hipMalloc((void**)&c->arena, want));
    c->arena_size = want;
  }
  c->arena_off = 0;
  c->rate_mats[0] = c->rate_mats[1] = c->rate_mats[2] = nullptr;           // (what zkir_prove_rate left there is about to be overwritten)
  return ZKIR_OK;
}

// ---- the commit phase over a codeword of M = 2^log_M values (cw[t M + j], canonical), folded by the schedule `ks` down to n_fin values ---------------------------------------
// Enqueued as a whole: per layer  leaf hash -> tree -> fri_transcript_kernel (root -> beta on the device) -> fold;  ONE copy and ONE synchronisation at the end bring the
// roots, the betas and the final layer to the host, which replays the transcript and refuses to go on if its betas are not the device's.  `ch` is the transcript as it stands
// once the codeword's challenge is drawn (nothing pending); it leaves with the layer roots and the final layer observed.  fri_layers (ks.size() + 1 entries) and fri_trees
// (ks.size()) are filled for the queries; `words` gains what the proof carries: the layer roots, then the final layer value by value.
// addends (may be null: none; else ks.size() entries): entry j is null or a codeword of (1 << log_m_j) >> ks[j] values that is added by index to the layer fold j leaves.
int fri_commit(ProofRun& r, Challenger& ch, const std::vector<int>& ks, uint32_t log_M, uint32_t n_fin, uint32_t* codeword, std::vector<uint32_t*>& fri_layers,
               std::vector<uint32_t*>& fri_trees, std::vector<uint32_t>& words, const std::vector<const uint32_t*>* addends = nullptr) {
  const zkir_stark_ctx* c = r.c;
  hipStream_t s = r.s;
  const int n_layers = (int)ks.size();
  uint32_t fin_cols[4 * 32];                                                   // n_fin = fri_final_size(b) <= 32: a context has b <= 3
  uint32_t *dChSt, *dFri;
  HIP_OK(r.ar.take(&dChSt, 16)); HIP_OK(r.ar.take(&dFri, 16 * (size_t)(n_layers + 1)));
  fri_layers.assign(n_layers + 1, nullptr); fri_trees.assign(n_layers, nullptr);
  fri_layers[0] = codeword;
  if (!ch.in.empty()) return r.fail(ZKIR_ERR_OTHER, "the transcript has pending input at the FRI commit phase");
  HIP_OK(r.h2d(dChSt, ch.st, sizeof(ch.st)));
  uint32_t shift = bb::GEN;
  int log_m = (int)log_M;
  for (int j = 0; j < n_layers; j++) {
    const int k = ks[j];
    const uint64_t m = 1ull << log_m, g = m >> k;
    HIP_OK(r.ar.take(&fri_trees[j], 4 * (2 * g - 1)));
    uint32_t* tree = fri_trees[j];
    if (g <= (1u << 11)) hipLaunchKernelGGL(fri_leaf_hash_row16_kernel, dim3(grid_for(16 * g)), dim3(NT), 0, s, c->d_p2, fri_layers[j], m, (uint32_t)k, tree);
    else if (g <= (1u << 14)) hipLaunchKernelGGL(fri_leaf_hash_quad_kernel, dim3(grid_for(4 * g)), dim3(NT), 0, s, c->d_p2, fri_layers[j], m, (uint32_t)k, tree);
    else hipLaunchKernelGGL(fri_leaf_hash_kernel, dim3(grid_for(g)), dim3(NT), 0, s, c->d_p2, fri_layers[j], m, (uint32_t)k, tree);
    launch_tree_levels(c->d_p2, tree, g, c->sync, s);
    hipLaunchKernelGGL(fri_transcript_kernel, dim3(1), dim3(16), 0, s, c->d_p2, dChSt, tree + 4 * (2 * g - 2), dFri + 16 * j);
    FoldParams fp{};                                                           // k binary folds: beta^(2^f) (device), shift^(2^f) — one launch for all of them
    for (int f = 0; f < k; f++) {
      fp.half_shift_inv_m[f] = bb::to_mont(bb::inv(bb::mul(2, shift)));
      shift = bb::mul(shift, shift);
    }
    HIP_OK(r.ar.take(&fri_layers[j + 1], 4 * g));
    const E4* dBeta = reinterpret_cast<const E4*>(dFri + 16 * j + 4);
    fri_launch_fold(k, fri_layers[j], (uint32_t)log_m, log_M, c->d_tw_fwd, fp, dBeta, fri_layers[j + 1], addends ? (*addends)[j] : nullptr, s);
    log_m -= k;
  }
  std::vector<uint32_t> fri_out(16 * (size_t)n_layers);
  HIP_OK(r.d2h(fri_out.data(), dFri, fri_out.size() * 4));
  HIP_OK(r.d2h(fin_cols, fri_layers[n_layers], 4 * (size_t)n_fin * 4));
  HIP_OK(r.sync_d2h());
  if (check_launch(r.who) != ZKIR_OK) return ZKIR_ERR_DEVICE;
  for (int j = 0; j < n_layers; j++) {                                         // the host's replay of the device's transcript steps
    const uint32_t* out = &fri_out[16 * (size_t)j];
    ch.observe_n(out, 4);
    const E4 bm = bb::e_to_mont(ch.sample_ext());
    if (memcmp(bm.c, out + 4, 16)) return r.fail(ZKIR_ERR_OTHER, "the device's FRI transcript diverged from the host's");
    words.insert(words.end(), out, out + 4);
  }
  for (uint32_t i = 0; i < n_fin; i++) for (int t = 0; t < 4; t++) { ch.observe(fin_cols[t * n_fin + i]); words.push_back(fin_cols[t * n_fin + i]); }
  return ZKIR_OK;
}

// ---- grinding: the SMALLEST nonce whose absorption makes the next squeezed element end in pow_bits zero bits (so::Challenger::grind) — batches in rising order, the smallest
//      hit of a batch; the transcript leaves with the nonce absorbed (check_pow) ----------------------------------------------------------------------------------------------
int fri_grind(ProofRun& r, Challenger& ch, uint32_t pow_bits, uint32_t* nonce) {
  uint32_t *dState, *dBest;
  HIP_OK(r.ar.take(&dState, 16)); HIP_OK(r.ar.take(&dBest, 4));
  uint32_t pow_nonce = 0xFFFFFFFFu;
  ch.flush();
  HIP_OK(r.h2d(dState, ch.st, sizeof(ch.st)));
  const uint32_t batch = 1u << 18;
  for (uint64_t base = 0; base < bb::P && pow_nonce == 0xFFFFFFFFu; base += batch) {
    HIP_OK(hipMemsetAsync(dBest, 0xFF, 4, r.s));
    hipLaunchKernelGGL(pow_grind_kernel, dim3(batch / NT), dim3(NT), 0, r.s, r.c->d_p2, dState, (uint32_t)base, pow_bits, dBest);
    HIP_OK(r.d2h(&pow_nonce, dBest, 4));
    HIP_OK(r.sync_d2h());
  }
  if (pow_nonce == 0xFFFFFFFFu || !ch.check_pow(pow_nonce, (int)pow_bits)) return r.fail(ZKIR_ERR_OTHER, "proof-of-work search failed");
  *nonce = pow_nonce;
  return ZKIR_OK;
}

// ---- the gather jobs of ONE query's FRI layers, appended at word `off` of the query section (advanced): per layer its 2^k values, then the path of its leaf ---------------
void fri_query_jobs(std::vector<GatherJob>& jobs, uint32_t& off, uint32_t q, uint32_t log_M, const std::vector<int>& ks, const std::vector<uint32_t*>& fri_layers,
                    const std::vector<uint32_t*>& fri_trees) {
  int log_m = (int)log_M;
  for (size_t j = 0; j < ks.size(); log_m -= ks[j], j++) {
    const uint64_t m = 1ull << log_m, g = m >> ks[j], li = q & (g - 1);
    for (uint64_t u = 0; u < (1ull << ks[j]); u++) { jobs.push_back({fri_layers[j] + li + u * g, m, 4, off, 0u, 0u}); off += 4; }
    jobs.push_back({fri_trees[j], g, (uint32_t)li, off, 0u, 2u}); off += 4 * (uint32_t)(log_m - ks[j]);
  }
}

}  // namespace
