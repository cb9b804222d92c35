// Repetition penalty over per-prompt token sets (gfx950): vsel_token_sets_build, vsel_repetition_penalty.  HF's
// RepetitionPenaltyLogitsProcessor restated per row: in fp32, y_i = x_i < 0 ? x_i * theta : x_i * inv for i in the
// row's set, y_i = x_i elsewhere (theta = (float)penalty, inv = (float)(1 / penalty) from the double penalty, as torch computes it);
// then the greedy token argmax(y) (torch.argmax's order: NaN above everything, equal values -- +0 and -0 included -- to the lowest
// index) and / or y itself, for the sampler.
//   sets   one bitset per prompt, uint32 [n_sets, ceil(V / 32)].  Build: one workgroup per set zeroes its words, then ORs in the set's
//          ids with global atomics (ids outside [0, V) are skipped).
//   step   one 1024-thread workgroup per row (grid = batch), no workspace, no communication between workgroups.  The row's previous
//          token (optional) counts as a member during the launch and is ORed into the row's set at its end; row ids are distinct within
//          a launch, so no two workgroups touch one set.  16-byte loads on the 16-byte-aligned body of the row, scalar head and tail
//          (as csrc/sample.hip), so odd vocabularies and strided rows take the same path.
#include <cmath>

#include "common.h"

namespace vsel {

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr int kBuildThreads = 256;

__global__ __launch_bounds__(kBuildThreads) void token_sets_build_kernel(const int64_t* ids, const int64_t* cu, int64_t vocab,
                                                                          int64_t words, uint32_t* sets) {
  const int64_t s = blockIdx.x;
  uint32_t* set = sets + s * words;
  for (int64_t w = threadIdx.x; w < words; w += kBuildThreads) set[w] = 0u;
  __threadfence();                                       // the zeros reach L2, where the atomics below run, before any of them
  __syncthreads();
  const int64_t end = cu[s + 1];
  for (int64_t j = cu[s] + threadIdx.x; j < end; j += kBuildThreads) {
    const int64_t id = ids[j];
    if (id >= 0 && id < vocab) atomicOr(&set[id >> 5], 1u << (id & 31));
  }
}

struct PenaltyArgs {
  const void* logits;
  int64_t vocab, row_stride, words, n_sets;
  float theta, inv_theta;
  uint32_t* sets;
  const int64_t* row_ids;
  const int64_t* prev;
  int64_t* tokens;
  float* out;
};

// raw element -> fp32
template <typename T> struct Load;
template <> struct Load<bf16_t> {
  static constexpr int kVec = 8;
  static __device__ __forceinline__ float scalar(const void* p, int64_t i) { return bf16_to_f32(static_cast<const uint16_t*>(p)[i]); }
  static __device__ __forceinline__ u32x4 raw(const void* p, int64_t i) {
    return *reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(p) + i);
  }
  static __device__ __forceinline__ float elem(const u32x4& r, int t) {
    return __uint_as_float((t & 1) ? (r[t >> 1] & 0xffff0000u) : (r[t >> 1] << 16));
  }
};
template <> struct Load<float> {
  static constexpr int kVec = 4;
  static __device__ __forceinline__ float scalar(const void* p, int64_t i) { return static_cast<const float*>(p)[i]; }
  static __device__ __forceinline__ u32x4 raw(const void* p, int64_t i) {
    return *reinterpret_cast<const u32x4*>(static_cast<const float*>(p) + i);
  }
  static __device__ __forceinline__ float elem(const u32x4& r, int t) { return __uint_as_float(r[t]); }
};

// torch.argmax's order as an unsigned key: NaN above everything, -0 folded onto +0 (they are equal), order-preserving otherwise.
// Every key of a non-NaN value is > 0, so 0 is below all of them.
__device__ __forceinline__ uint32_t argmax_key(float y) {
  uint32_t u = __float_as_uint(y);
  u = u == 0x80000000u ? 0u : u;
  const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return isnan(y) ? 0xffffffffu : k;
}
// (key, index) pairs of different threads: the larger key, equal keys to the lower index
__device__ __forceinline__ bool beats(uint32_t k, int i, uint32_t bk, int bi) { return k > bk || (k == bk && i < bi); }

template <typename T>
__global__ __launch_bounds__(kThreads) void repetition_penalty_kernel(PenaltyArgs a) {
  using L = Load<T>;
  constexpr int V = L::kVec;
  constexpr int64_t esz = sizeof(T);
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const void* row = static_cast<const char*>(a.logits) + r * a.row_stride * esz;
  const int64_t vocab = a.vocab;
  const int64_t sid = a.row_ids ? a.row_ids[r] : r;
  // a row id outside [0, n_sets) reads as the empty set and is never written (device values are not trusted with addresses)
  const uint32_t* set = sid >= 0 && sid < a.n_sets ? a.sets + sid * a.words : nullptr;
  const int64_t prev = a.prev ? a.prev[r] : -1;
  float* out = a.out ? a.out + r * vocab : nullptr;
  const bool want_tok = a.tokens != nullptr;
  const float theta = a.theta, inv = a.inv_theta;

  // each thread visits its elements in increasing index order (head, body, tail), so a later element must be strictly larger to win
  uint32_t best = 0u;
  int best_i = INT32_MAX;
  auto penalize = [&](float x, bool member) { return member ? (x < 0.0f ? x * theta : x * inv) : x; };
  auto take = [&](float y, int64_t i) {
    const uint32_t k = argmax_key(y);
    if (k > best) { best = k; best_i = (int)i; }
  };
  auto scalar = [&](int64_t i) {
    const bool member = i == prev || (set && ((set[i >> 5] >> (i & 31)) & 1u));
    const float y = penalize(L::scalar(row, i), member);
    if (out) out[i] = y;
    if (want_tok) take(y, i);
  };

  const int64_t mis = (int64_t)((uintptr_t)row & 15);
  const int64_t head = min(vocab, mis ? (16 - mis) / esz : (int64_t)0);
  const int64_t nvec = (vocab - head) / V;
  const int64_t body_end = head + nvec * V;
  // head (< V elements), one element per thread
  if (tid < head) scalar(tid);
  // body: 16 bytes of logits and the (at most two) bitset words that cover them per vector; two vectors in flight per thread
  const bool out_vec = out && (((uintptr_t)(out + head)) & 15) == 0;      // body stores 16-byte aligned (uniform over the row)
  auto member_bits = [&](int64_t i0) -> uint32_t {
    if (!set) return 0u;
    const int64_t w0 = i0 >> 5;
    const int sh = (int)(i0 & 31);
    const uint64_t lo = set[w0];
    const uint64_t hi = sh + V > 32 ? (uint64_t)set[w0 + 1] : 0ull;         // w0 + 1 holds element i0 + V - 1 < vocab
    return (uint32_t)(((hi << 32) | lo) >> sh) & ((1u << V) - 1u);
  };
  auto process = [&](int64_t i0, const u32x4& raw, uint32_t bits) {
    float y[V];
#pragma unroll
    for (int t = 0; t < V; ++t) {
      const int64_t i = i0 + t;
      y[t] = penalize(L::elem(raw, t), ((bits >> t) & 1u) || i == prev);
      if (want_tok) take(y[t], i);
    }
    if (out_vec) {
#pragma unroll
      for (int t = 0; t < V; t += 4) *reinterpret_cast<f32x4*>(out + i0 + t) = f32x4{y[t], y[t + 1], y[t + 2], y[t + 3]};
    } else if (out) {
#pragma unroll
      for (int t = 0; t < V; ++t) out[i0 + t] = y[t];
    }
  };
  for (int64_t v0 = 0; v0 < nvec; v0 += 2 * kThreads) {
    const int64_t va = v0 + tid, vb = va + kThreads;
    const bool ok_a = va < nvec, ok_b = vb < nvec;
    const int64_t ia = head + va * V, ib = head + vb * V;
    u32x4 ra = {0u, 0u, 0u, 0u}, rb = {0u, 0u, 0u, 0u};
    uint32_t ma = 0u, mb = 0u;
    if (ok_a) { ra = L::raw(row, ia); ma = member_bits(ia); }
    if (ok_b) { rb = L::raw(row, ib); mb = member_bits(ib); }
    if (ok_a) process(ia, ra, ma);
    if (ok_b) process(ib, rb, mb);
  }
  // tail (< V elements), one element per thread, after the body (index order)
  if (tid < vocab - body_end) scalar(body_end + tid);

  if (want_tok) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t ob = __shfl_xor(best, o, kWave);
      const int oi = __shfl_xor(best_i, o, kWave);
      if (beats(ob, oi, best, best_i)) { best = ob; best_i = oi; }
    }
    __shared__ uint32_t red_k[kWaves];
    __shared__ int red_i[kWaves];
    if (lane == 0) { red_k[wave] = best; red_i[wave] = best_i; }
    __syncthreads();
    if (tid == 0) {
      uint32_t bb = red_k[0];
      int bi = red_i[0];
      for (int w = 1; w < kWaves; ++w)
        if (beats(red_k[w], red_i[w], bb, bi)) { bb = red_k[w]; bi = red_i[w]; }
      a.tokens[r] = bi;
    }
  }
  // the previous token joins the set for the launches that follow (this launch already counted it)
  if (tid == 0 && set && prev >= 0 && prev < vocab) atomicOr(a.sets + sid * a.words + (prev >> 5), 1u << (prev & 31));
}

}  // namespace

}  // namespace vsel

using namespace vsel;

extern "C" int vsel_token_sets_build(void* stream, const int64_t* ids, const int64_t* cu, int64_t n_sets, int64_t vocab, uint32_t* sets) {
  if (!ids || !cu || !sets) return fail(VSEL_ERR_INVALID, "NULL ids / cu / sets");
  if (n_sets < 0 || vocab < 1) return fail(VSEL_ERR_INVALID, "bad shape (n_sets=%lld vocab=%lld)", (long long)n_sets, (long long)vocab);
  if (vocab >= (1ll << 31)) return fail(VSEL_ERR_UNSUPPORTED, "vocab %lld >= 2^31", (long long)vocab);
  if (n_sets > INT32_MAX) return fail(VSEL_ERR_UNSUPPORTED, "n_sets %lld > 2^31 - 1", (long long)n_sets);
  if (n_sets == 0) return VSEL_OK;
  hipStream_t st = (hipStream_t)stream;
  VSEL_LAUNCH(token_sets_build_kernel, dim3((unsigned)n_sets), dim3(kBuildThreads), 0, st, ids, cu, vocab, (vocab + 31) / 32, sets);
  VSEL_AFTER_LAUNCH(st, "token_sets_build_kernel");
  return VSEL_OK;
}

extern "C" int vsel_repetition_penalty(void* stream, const void* logits, vsel_dtype dtype, int64_t batch, int64_t vocab, int64_t row_stride,
                                       double penalty, uint32_t* sets, int64_t n_sets, const int64_t* row_ids, const int64_t* prev_tokens,
                                       int64_t* tokens, float* out) {
  if (!logits || !sets) return fail(VSEL_ERR_INVALID, "NULL logits / sets");
  if (!tokens && !out) return fail(VSEL_ERR_INVALID, "no output requested (tokens and out are both NULL)");
  if (dtype != VSEL_BF16 && dtype != VSEL_F32) return fail(VSEL_ERR_INVALID, "dtype must be bf16 or f32");
  if (!(penalty > 0.0) || !std::isfinite(penalty) || !((float)penalty > 0.0f) || !std::isfinite((float)penalty))
    return fail(VSEL_ERR_INVALID, "penalty %g must be finite and > 0 (also as float32)", penalty);
  if (vocab < 1 || batch < 0 || row_stride < vocab || n_sets < 0)
    return fail(VSEL_ERR_INVALID, "bad shape (batch=%lld vocab=%lld row_stride=%lld n_sets=%lld)", (long long)batch, (long long)vocab,
                (long long)row_stride, (long long)n_sets);
  if (vocab >= (1ll << 31)) return fail(VSEL_ERR_UNSUPPORTED, "vocab %lld >= 2^31", (long long)vocab);
  if (batch > INT32_MAX) return fail(VSEL_ERR_UNSUPPORTED, "batch %lld > 2^31 - 1", (long long)batch);
  if (batch == 0) return VSEL_OK;

  PenaltyArgs a{};
  a.logits = logits;
  a.vocab = vocab;
  a.row_stride = row_stride;
  a.words = (vocab + 31) / 32;
  a.n_sets = n_sets;
  // torch's GPU kernels on a float tensor and a Python scalar (a double): x * theta multiplies by (float)theta; x / theta multiplies by
  // the reciprocal taken in double and rounded once, (float)(1 / theta) -- not 1.0f / (float)theta, which differs by an ulp for some theta
  a.theta = (float)penalty;
  a.inv_theta = (float)(1.0 / penalty);
  a.sets = sets;
  a.row_ids = row_ids;
  a.prev = prev_tokens;
  a.tokens = tokens;
  a.out = out;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VSEL_BF16) {
    VSEL_LAUNCH(repetition_penalty_kernel<bf16_t>, dim3((unsigned)batch), dim3(kThreads), 0, st, a);
  } else {
    VSEL_LAUNCH(repetition_penalty_kernel<float>, dim3((unsigned)batch), dim3(kThreads), 0, st, a);
  }
  VSEL_AFTER_LAUNCH(st, "repetition_penalty_kernel");
  return VSEL_OK;
}
