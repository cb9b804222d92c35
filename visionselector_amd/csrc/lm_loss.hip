// Fused LM cross-entropy over [rows, vocab] logits (gfx950): vsel_token_logprob_fwd, vsel_token_logprob_bwd.
//   forward   per row r with target t: lse = log sum_j exp(x_j), logprob = x_t - lse.  One 1024-thread workgroup per row (grid = rows),
//             no workspace, no communication between workgroups: a row's bits depend on its logits and target alone.  One streaming pass:
//             every thread keeps an online (max, sum) over its elements in fp32, the block then takes the row max, every thread rescales
//             its sum to it once, and the 1024 sums are added in fp64 in a fixed order; lse = (float)(max + log(sum)) and
//             logprob = (float)(x_t - (max + log(sum))) are each rounded once from fp64.  exp() is v_exp_f32 on a product whose
//             rounding error is carried along (exp_acc), so that a term is good to about an ulp; rows of at most 4096 elements, one
//             chunk per thread, take their terms in fp64 against the row max instead.  A row whose target is ignore_index
//             exits before reading a logit; a target outside [0, vocab) gives NaN the same way.
//   sum       a second one-workgroup launch adds logprob over the rows (fp64, fixed order documented in include/vsel.h) and counts the
//             rows that are not ignored: no float atomics anywhere.
//   backward  grad[r, j] = c_r ([j == t] - exp(x_j - lse_r)), one rounding to the output dtype; bf16 rows in fp32, fp32 rows in fp64
//             (x_j - lse_r rounded to fp32 alone is worth several fp32 ulps of the result).  Ignored and out-of-range rows are
//             zero-filled without reading their logits.
// 16-byte non-temporal loads.  The forward cuts a row into 8-element (fp32: 4-element) chunks by element index, so that its sums do not
// depend on the row's address: an aligned row loads a chunk at once, a misaligned one (odd vocabulary or stride) element by element.
// The backward is element-wise: 16-byte-aligned body, scalar head and tail (as csrc/sample.hip).  All element offsets are 64-bit.
#include <cmath>

#include "common.h"

// no fused multiply-adds but the ones written out: a row's bits must not depend on which copy of the arithmetic a path runs through
#pragma clang fp contract(off)

namespace vsel {

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr int64_t kSmallVocab = 4096;                  // <= kThreads chunks of either dtype

template <typename T> struct Row;
template <> struct Row<bf16_t> {
  static constexpr int kVec = 8;
  static __device__ __forceinline__ float scalar(const void* p, int64_t i) { return bf16_to_f32(static_cast<const uint16_t*>(p)[i]); }
  static __device__ __forceinline__ void vec(const void* p, int64_t i, float (&v)[8]) {
    load_vec_stream(reinterpret_cast<const bf16_t*>(static_cast<const uint16_t*>(p) + i), v);
  }
};
template <> struct Row<float> {
  static constexpr int kVec = 4;
  static __device__ __forceinline__ float scalar(const void* p, int64_t i) { return static_cast<const float*>(p)[i]; }
  static __device__ __forceinline__ void vec(const void* p, int64_t i, float (&v)[4]) { load_vec_stream(static_cast<const float*>(p) + i, v); }
};

// head / body / tail split of a row around its 16-byte-aligned part
template <typename T>
struct Split {
  int64_t head, nvec, body_end;
  __device__ __forceinline__ Split(const void* row, int64_t vocab) {
    constexpr int64_t esz = sizeof(T);
    const int64_t mis = (int64_t)((uintptr_t)row & 15);
    head = min(vocab, mis ? (16 - mis) / esz : (int64_t)0);
    nvec = (vocab - head) / Row<T>::kVec;
    body_end = head + nvec * Row<T>::kVec;
  }
};

// exp(a) for a <= 0 (NaN stays NaN, -inf and anything below -200 give 0): v_exp_f32 of t = a * log2(e), times 1 + ln2 * (the part of
// a * log2(e) that t's rounding and the fp32 constant left out).  Error about one ulp instead of |a| * 2^-24 relative.
__device__ __forceinline__ float exp_acc(float a) {
  constexpr float kL2eHi = 0x1.715476p+0f, kL2eLo = 0x1.4ae0c0p-26f, kLn2 = 0x1.62e430p-1f;
  a = a < -200.0f ? -200.0f : a;                      // (a select, not fmaxf: a NaN must come through)
  const float t = a * kL2eHi;
  const float r = fmaf(a, kL2eLo, fmaf(a, kL2eHi, -t));
  const float e = __builtin_amdgcn_exp2f(t);
  return fmaf(e, r * kLn2, e);
}

struct FwdArgs {
  const void* logits;
  int64_t vocab, row_stride, ignore_index;
  const int64_t* targets;
  float* logprob;
  float* lse;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void token_logprob_fwd_kernel(FwdArgs a) {
  using R = Row<T>;
  constexpr int V = R::kVec;
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t vocab = a.vocab;
  const int64_t tgt = a.targets[r];
  if (tgt == a.ignore_index || tgt < 0 || tgt >= vocab) {            // uniform over the block; no logit is read
    if (tid == 0) {
      const float v = tgt == a.ignore_index ? 0.0f : __builtin_nanf("");
      a.logprob[r] = v;
      a.lse[r] = v;
    }
    return;
  }
  const void* row = static_cast<const char*>(a.logits) + r * a.row_stride * (int64_t)sizeof(T);

  // The row is cut into chunks of V elements BY ELEMENT INDEX, chunk c goes to thread c % 1024, and a thread takes its chunks in
  // ascending order: which element meets which in the sums does not depend on where the row lies in memory.  A chunk of a 16-byte
  // aligned row is one 16-byte load; the last, partial chunk and every chunk of a misaligned row (an odd vocabulary or stride) are
  // element loads, padded with -inf, which adds exactly +0.
  // online (m, s): s = sum exp(x - m) over the elements seen so far, m their max (-inf: none finite yet, s = 0)
  float m = -INFINITY, s = 0.0f;
  auto chunk = [&](const float (&x)[V]) {
    float vm = x[0];
#pragma unroll
    for (int t = 1; t < V; ++t) vm = fmaxf(vm, x[t]);
    if (vm > m) {
      if (m != -INFINITY) s *= exp_acc(m - vm);
      m = vm;
    }
    const float mu = m == -INFINITY ? 0.0f : m;
#pragma unroll
    for (int t = 0; t < V; ++t) s += exp_acc(x[t] - mu);
  };
  const bool aligned = ((uintptr_t)row & 15) == 0;
  const int64_t nchunk = (vocab + V - 1) / V;
  auto load = [&](int64_t c, float (&x)[V]) {
    const int64_t i0 = c * V;
    if (aligned && i0 + V <= vocab) {
      R::vec(row, i0, x);
    } else {
#pragma unroll
      for (int t = 0; t < V; ++t) x[t] = i0 + t < vocab ? R::scalar(row, i0 + t) : -INFINITY;
    }
  };
  // Up to kSmallVocab elements a thread holds at most one chunk: it keeps the chunk, and its terms are taken in fp64 against the row
  // max below.  (With a handful of terms the ulp of every fp32 exp() shows in the sum; over a long row those errors average out.)
  const bool small = vocab <= kSmallVocab;
  float xs[V];
  if (small) {
#pragma unroll
    for (int t = 0; t < V; ++t) xs[t] = -INFINITY;
    if (tid < nchunk) load(tid, xs);
#pragma unroll
    for (int t = 0; t < V; ++t) m = fmaxf(m, xs[t]);
  } else {
    for (int64_t c0 = 0; c0 < nchunk; c0 += 2 * kThreads) {           // two chunks in flight per thread
      const int64_t ca = c0 + tid, cb = ca + kThreads;
      const bool ok_a = ca < nchunk, ok_b = cb < nchunk;
      float xa[V], xb[V];
      if (ok_a) load(ca, xa);
      if (ok_b) load(cb, xb);
      if (ok_a) chunk(xa);
      if (ok_b) chunk(xb);
    }
  }

  __shared__ float red_m[kWaves];
  __shared__ double red_s[kWaves];
  const float wm = wave_max(m);
  if (lane == 0) red_m[wave] = wm;
  __syncthreads();
  float mx = red_m[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) mx = fmaxf(mx, red_m[w]);
  // every thread's sum at the row max (a thread that saw nothing finite holds 0, or NaN), then fp64: lanes by a butterfly, waves in order
  double sd = 0.0;
  if (small) {
#pragma unroll
    for (int t = 0; t < V; ++t) sd += exp((double)xs[t] - (double)mx);
  } else {
    sd = (double)(m == -INFINITY ? s : s * exp_acc(m - mx));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sd += __shfl_xor(sd, o, kWave);
  if (lane == 0) red_s[wave] = sd;
  __syncthreads();
  if (tid == 0) {
    double tot = red_s[0];
    for (int w = 1; w < kWaves; ++w) tot += red_s[w];
    // a +inf in the row made x - m NaN for that entry; no finite entry at all leaves mx = -inf
    const double l = mx == -INFINITY ? (double)__builtin_nanf("") : (double)mx + log(tot);
    a.lse[r] = (float)l;
    a.logprob[r] = (float)((double)R::scalar(row, tgt) - l);
  }
}

// sum_out = the sum of logprob over the rows, n_valid = the rows whose target is not ignore_index.  Order (include/vsel.h): thread i
// adds rows i, i + 1024, ... in fp64, then the 1024 partials are folded in halves (p[i] += p[i + h], h = 512 .. 1).
__global__ __launch_bounds__(kThreads) void token_logprob_sum_kernel(const float* logprob, const int64_t* targets, int64_t rows,
                                                                     int64_t ignore_index, float* sum_out, int32_t* n_valid_out) {
  __shared__ double p[kThreads];
  __shared__ int cnt[kThreads];
  const int tid = threadIdx.x;
  double acc = 0.0;
  int n = 0;
  for (int64_t i = tid; i < rows; i += kThreads) {
    acc += (double)logprob[i];
    n += targets[i] != ignore_index;
  }
  p[tid] = acc;
  cnt[tid] = n;
  __syncthreads();
  for (int h = kThreads / 2; h > 0; h >>= 1) {
    if (tid < h) {
      p[tid] += p[tid + h];
      cnt[tid] += cnt[tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (sum_out) sum_out[0] = (float)p[0];
    if (n_valid_out) n_valid_out[0] = cnt[0];
  }
}

struct BwdArgs {
  const void* logits;
  int64_t vocab, row_stride, ignore_index;
  const int64_t* targets;
  const float* lse;
  const float* grad_rows;
  const float* grad_scale;
  void* grad;
};

// one gradient element; bf16 rows in fp32, fp32 rows in fp64
template <typename T> struct Grad;
template <> struct Grad<bf16_t> {
  using Acc = float;
  static __device__ __forceinline__ float at(float x, float lse, float c, bool hit) {
    return c * ((hit ? 1.0f : 0.0f) - exp2f((x - lse) * 0x1.715476p+0f));
  }
};
template <> struct Grad<float> {
  using Acc = double;
  static __device__ __forceinline__ float at(float x, double lse, double c, bool hit) {
    return (float)(c * ((hit ? 1.0 : 0.0) - exp((double)x - lse)));
  }
};

template <typename T>
__global__ __launch_bounds__(kThreads) void token_logprob_bwd_kernel(BwdArgs a) {
  using R = Row<T>;
  using G = Grad<T>;
  using Acc = typename G::Acc;
  constexpr int V = R::kVec;
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t vocab = a.vocab;
  const int64_t tgt = a.targets[r];
  T* out = static_cast<T*>(a.grad) + r * vocab;
  if (tgt == a.ignore_index || tgt < 0 || tgt >= vocab) {            // zero row, split around the OUTPUT's 16-byte-aligned part
    const Split<T> so(out, vocab);
    const float z[V] = {};
    if (tid < so.head) store_elem(out + tid, 0.0f);
    for (int64_t v = tid; v < so.nvec; v += kThreads) store_vec(out + so.head + v * V, z);
    if (tid < vocab - so.body_end) store_elem(out + so.body_end + tid, 0.0f);
    return;
  }
  const void* row = static_cast<const char*>(a.logits) + r * a.row_stride * (int64_t)sizeof(T);
  const Split<T> sp(row, vocab);
  const Acc lse = (Acc)a.lse[r];
  const Acc c = (Acc)(a.grad_rows ? a.grad_rows[r] : 1.0f) * (Acc)(a.grad_scale ? a.grad_scale[0] : 1.0f);
  auto one = [&](int64_t i) { store_elem(out + i, G::at(R::scalar(row, i), lse, c, i == tgt)); };
  if (tid < sp.head) one(tid);
  const bool out_vec = (((uintptr_t)(out + sp.head)) & 15) == 0;     // body stores 16-byte aligned (uniform over the row)
  auto body = [&](int64_t i0, const float (&x)[V]) {
    float g[V];
#pragma unroll
    for (int t = 0; t < V; ++t) g[t] = G::at(x[t], lse, c, i0 + t == tgt);
    if (out_vec) {
      store_vec(out + i0, g);
    } else {
#pragma unroll
      for (int t = 0; t < V; ++t) store_elem(out + i0 + t, g[t]);
    }
  };
  for (int64_t v0 = 0; v0 < sp.nvec; v0 += 2 * kThreads) {
    const int64_t va = v0 + tid, vb = va + kThreads;
    const bool ok_a = va < sp.nvec, ok_b = vb < sp.nvec;
    float xa[V], xb[V];
    if (ok_a) R::vec(row, sp.head + va * V, xa);
    if (ok_b) R::vec(row, sp.head + vb * V, xb);
    if (ok_a) body(sp.head + va * V, xa);
    if (ok_b) body(sp.head + vb * V, xb);
  }
  if (tid < vocab - sp.body_end) one(sp.body_end + tid);
}

int check_rows(const void* logits, const int64_t* targets, vsel_dtype dtype, int64_t rows, int64_t vocab, int64_t row_stride) {
  if (!logits || !targets) return fail(VSEL_ERR_INVALID, "NULL logits / targets");
  if (dtype != VSEL_BF16 && dtype != VSEL_F32) return fail(VSEL_ERR_INVALID, "dtype must be bf16 or f32");
  if (rows < 0 || vocab < 1 || row_stride < vocab)
    return fail(VSEL_ERR_INVALID, "bad shape (rows=%lld vocab=%lld row_stride=%lld)", (long long)rows, (long long)vocab, (long long)row_stride);
  if (vocab >= (1ll << 31)) return fail(VSEL_ERR_UNSUPPORTED, "vocab %lld >= 2^31", (long long)vocab);
  if (rows > INT32_MAX) return fail(VSEL_ERR_UNSUPPORTED, "rows %lld > 2^31 - 1", (long long)rows);
  return VSEL_OK;
}

}  // namespace

}  // namespace vsel

using namespace vsel;

extern "C" int vsel_token_logprob_fwd(void* stream, const void* logits, vsel_dtype dtype, int64_t rows, int64_t vocab, int64_t row_stride,
                                      const int64_t* targets, int64_t ignore_index, float* logprob, float* lse, float* sum_out,
                                      int32_t* n_valid_out) {
  if (!logprob || !lse) return fail(VSEL_ERR_INVALID, "NULL logprob / lse");
  if (const int st = check_rows(logits, targets, dtype, rows, vocab, row_stride)) return st;
  hipStream_t st = (hipStream_t)stream;
  if (rows > 0) {
    FwdArgs a{logits, vocab, row_stride, ignore_index, targets, logprob, lse};
    if (dtype == VSEL_BF16) {
      VSEL_LAUNCH(token_logprob_fwd_kernel<bf16_t>, dim3((unsigned)rows), dim3(kThreads), 0, st, a);
    } else {
      VSEL_LAUNCH(token_logprob_fwd_kernel<float>, dim3((unsigned)rows), dim3(kThreads), 0, st, a);
    }
    VSEL_AFTER_LAUNCH(st, "token_logprob_fwd_kernel");
  }
  if (sum_out || n_valid_out) {
    VSEL_LAUNCH(token_logprob_sum_kernel, dim3(1), dim3(kThreads), 0, st, logprob, targets, rows, ignore_index, sum_out, n_valid_out);
    VSEL_AFTER_LAUNCH(st, "token_logprob_sum_kernel");
  }
  return VSEL_OK;
}

extern "C" int vsel_token_logprob_bwd(void* stream, const void* logits, vsel_dtype dtype, int64_t rows, int64_t vocab, int64_t row_stride,
                                      const int64_t* targets, int64_t ignore_index, const float* lse, const float* grad_rows,
                                      const float* grad_scale, void* grad_logits) {
  if (!lse || !grad_logits) return fail(VSEL_ERR_INVALID, "NULL lse / grad_logits");
  if (const int st = check_rows(logits, targets, dtype, rows, vocab, row_stride)) return st;
  if (rows == 0) return VSEL_OK;
  BwdArgs a{logits, vocab, row_stride, ignore_index, targets, lse, grad_rows, grad_scale, grad_logits};
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VSEL_BF16) {
    VSEL_LAUNCH(token_logprob_bwd_kernel<bf16_t>, dim3((unsigned)rows), dim3(kThreads), 0, st, a);
  } else {
    VSEL_LAUNCH(token_logprob_bwd_kernel<float>, dim3((unsigned)rows), dim3(kThreads), 0, st, a);
  }
  VSEL_AFTER_LAUNCH(st, "token_logprob_bwd_kernel");
  return VSEL_OK;
}
