// Temperature / top-k / top-p sampling of one token per row (gfx950): vsel_sample_tokens, HF's warper order (temperature ->
// TopKLogitsWarper -> TopPLogitsWarper -> multinomial).  The exact rules are DESIGN.md §13; in short, per row:
//   pass 1     row max m, the invalid flag (a NaN / +inf, or no finite entry -> token -1) and the finite count;
//   descent    order-preserving unsigned keys of the raw logits (monotone in x / T for T > 0), radix 256 from the top digit
//              (bf16: 2 levels, fp32: 4): top-k by count (tau_k = the k-th largest key), accumulating the fixed-point mass
//              Z = sum_{x >= tau_k} w, w = floor(exp2((x - m) * log2e / T) * 2^40) as uint64; then top-p by mass (tau = the
//              largest key whose mass at or above it reaches ceil(top_p * Z)).  Integer sums: the result does not depend on
//              the order of the additions.  Skipped when both filters are off; top_k == 1 keeps the entries equal to m;
//   last pass  Gumbel-max over the kept set {x finite, key >= tau}: argmax of (x - m) / T - log(-log u), equal scores to the
//              lowest index, u from Philox4x32-10 (key = seed, counter = (i >> 2, row_id, step lo, step hi), word i & 3).
// One workgroup of 1024 threads per row (grid = batch): no workspace, no communication between workgroups.  The row is read
// once per pass (the later passes hit L2 / the Infinity Cache); 16-byte loads on the aligned body of the row, scalar head and
// tail, so odd vocabularies and strided rows (logits[:, -1, :] of [B, S, V]) take the same path.
#include <cmath>

#include "common.h"

namespace vsel {

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr int kBins = 256;

struct SampleArgs {
  const void* logits;
  int64_t vocab, row_stride;
  float c;                     // log2(e) / T   (mass exponent scale)
  float inv_t;                 // 1 / T         (Gumbel score scale)
  float top_p;
  int64_t top_k;
  uint32_t seed_lo, seed_hi, step_lo, step_hi;
  const int64_t* row_ids;
  int64_t* tokens;
  int32_t* kept;
};

// element access: raw bits -> (fp32 value, order-preserving key).  -0 is folded onto +0 so that equal values have equal keys.
template <typename T> struct Bits;
template <> struct Bits<bf16_t> {
  static constexpr int kVec = 8, kLevels = 2;
  static __device__ __forceinline__ float value(uint32_t b) { return __uint_as_float(b << 16); }
  static __device__ __forceinline__ uint32_t key(uint32_t b) {
    b = b == 0x8000u ? 0u : b;
    return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
  }
  static __device__ __forceinline__ uint32_t scalar(const void* p, int64_t i) { return static_cast<const uint16_t*>(p)[i]; }
  static __device__ __forceinline__ void vec(const void* p, int64_t i, uint32_t (&b)[8]) {
    const u32x4 r = *reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(p) + i);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      b[2 * t] = r[t] & 0xffffu;
      b[2 * t + 1] = r[t] >> 16;
    }
  }
};
template <> struct Bits<float> {
  static constexpr int kVec = 4, kLevels = 4;
  static __device__ __forceinline__ float value(uint32_t b) { return __uint_as_float(b); }
  static __device__ __forceinline__ uint32_t key(uint32_t b) {
    b = b == 0x80000000u ? 0u : b;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  }
  static __device__ __forceinline__ uint32_t scalar(const void* p, int64_t i) { return static_cast<const uint32_t*>(p)[i]; }
  static __device__ __forceinline__ void vec(const void* p, int64_t i, uint32_t (&b)[4]) {
    const u32x4 r = *reinterpret_cast<const u32x4*>(static_cast<const uint32_t*>(p) + i);
#pragma unroll
    for (int t = 0; t < 4; ++t) b[t] = r[t];
  }
};

// Visit every element of a row as fn(index, bits).  The call is made by every thread of the block the same number of times
// (`valid` false on the padding lanes of the last sweep), so that fn may use whole-wave operations.  Scalar head up to the first
// 16-byte boundary, 16-byte body, scalar tail.
template <typename T, typename Fn>
__device__ __forceinline__ void for_row(const void* row, int64_t vocab, Fn&& fn) {
  constexpr int V = Bits<T>::kVec;
  constexpr int64_t esz = sizeof(T);
  const int64_t mis = (int64_t)((uintptr_t)row & 15);
  const int64_t head = min(vocab, mis ? (16 - mis) / esz : (int64_t)0);
  const int64_t nvec = (vocab - head) / V;
  const int64_t body_end = head + nvec * V;
  const int tid = threadIdx.x;
  // head (< 8 elements) and tail (< 8 elements) in one sweep
  {
    const int64_t n_tail = vocab - body_end;
    const bool in_head = tid < head, in_tail = tid >= 16 && tid - 16 < n_tail;
    const int64_t i = in_head ? tid : body_end + (tid - 16);
    const bool ok = in_head || in_tail;
    fn(ok ? i : 0, ok ? Bits<T>::scalar(row, i) : 0u, ok);
  }
  for (int64_t v0 = 0; v0 < nvec; v0 += kThreads) {
    const int64_t v = v0 + tid;
    const bool ok = v < nvec;
    uint32_t b[V];
    if (ok) {
      Bits<T>::vec(row, head + v * V, b);
    } else {
#pragma unroll
      for (int t = 0; t < V; ++t) b[t] = 0u;
    }
#pragma unroll
    for (int t = 0; t < V; ++t) fn(head + v * V + t, b[t], ok);
  }
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

__device__ __forceinline__ uint32_t wave_total_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readlane((int)wave_prefix_sum_u32(v), kWave - 1);
}

// histogram add with the lanes of a wave that hit the same bin combined first: logits crowd into a few top-digit bins, and 64
// lanes adding to one LDS word serialise.  Called with the whole wave active.
__device__ __forceinline__ void hist_add(bool act, uint32_t bin, unsigned long long w, bool with_mass, uint32_t* hc,
                                         unsigned long long* hm) {
  const int lane = threadIdx.x & (kWave - 1);
  unsigned long long pend = __ballot(act);
  while (pend) {
    const int leader = __ffsll((long long)pend) - 1;
    const uint32_t lb = __shfl(bin, leader, kWave);
    const bool mine = act && bin == lb;
    const unsigned long long mm = __ballot(mine);
    unsigned long long s = 0;
    if (with_mass) s = __popcll(mm) == 1 ? w : wave_sum_u64(mine ? w : 0ull);
    if (lane == leader) {
      atomicAdd(&hc[lb], (uint32_t)__popcll(mm));
      if (with_mass) atomicAdd(&hm[lb], s);
    }
    pend &= ~mm;
  }
}

// Wave 0: walk the 256 bins from the top, find the bin where the running total (counts, or masses) reaches `target`.
// -> bin, and the count / mass of the bins above it.  Lane l owns bins 255 - 4l .. 252 - 4l.
__device__ __forceinline__ void pick_bin(const uint32_t* hc, const unsigned long long* hm, bool by_mass, unsigned long long target,
                                         int* o_bin, uint32_t* o_cnt_above, unsigned long long* o_mass_above) {
  const int lane = threadIdx.x;
  unsigned long long own = 0, own_m = 0;
  uint32_t own_c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int b = 255 - 4 * lane - j;
    own_c += hc[b];
    own_m += hm[b];
  }
  own = by_mass ? own_m : own_c;
  // inclusive prefix sums over lanes (bins in descending order)
  unsigned long long inc = own, inc_m = own_m;
  uint32_t inc_c = own_c;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const unsigned long long a = __shfl_up(inc, o, kWave), am = __shfl_up(inc_m, o, kWave);
    const uint32_t ac = __shfl_up(inc_c, o, kWave);
    if (lane >= o) { inc += a; inc_m += am; inc_c += ac; }
  }
  const unsigned long long hit = __ballot(inc >= target);
  const int l = hit ? __ffsll((long long)hit) - 1 : kWave - 1;
  if (lane == l) {
    unsigned long long acc = inc - own, acc_m = inc_m - own_m;
    uint32_t acc_c = inc_c - own_c;
    int b = 255 - 4 * l;
    for (int j = 0; j < 4; ++j) {
      b = 255 - 4 * l - j;
      const unsigned long long here = by_mass ? hm[b] : hc[b];
      if (acc + here >= target || j == 3) break;
      acc += here;
      acc_m += hm[b];
      acc_c += hc[b];
    }
    *o_bin = b;
    *o_cnt_above = acc_c;
    *o_mass_above = acc_m;
  }
}

__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
    const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// -log(u), u = ((word >> 8) + 0.5) * 2^-24, without rounding u: below 1/2 u is exact in fp32; above, 1 - u is.
__device__ __forceinline__ float neg_log_u(uint32_t word) {
  const uint32_t k = word >> 8;
  if (k < (1u << 23)) return -__logf(((float)k + 0.5f) * 0x1p-24f);
  return -log1pf(-((float)((1u << 24) - 1u - k) + 0.5f) * 0x1p-24f);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void sample_tokens_kernel(SampleArgs a) {
  using B = Bits<T>;
  constexpr int kLevels = B::kLevels;
  constexpr int kKeyBits = 8 * kLevels;
  const int64_t r = blockIdx.x;
  const void* row = static_cast<const char*>(a.logits) + r * a.row_stride * (int64_t)sizeof(T);
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

  __shared__ uint32_t hc0[kBins], hc1[kBins];
  __shared__ unsigned long long hm0[kBins], hm1[kBins];
  __shared__ float red_f[kWaves];
  __shared__ int red_i[kWaves];
  __shared__ uint32_t red_u[kWaves];
  __shared__ int s_bin;
  __shared__ uint32_t s_cnt_above;
  __shared__ unsigned long long s_mass_above;

  // ---- pass 1: max over the finite entries, invalid flag, finite count --------------------------------------------------------
  float mx = -INFINITY;
  uint32_t nfin = 0;
  bool bad = false;
  for_row<T>(row, a.vocab, [&](int64_t, uint32_t bits, bool ok) {
    const float x = B::value(bits);
    if (ok) {
      bad |= isnan(x) || x == INFINITY;
      if (x != -INFINITY) { mx = fmaxf(mx, x); ++nfin; }
    }
  });
  mx = wave_max(mx);
  nfin = wave_total_u32(nfin);
  const bool wave_bad = __any(bad);
  if (lane == 0) { red_f[wave] = mx; red_u[wave] = nfin; red_i[wave] = wave_bad; }
  __syncthreads();
  mx = -INFINITY; nfin = 0; bad = false;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) { mx = fmaxf(mx, red_f[w]); nfin += red_u[w]; bad |= red_i[w] != 0; }
  if (bad || nfin == 0) {
    if (tid == 0) {
      a.tokens[r] = -1;
      if (a.kept) a.kept[r] = 0;
    }
    return;
  }
  const float m = mx;
  auto mass = [&](float x) -> unsigned long long { return (unsigned long long)(exp2f((x - m) * a.c) * 0x1p40f); };

  // ---- descent: tau as a key; every finite entry with key >= tau is kept -----------------------------------------------------
  const bool topk_on = a.top_k > 0 && a.top_k < (int64_t)nfin;
  const bool topp_on = a.top_p < 1.0f;
  uint32_t tau = 0;
  if (topk_on && a.top_k == 1) {
    tau = B::key(kLevels == 2 ? (__float_as_uint(m) >> 16) : __float_as_uint(m));   // tau_k = m, and tau >= tau_k
  } else if (topk_on || topp_on) {
    // histogram of level `lvl` (into h0 for level 0, h1 deeper) over the finite entries whose key has the higher digits `prefix`
    // and is >= floor_key; masses only when with_mass
    auto level = [&](int lvl, uint32_t prefix, uint32_t floor_key, bool with_mass) {
      uint32_t* hc = lvl ? hc1 : hc0;
      unsigned long long* hm = lvl ? hm1 : hm0;
      for (int i = tid; i < kBins; i += kThreads) { hc[i] = 0; hm[i] = 0; }
      __syncthreads();
      const int shift = kKeyBits - 8 * (lvl + 1);
      for_row<T>(row, a.vocab, [&](int64_t, uint32_t bits, bool ok) {
        const float x = B::value(bits);
        const uint32_t k = B::key(bits);
        const bool act = ok && x != -INFINITY && (lvl == 0 || (k >> (shift + 8)) == prefix) && k >= floor_key;
        hist_add(act, (k >> shift) & 255u, act && with_mass ? mass(x) : 0ull, with_mass, hc, hm);
      });
      __syncthreads();
    };
    // the bin of level `lvl` where the running count / mass from the top reaches `target`; the count and mass above it, and its
    // own mass
    auto pick = [&](int lvl, bool by_mass, unsigned long long target, uint32_t& cnt_above, unsigned long long& mass_above,
                    unsigned long long& mass_bin) {
      const uint32_t* hc = lvl ? hc1 : hc0;
      const unsigned long long* hm = lvl ? hm1 : hm0;
      if (wave == 0) pick_bin(hc, hm, by_mass, target, &s_bin, &s_cnt_above, &s_mass_above);
      __syncthreads();
      const int b = s_bin;
      cnt_above = s_cnt_above;
      mass_above = s_mass_above;
      mass_bin = hm[b];
      __syncthreads();
      return (uint32_t)b;
    };
    uint32_t ca;
    unsigned long long ma, mb, z = 0;
    uint32_t tau_k = 0;
    level(0, 0, 0, topp_on);
    if (topk_on) {
      uint32_t prefix = 0, need = (uint32_t)a.top_k;
      for (int lvl = 0; lvl < kLevels; ++lvl) {
        if (lvl > 0) level(lvl, prefix, 0, topp_on);
        const uint32_t b = pick(lvl, false, need, ca, ma, mb);
        z += ma;
        need -= ca;
        prefix = (prefix << 8) | b;
        if (lvl == kLevels - 1) z += mb;                       // every entry equal to tau_k is kept
      }
      tau_k = prefix;
    } else if (topp_on) {
      pick(0, true, ~0ull, ca, z, mb);                        // no bin reaches the target: z = the whole row's mass
      z += mb;
    }
    tau = tau_k;
    if (topp_on) {
      // level 0 is not restricted to key >= tau_k; the bin where its running mass reaches the target is nevertheless the bin the
      // restricted histogram gives: entries below tau_k only add mass at or below tau_k's own top digit, where the restricted
      // running mass already reaches Z >= target.  The deeper levels are restricted.
      const double t = ceil((double)a.top_p * (double)z);
      unsigned long long need = t >= (double)z ? z : (unsigned long long)t;
      need = need < 1 ? 1 : need;
      uint32_t prefix = 0;
      for (int lvl = 0; lvl < kLevels; ++lvl) {
        if (lvl > 0) level(lvl, prefix, tau_k, true);
        prefix = (prefix << 8) | pick(lvl, true, need, ca, ma, mb);
        need -= ma;
      }
      tau = max(prefix, tau_k);
    }
  }

  // ---- last pass: Gumbel-max over the kept set -------------------------------------------------------------------------------
  const uint32_t rid = a.row_ids ? (uint32_t)a.row_ids[r] : (uint32_t)r;
  float best = -INFINITY;
  int best_i = INT32_MAX;
  uint32_t kept = 0;
  int64_t blk = -1;
  uint32_t words[4] = {0u, 0u, 0u, 0u};
  for_row<T>(row, a.vocab, [&](int64_t i, uint32_t bits, bool ok) {
    const float x = B::value(bits);
    if (ok && x != -INFINITY && B::key(bits) >= tau) {
      ++kept;
      if ((i >> 2) != blk) {
        blk = i >> 2;
        words[0] = (uint32_t)blk; words[1] = rid; words[2] = a.step_lo; words[3] = a.step_hi;
        philox4x32_10(words, a.seed_lo, a.seed_hi);
      }
      const uint32_t wd = words[i & 3];
      const float s = (x - m) * a.inv_t - __logf(neg_log_u(wd));
      if (s > best || (s == best && (int)i < best_i)) { best = s; best_i = (int)i; }
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, kWave);
    const int oi = __shfl_xor(best_i, o, kWave);
    if (ob > best || (ob == best && oi < best_i)) { best = ob; best_i = oi; }
  }
  kept = wave_total_u32(kept);
  __syncthreads();
  if (lane == 0) { red_f[wave] = best; red_i[wave] = best_i; red_u[wave] = kept; }
  __syncthreads();
  if (tid == 0) {
    float bb = red_f[0];
    int bi = red_i[0];
    uint32_t kk = red_u[0];
    for (int w = 1; w < kWaves; ++w) {
      if (red_f[w] > bb || (red_f[w] == bb && red_i[w] < bi)) { bb = red_f[w]; bi = red_i[w]; }
      kk += red_u[w];
    }
    a.tokens[r] = bi;
    if (a.kept) a.kept[r] = (int32_t)kk;
  }
}

// ---- per-row parameters, min-p and the drawn token's log-probability: vsel_sample_tokens_rows ------------------------------------
struct SampleRowsArgs {
  const void* logits;
  int64_t vocab, row_stride;
  const float* temperature;    // DEVICE [batch] each, or NULL: 1, 1, 0, 0
  const float* top_p;
  const int32_t* top_k;
  const float* min_p;
  uint32_t seed_lo, seed_hi, step_lo, step_hi;
  const int64_t* row_ids;
  int64_t* tokens;
  int32_t* kept;
  float* logprob;
};

constexpr double kLog2e = 1.4426950408889634, kLn2 = 0.6931471805599453;

// ln of (d_t, Z): the drawn token's mass exponent d_t = (x_t - m) * c and the integer mass of the set it was drawn from
__device__ __forceinline__ float logprob_of(float d_t, unsigned long long z) {
  return (float)((double)d_t * kLn2 - log((double)z * 0x1p-40));
}

// sample_tokens_kernel with the parameters of row r read from the device (workgroup-uniform: no divergence).  The passes, the
// descent and the Gumbel scores are those of the kernel above, expression for expression, so that a batch of equal parameters with
// min_p 0 gives its tokens and kept counts bit for bit.  Added: T == 0 rows (argmax, tracked in pass 1), the min-p threshold on
// d = (x - m) * c in the last pass, and there the integer mass of the final set for the log-probability.
template <typename T>
__global__ __launch_bounds__(kThreads) void sample_tokens_rows_kernel(SampleRowsArgs a) {
  using B = Bits<T>;
  constexpr int kLevels = B::kLevels;
  constexpr int kKeyBits = 8 * kLevels;
  const int64_t r = blockIdx.x;
  const void* row = static_cast<const char*>(a.logits) + r * a.row_stride * (int64_t)sizeof(T);
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

  __shared__ uint32_t hc0[kBins], hc1[kBins];
  __shared__ unsigned long long hm0[kBins], hm1[kBins];
  __shared__ float red_f[kWaves];
  __shared__ int red_i[kWaves];
  __shared__ uint32_t red_u[kWaves];
  __shared__ unsigned long long red_m[kWaves];
  __shared__ int s_bin;
  __shared__ uint32_t s_cnt_above;
  __shared__ unsigned long long s_mass_above;

  auto reject = [&]() {
    if (tid == 0) {
      a.tokens[r] = -1;
      if (a.kept) a.kept[r] = 0;
      if (a.logprob) a.logprob[r] = __uint_as_float(0x7fc00000u);
    }
  };

  // ---- the row's parameters ---------------------------------------------------------------------------------------------------
  const float temp = a.temperature ? a.temperature[r] : 1.0f;
  const bool greedy = temp == 0.0f;                               // the other parameters of a greedy row are not looked at
  const float top_p = a.top_p && !greedy ? a.top_p[r] : 1.0f;
  const int64_t top_k = a.top_k && !greedy ? (int64_t)a.top_k[r] : 0;
  const float min_p = a.min_p && !greedy ? a.min_p[r] : 0.0f;
  if (!(temp >= 0.0f) || isinf(temp) || !(top_p > 0.0f && top_p <= 1.0f) || top_k < 0 || !(min_p >= 0.0f && min_p <= 1.0f)) {
    reject();
    return;
  }
  const float c = (float)(kLog2e / (double)(greedy ? 1.0f : temp));          // greedy: the model's own softmax for logprob
  const float inv_t = (float)(1.0 / (double)(greedy ? 1.0f : temp));
  const bool minp_on = min_p > 0.0f;
  const float lmin = (float)log2((double)min_p);

  // ---- pass 1: max over the finite entries (and its lowest index), invalid flag, finite count ----------------------------------
  float mx = -INFINITY;
  int mi = INT32_MAX;
  uint32_t nfin = 0;
  bool bad = false;
  for_row<T>(row, a.vocab, [&](int64_t i, uint32_t bits, bool ok) {
    const float x = B::value(bits);
    if (ok) {
      bad |= isnan(x) || x == INFINITY;
      if (x != -INFINITY) {
        if (x > mx || (x == mx && (int)i < mi)) { mx = x; mi = (int)i; }
        ++nfin;
      }
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ox = __shfl_xor(mx, o, kWave);
    const int oi = __shfl_xor(mi, o, kWave);
    if (ox > mx || (ox == mx && oi < mi)) { mx = ox; mi = oi; }
  }
  nfin = wave_total_u32(nfin);
  const bool wave_bad = __any(bad);
  if (lane == 0) { red_f[wave] = mx; red_u[wave] = nfin; red_i[wave] = wave_bad ? -1 : mi; }
  __syncthreads();
  mx = -INFINITY; mi = INT32_MAX; nfin = 0; bad = false;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const float ox = red_f[w];
    const int oi = red_i[w];
    bad |= oi < 0;
    if (ox > mx || (ox == mx && oi < mi)) { mx = ox; mi = oi; }
    nfin += red_u[w];
  }
  if (bad || nfin == 0) {
    reject();
    return;
  }
  const float m = mx;
  auto mass = [&](float x) -> unsigned long long { return (unsigned long long)(exp2f((x - m) * c) * 0x1p40f); };

  // ---- greedy row: the argmax; with logprob one more pass for the mass of all finite entries at T = 1 ---------------------------
  if (greedy) {
    unsigned long long z = 0;
    if (a.logprob) {
      for_row<T>(row, a.vocab, [&](int64_t, uint32_t bits, bool ok) {
        const float x = B::value(bits);
        if (ok && x != -INFINITY) z += mass(x);
      });
      z = wave_sum_u64(z);
      __syncthreads();
      if (lane == 0) red_m[wave] = z;
      __syncthreads();
    }
    if (tid == 0) {
      a.tokens[r] = mi;
      if (a.kept) a.kept[r] = 1;
      if (a.logprob) {
        z = 0;
        for (int w = 0; w < kWaves; ++w) z += red_m[w];
        a.logprob[r] = logprob_of(0.0f, z);
      }
    }
    return;
  }

  // ---- descent: tau as a key; every finite entry with key >= tau is kept (as in sample_tokens_kernel) ---------------------------
  const bool topk_on = top_k > 0 && top_k < (int64_t)nfin;
  const bool topp_on = top_p < 1.0f;
  uint32_t tau = 0;
  if (topk_on && top_k == 1) {
    tau = B::key(kLevels == 2 ? (__float_as_uint(m) >> 16) : __float_as_uint(m));   // tau_k = m, and tau >= tau_k
  } else if (topk_on || topp_on) {
    auto level = [&](int lvl, uint32_t prefix, uint32_t floor_key, bool with_mass) {
      uint32_t* hc = lvl ? hc1 : hc0;
      unsigned long long* hm = lvl ? hm1 : hm0;
      for (int i = tid; i < kBins; i += kThreads) { hc[i] = 0; hm[i] = 0; }
      __syncthreads();
      const int shift = kKeyBits - 8 * (lvl + 1);
      for_row<T>(row, a.vocab, [&](int64_t, uint32_t bits, bool ok) {
        const float x = B::value(bits);
        const uint32_t k = B::key(bits);
        const bool act = ok && x != -INFINITY && (lvl == 0 || (k >> (shift + 8)) == prefix) && k >= floor_key;
        hist_add(act, (k >> shift) & 255u, act && with_mass ? mass(x) : 0ull, with_mass, hc, hm);
      });
      __syncthreads();
    };
    auto pick = [&](int lvl, bool by_mass, unsigned long long target, uint32_t& cnt_above, unsigned long long& mass_above,
                    unsigned long long& mass_bin) {
      const uint32_t* hc = lvl ? hc1 : hc0;
      const unsigned long long* hm = lvl ? hm1 : hm0;
      if (wave == 0) pick_bin(hc, hm, by_mass, target, &s_bin, &s_cnt_above, &s_mass_above);
      __syncthreads();
      const int b = s_bin;
      cnt_above = s_cnt_above;
      mass_above = s_mass_above;
      mass_bin = hm[b];
      __syncthreads();
      return (uint32_t)b;
    };
    uint32_t ca;
    unsigned long long ma, mb, z = 0;
    uint32_t tau_k = 0;
    level(0, 0, 0, topp_on);
    if (topk_on) {
      uint32_t prefix = 0, need = (uint32_t)top_k;
      for (int lvl = 0; lvl < kLevels; ++lvl) {
        if (lvl > 0) level(lvl, prefix, 0, topp_on);
        const uint32_t b = pick(lvl, false, need, ca, ma, mb);
        z += ma;
        need -= ca;
        prefix = (prefix << 8) | b;
        if (lvl == kLevels - 1) z += mb;                       // every entry equal to tau_k is kept
      }
      tau_k = prefix;
    } else if (topp_on) {
      pick(0, true, ~0ull, ca, z, mb);                        // no bin reaches the target: z = the whole row's mass
      z += mb;
    }
    tau = tau_k;
    if (topp_on) {
      const double t = ceil((double)top_p * (double)z);        // Z and the target before min-p: HF's order
      unsigned long long need = t >= (double)z ? z : (unsigned long long)t;
      need = need < 1 ? 1 : need;
      uint32_t prefix = 0;
      for (int lvl = 0; lvl < kLevels; ++lvl) {
        if (lvl > 0) level(lvl, prefix, tau_k, true);
        prefix = (prefix << 8) | pick(lvl, true, need, ca, ma, mb);
        need -= ma;
      }
      tau = max(prefix, tau_k);
    }
  }

  // ---- last pass: Gumbel-max over the final set {key >= tau, d >= lmin}; its integer mass when logprob is wanted ----------------
  const uint32_t rid = a.row_ids ? (uint32_t)a.row_ids[r] : (uint32_t)r;
  const bool with_lp = a.logprob != nullptr;
  float best = -INFINITY;
  int best_i = INT32_MAX;
  uint32_t kept = 0;
  unsigned long long zk = 0;
  int64_t blk = -1;
  uint32_t words[4] = {0u, 0u, 0u, 0u};
  for_row<T>(row, a.vocab, [&](int64_t i, uint32_t bits, bool ok) {
    const float x = B::value(bits);
    if (ok && x != -INFINITY && B::key(bits) >= tau && !(minp_on && (x - m) * c < lmin)) {
      ++kept;
      if (with_lp) zk += mass(x);
      if ((i >> 2) != blk) {
        blk = i >> 2;
        words[0] = (uint32_t)blk; words[1] = rid; words[2] = a.step_lo; words[3] = a.step_hi;
        philox4x32_10(words, a.seed_lo, a.seed_hi);
      }
      const uint32_t wd = words[i & 3];
      const float s = (x - m) * inv_t - __logf(neg_log_u(wd));
      if (s > best || (s == best && (int)i < best_i)) { best = s; best_i = (int)i; }
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, kWave);
    const int oi = __shfl_xor(best_i, o, kWave);
    if (ob > best || (ob == best && oi < best_i)) { best = ob; best_i = oi; }
  }
  kept = wave_total_u32(kept);
  if (with_lp) zk = wave_sum_u64(zk);
  __syncthreads();
  if (lane == 0) { red_f[wave] = best; red_i[wave] = best_i; red_u[wave] = kept; red_m[wave] = zk; }
  __syncthreads();
  if (tid == 0) {
    float bb = red_f[0];
    int bi = red_i[0];
    uint32_t kk = red_u[0];
    unsigned long long zz = red_m[0];
    for (int w = 1; w < kWaves; ++w) {
      if (red_f[w] > bb || (red_f[w] == bb && red_i[w] < bi)) { bb = red_f[w]; bi = red_i[w]; }
      kk += red_u[w];
      zz += red_m[w];
    }
    a.tokens[r] = bi;
    if (a.kept) a.kept[r] = (int32_t)kk;
    // (the row maximum is in every final set, so bi is an index of the row; the bound only keeps the read inside it regardless)
    if (with_lp) a.logprob[r] = bi < a.vocab ? logprob_of((B::value(B::scalar(row, bi)) - m) * c, zz) : __uint_as_float(0x7fc00000u);
  }
}

}  // namespace

}  // namespace vsel

using namespace vsel;

extern "C" int vsel_sample_tokens(void* stream, const void* logits, vsel_dtype dtype, int64_t batch, int64_t vocab, int64_t row_stride,
                                  float temperature, float top_p, int64_t top_k, uint64_t seed, const int64_t* row_ids, uint64_t step,
                                  int64_t* tokens, int32_t* kept) {
  if (!logits || !tokens) return fail(VSEL_ERR_INVALID, "NULL logits / tokens");
  if (dtype != VSEL_BF16 && dtype != VSEL_F32) return fail(VSEL_ERR_INVALID, "dtype must be bf16 or f32");
  if (!(temperature > 0.0f) || !std::isfinite(temperature)) return fail(VSEL_ERR_INVALID, "temperature %g must be finite and > 0", (double)temperature);
  if (!(top_p > 0.0f && top_p <= 1.0f)) return fail(VSEL_ERR_INVALID, "top_p %g outside (0, 1]", (double)top_p);
  if (top_k < 0) return fail(VSEL_ERR_INVALID, "top_k %lld < 0", (long long)top_k);
  if (vocab < 1 || batch < 0 || row_stride < vocab)
    return fail(VSEL_ERR_INVALID, "bad shape (batch=%lld vocab=%lld row_stride=%lld)", (long long)batch, (long long)vocab, (long long)row_stride);
  // uint64 mass sums stay below vocab * 2^40 < 2^64; token indices and Philox counters fit 31 bits
  if (vocab >= (1ll << 24)) return fail(VSEL_ERR_UNSUPPORTED, "vocab %lld >= 2^24", (long long)vocab);
  if (batch > INT32_MAX) return fail(VSEL_ERR_UNSUPPORTED, "batch %lld > 2^31 - 1", (long long)batch);
  if (batch == 0) return VSEL_OK;

  SampleArgs a{};
  a.logits = logits;
  a.vocab = vocab;
  a.row_stride = row_stride;
  a.c = (float)(1.4426950408889634 / (double)temperature);
  a.inv_t = (float)(1.0 / (double)temperature);
  a.top_p = top_p;
  a.top_k = top_k;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
  a.step_lo = (uint32_t)step; a.step_hi = (uint32_t)(step >> 32);
  a.row_ids = row_ids;
  a.tokens = tokens;
  a.kept = kept;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VSEL_BF16) {
    VSEL_LAUNCH(sample_tokens_kernel<bf16_t>, dim3((unsigned)batch), dim3(kThreads), 0, st, a);
  } else {
    VSEL_LAUNCH(sample_tokens_kernel<float>, dim3((unsigned)batch), dim3(kThreads), 0, st, a);
  }
  VSEL_AFTER_LAUNCH(st, "sample_tokens_kernel");
  return VSEL_OK;
}

extern "C" int vsel_sample_tokens_rows(void* stream, const void* logits, vsel_dtype dtype, int64_t batch, int64_t vocab, int64_t row_stride,
                                       const float* temperature, const float* top_p, const int32_t* top_k, const float* min_p,
                                       uint64_t seed, const int64_t* row_ids, uint64_t step, int64_t* tokens, int32_t* kept,
                                       float* logprob) {
  if (!logits || !tokens) return fail(VSEL_ERR_INVALID, "NULL logits / tokens");
  if (dtype != VSEL_BF16 && dtype != VSEL_F32) return fail(VSEL_ERR_INVALID, "dtype must be bf16 or f32");
  if (vocab < 1 || batch < 0 || row_stride < vocab)
    return fail(VSEL_ERR_INVALID, "bad shape (batch=%lld vocab=%lld row_stride=%lld)", (long long)batch, (long long)vocab, (long long)row_stride);
  if (vocab >= (1ll << 24)) return fail(VSEL_ERR_UNSUPPORTED, "vocab %lld >= 2^24", (long long)vocab);
  if (batch > INT32_MAX) return fail(VSEL_ERR_UNSUPPORTED, "batch %lld > 2^31 - 1", (long long)batch);
  if (batch == 0) return VSEL_OK;

  SampleRowsArgs a{};
  a.logits = logits;
  a.vocab = vocab;
  a.row_stride = row_stride;
  a.temperature = temperature;
  a.top_p = top_p;
  a.top_k = top_k;
  a.min_p = min_p;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
  a.step_lo = (uint32_t)step; a.step_hi = (uint32_t)(step >> 32);
  a.row_ids = row_ids;
  a.tokens = tokens;
  a.kept = kept;
  a.logprob = logprob;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VSEL_BF16) {
    VSEL_LAUNCH(sample_tokens_rows_kernel<bf16_t>, dim3((unsigned)batch), dim3(kThreads), 0, st, a);
  } else {
    VSEL_LAUNCH(sample_tokens_rows_kernel<float>, dim3((unsigned)batch), dim3(kThreads), 0, st, a);
  }
  VSEL_AFTER_LAUNCH(st, "sample_tokens_rows_kernel");
  return VSEL_OK;
}
