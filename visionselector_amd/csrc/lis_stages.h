// Host side of the LIS stages for every file that plans, checks or launches them: constants, workspace plan, argument checks, choice
// of form, and the launchers lis.hip exports.  No __global__ here: lis.hip alone compiles lis_kernels.h, lis_small.h, proj_bf16x3.h.
#pragma once
#include "common.h"
#include <algorithm>

namespace vsel {

constexpr int kProjWaves = 4;         // waves per workgroup of the bf16x3 projection GEMMs (independent waves sharing one operand tile through L1)
constexpr int kRowsPerChunk = 128;   // sweep-1 row chunk (batch-invariant summation order)
constexpr int kSliceNT = 256;        // split-K slice of the kbar projection (fixed => batch-invariant)
constexpr int kSliceNN = 128;        // split-K slice of the w projection
constexpr int kSmallMaxSeg = 8;      // small-batch form (lis_small.h): rows of the M dimension a workgroup rebuilds in its prologue
constexpr int kSumMaxSlices = 16;    // split-K summed in LDS (proj_bf16x3.h): waves per workgroup (1024 threads); a projection with more K-slices keeps the slab form

// Cache policy of the three kernels that touch the token tensor: non-temporal once the tensor clearly exceeds the Infinity
// Cache (256 MB) + L2 (32 MB).  Measured crossover between 264 MB (default policy 4 % faster) and 528 MB (nt 12 % faster).
constexpr int64_t kStreamBytes = 384ll << 20;
inline bool stream_policy(int64_t total_rows, int64_t d, size_t elem) { return total_rows * d * (int64_t)elem >= kStreamBytes; }

struct LisPlan {
  int64_t S, maxn, d, hd;
  int row_splits;
  int ks1, kslice1;  // kbar projection  [S, D] x [Hd, D]^T
  int ks2, kslice2;  // w projection     [S, Hd] x [Hd, D]
  int n_cpart;       // blocks of 256 over Hd
  bool mfma_bf16;    // shapes allow the bf16x3 MFMA projections (K % 16 == 0); weights must also be bf16
  size_t off_partial, off_xbar, off_part1, off_kbar, off_c, off_part2, off_w, off_xs, off_ksp, off_cpart, total;
};

inline LisPlan make_plan(int64_t S, int64_t maxn, int64_t d, int64_t hd) {
  LisPlan p{};
  p.S = S; p.maxn = maxn; p.d = d; p.hd = hd;
  // Batch-invariant plan: the summation tree of one segment never depends on how many segments share the call
  // (fixed 128-row chunks in sweep 1, fixed split-K slices in the projections), so batching and the ragged form
  // reproduce a single-image call bit for bit.
  p.row_splits = (int)std::max<int64_t>(1, cdiv(maxn, kRowsPerChunk));
  p.mfma_bf16 = (d % 16 == 0) && (hd % 16 == 0);
  p.kslice1 = (int)std::min<int64_t>(kSliceNT, cdiv(d, 16) * 16);
  p.ks1 = (int)cdiv(d, p.kslice1);
  p.kslice2 = (int)std::min<int64_t>(kSliceNN, cdiv(hd, 16) * 16);
  p.ks2 = (int)cdiv(hd, p.kslice2);
  p.n_cpart = (int)cdiv(hd, 8);
  const int64_t m_pad = 32 * cdiv(S, 32);
  size_t o = 0;
  auto take = [&](size_t nfloat) { size_t r = o; o += align_up(nfloat * sizeof(float), 256); return r; };
  p.off_partial = take((size_t)S * p.row_splits * d);
  p.off_xbar = take((size_t)S * d);
  p.off_part1 = take((size_t)p.ks1 * m_pad * hd);
  p.off_kbar = take((size_t)S * hd);
  p.off_c = take((size_t)S);
  p.off_part2 = take((size_t)p.ks2 * m_pad * d);
  p.off_w = take((size_t)S * d);
  p.off_xs = take(((size_t)3 * m_pad * d + 1) / 2);
  p.off_ksp = take(((size_t)3 * m_pad * hd + 1) / 2);
  p.off_cpart = take((size_t)S * p.n_cpart);
  p.total = o;
  return p;
}

inline int check_scorer(const vsel_scorer* sc, vsel_dtype hdtype) {
  if (!sc || !sc->wq || !sc->bq || !sc->wk || !sc->bk) return fail(VSEL_ERR_INVALID, "scorer parameter pointer is NULL");
  if (sc->d < 8 || sc->hd < 1) return fail(VSEL_ERR_INVALID, "bad scorer dims d=%lld hd=%lld", (long long)sc->d, (long long)sc->hd);
  if (sc->d % 8 != 0) return fail(VSEL_ERR_UNSUPPORTED, "in_features D=%lld must be a multiple of 8 (16-byte rows)", (long long)sc->d);
  if (sc->wdtype != VSEL_BF16 && sc->wdtype != VSEL_F32) return fail(VSEL_ERR_INVALID, "bad weight dtype");
  if (hdtype != VSEL_BF16 && hdtype != VSEL_F32) return fail(VSEL_ERR_INVALID, "bad token dtype");
  return VSEL_OK;
}

// Calls f(T{}) / f(T{}, TW{}) with T the element type of the tokens (hdtype) and TW that of the scorer weights (wdtype): bf16_t or
// float.  The dtypes have passed check_scorer (or the entry's own "bad dtype" check).
template <typename F> inline int with_dtype(vsel_dtype hdtype, F&& f) { return hdtype == VSEL_BF16 ? f(bf16_t{}) : f(float{}); }
template <typename F> inline int with_dtypes(vsel_dtype hdtype, vsel_dtype wdtype, F&& f) {
  return with_dtype(hdtype, [&](auto t) { return wdtype == VSEL_BF16 ? f(t, bf16_t{}) : f(t, float{}); });
}

// Checks every entry with a scorer and a workspace shares: the scorer, then the workspace size (`need` = the entry's plan, made
// once the scorer's dims are known good) and the 16-byte alignment of h, workspace and weights (`also`: one more pointer of the
// entry's that `what` names).
template <typename Need>
inline int check_scorer_workspace(const void* h, vsel_dtype hdtype, const vsel_scorer* sc, const void* ws, size_t ws_bytes,
                                  Need&& need, const char* what = "h / workspace / weights", const void* also = nullptr) {
  int st = check_scorer(sc, hdtype);
  if (st) return st;
  const size_t total = need();
  if (!ws || ws_bytes < total) return fail(VSEL_ERR_WORKSPACE, "workspace %zu B < required %zu B", ws_bytes, total);
  if (((uintptr_t)h | (uintptr_t)ws | (uintptr_t)sc->wq | (uintptr_t)sc->wk | (uintptr_t)also) & 15)
    return fail(VSEL_ERR_INVALID, "%s must be 16-byte aligned", what);
  return VSEL_OK;
}

// sweep 1 as colsum_seg_kernel (the segments' sums, one "chunk") instead of per-chunk partials: when some slab width (512 / 256 /
// 128 bf16 columns) gives knob LIS_SEG_SUMS (segment, slab) pairs = waves (default 896 = 3.5 per CU; 0 = never; measured per call at
// the 7B geometry, chunked vs this: B = 32 231 vs 228 us, 64 446 vs 428, 96 721 vs 685, 128 848-895 vs 826-830; with 672 pairs no
// gain, with one 512-column slab per wave at B = 64 a loss: 483 vs 442), never for the <= 8 segments the small-batch form may take
// (its kernels rebuild x-bar from chunk partials), more than one chunk, and no segment longer than 1.375 x the average: a wave
// streams its (segment, slab) alone, at most twice as fast once the others are done, so the longest segment's waves finish last --
// tools/exp_ragged_lis.py, profiles/r04_ragged_lis.txt, call time chunked vs this form by max / mean: 1.0 +1.5 %, 1.13 +1.8 ... +3.2 %,
// 1.33 +1.2 ... 0 %, 1.5 - 1.7 (N_i ~ U{576..4096}) -4 % (32 prompts), -7 % (64), -10 % (128: sweep 1 446 -> 336 us).  Same sums bit for
// bit either way: batch invariance is untouched.
inline bool seg_sums_form(const LisPlan& p, const vsel_segments* seg) {
  const int mn = knob(VSEL_KNOB_LIS_SEG_SUMS);
  // (pairs counted for the narrowest slab of bf16 tokens, 128 columns, whatever the token type: the projection stage does not know it)
  return mn > 0 && p.S > 8 && p.S * cdiv(p.d, 128) >= mn && p.row_splits > 1 && p.d % 8 == 0 && seg->total_rows * 11 >= (int64_t)p.S * p.maxn * 8;
}

// The bf16x3 projections with their split-K slices summed in LDS (gemm_nt_sum / gemm_nn_sum_bf16x3_kernel: two launches, no slabs)
// instead of slab GEMM + finish kernel twice (four launches): knob LIS_PROJ_SUM 0 never, 1 whenever both projections have at most
// kSumMaxSlices K-slices (one wave per slice in one workgroup), -1 (default) from kProjSumMinSeg segments.  Same bits either way.
// Measured (tools/ab_proj.py, profiles/proj_sum_ab.txt; us of the four / two projection launches, forms alternated, 7B geometry): 8 images
// 34.7 / 30.6 with the step 83-90 / 85, 16 images 37.0 / 41.2, 32 images 38.6 / 41.2 (one m-tile: one workgroup per 32 weight rows leaves
// most CUs idle, the slab form's 14 slices on 14 CUs win), 64 images 43.6 / 35.7 (step 431-448 / 428-429), 128 images 55.1 / 36.9
// (step 855-857 / 812-844), 3B x 512 60.1 / 43.0, LLaVA-OV x 48 (16 slices) 47.4 / 36.7: a gain from two m-tiles on, and 48 segments is
// the smallest count at which one was measured.
constexpr int kProjSumMinSeg = 48;
inline bool proj_sum_form(const LisPlan& p) {
  const int f = knob(VSEL_KNOB_LIS_PROJ_SUM);
  if (f == 0 || p.ks1 > kSumMaxSlices || p.ks2 > kSumMaxSlices || p.d * p.hd >= (1ll << 30)) return false;      // (32-bit weight offsets)
  return f > 0 || (p.S > 8 && p.S >= kProjSumMinSeg);
}

inline bool small_path_ok(const vsel_segments* seg, const vsel_scorer* sc, const LisPlan& p) {
  return seg->n_seg <= kSmallMaxSeg && sc->wdtype == VSEL_BF16 && p.mfma_bf16 && p.kslice1 <= kSliceNT && p.kslice2 <= kSliceNN &&
         sc->d % 8 == 0 && sc->hd % 8 == 0;
}

// What the inference entries pass to lis_scores_stage: the form is used up to knob VSEL_KNOB_LIS_SMALL_PATH segments per call.
// Measured on MI355X (Qwen2.5-VL-7B geometry, us per call, small form vs batched form): 1 image 36.2 vs 51.7, 2 images 43.8 vs
// 55.8, 3 images 52.2 vs 60.8, 4 images 60.4 vs 65.3, 8 images 102.3 vs 86.2 -- the redundant prologues grow with the segment
// count, so the default limit is 4.  VSEL_SMALL_PATH=<n> / the knob set the limit (0 = never; at most kSmallMaxSeg).
static_assert(kSmallMaxSeg == 8, "common.hip clamps VSEL_KNOB_LIS_SMALL_PATH to 8");
inline bool use_small_path(const vsel_segments* seg, const vsel_scorer* sc, const LisPlan& p) {
  return seg->n_seg <= knob(VSEL_KNOB_LIS_SMALL_PATH) && small_path_ok(seg, sc, p);
}

// ---- exported by lis.hip: each launcher sits beside its kernel and works its grid out from (M, N, K, ks = K-slices of kslice) ----
// The scores stage of every LIS entry: column sums unless the caller supplies col_sums, then the small-batch form (lis_small.h) or
// the batched form of projections + score sweep -- the same bits either way.  The caller decides `small`: the inference entries
// pass knob LIS_SMALL_PATH and small_path_ok(), training passes small_path_ok() alone (one segment per call; the knob tunes
// inference batches and never reaches the training block).  hdtype / sc have passed check_scorer.
int lis_scores_stage(hipStream_t st, const void* h, vsel_dtype hdtype, const vsel_segments* seg, const vsel_scorer* sc, char* ws,
                     const LisPlan& p, float* scores, const int64_t* out_map, const float* col_sums, bool small);
int launch_select(hipStream_t st, const float* scores, const vsel_segments* seg, int64_t* idx, float* mask);
// fp32-input MFMA projections (lis_kernels.h); w, bk, bq are of wdtype (bf16 or fp32)
int launch_gemm_nt(hipStream_t st, vsel_dtype wdtype, const float* x, const void* w, int M, int N, int K, int kslice, int ks, float* part);
int launch_kbar_finish(hipStream_t st, vsel_dtype wdtype, const float* part, int ks, int M, int N, const void* bk, const void* bq, float* kbar, float* c);
int launch_gemm_nn(hipStream_t st, vsel_dtype wdtype, const float* x, const void* w, int M, int N, int K, int kslice, int ks, float* part, float* out);  // + slice_sum
// one-wave-per-tile bf16x3 projection of the small-batch form (lis_small.h), alone or two of one shape in one launch
int launch_proj_nt_small(hipStream_t st, const float* partial, const SegView& sv, int S, int row_splits, const uint16_t* w, int N, int K,
                         int kslice, int ks, float* part, int64_t split_stride, int mean);
int launch_proj_nt_small_pair(hipStream_t st, const float* partial0, const float* partial1, const SegView& sv, int S, int row_splits,
                              const uint16_t* w0, const uint16_t* w1, int N, int K, int kslice, int ks, float* part0, float* part1,
                              int64_t split_stride, int mean0, int mean1);
// bf16x3 planes of the column means and the slab form of the NT projection (proj_bf16x3.h); M = segments
int launch_colsum_finish_split(hipStream_t st, const float* partial, const SegView& sv, int d, int row_splits, int M, uint16_t* xs);
int launch_gemm_nt_bf16x3(hipStream_t st, const uint16_t* xs, const uint16_t* w, int M, int N, int K, int kslice, int ks, float* part);

}  // namespace vsel
