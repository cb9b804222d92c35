// C-ABI entry points of the LIS inference path and the one file that compiles its kernels (lis_kernels.h, lis_small.h, proj_bf16x3.h,
// with their launchers); the other files reach those through lis_stages.h.
#define VSEL_LIS_KERNELS_TU
#include "lis_kernels.h"
#include "lis_small.h"

int vsel::check_segments(const vsel_segments* seg, bool need_k) {
  if (!seg) return fail(VSEL_ERR_INVALID, "segments is NULL");
  if (seg->n_seg < 1 || seg->rows_per_seg < 1 || seg->total_rows < 1)
    return fail(VSEL_ERR_INVALID, "empty segments (n_seg=%lld rows_per_seg=%lld total_rows=%lld)", (long long)seg->n_seg, (long long)seg->rows_per_seg,
                (long long)seg->total_rows);
  if (seg->n_seg > 65535) return fail(VSEL_ERR_UNSUPPORTED, "n_seg %lld > 65535", (long long)seg->n_seg);
  if (seg->total_rows >= (1ll << 31)) return fail(VSEL_ERR_UNSUPPORTED, "total_rows must fit int32");
  if (!seg->seg_rows && seg->total_rows != seg->n_seg * seg->rows_per_seg)
    return fail(VSEL_ERR_INVALID, "uniform segments: total_rows != n_seg * rows_per_seg");
  if (need_k) {
    if (seg->k < 1 || seg->k > seg->rows_per_seg)
      return fail(VSEL_ERR_INVALID, "k=%lld must satisfy 1 <= k <= rows_per_seg=%lld", (long long)seg->k, (long long)seg->rows_per_seg);
    if ((seg->seg_rows != nullptr) != (seg->seg_out != nullptr))
      return fail(VSEL_ERR_INVALID, "seg_rows and seg_out must both be given (ragged) or both NULL (uniform)");
    if (!seg->seg_out && seg->total_out != seg->n_seg * seg->k)
      return fail(VSEL_ERR_INVALID, "uniform segments: total_out != n_seg * k");
  }
  return VSEL_OK;
}

using namespace vsel;

#ifdef VSEL_TRACE
// copies the stamps of the last small-batch call: out[kTraceKernels][kTraceBlocks][kTraceSlots] (tools/trace_small.py)
extern "C" int vsel_debug_read_trace(unsigned long long* out, int clear) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trace), sizeof(g_trace)) != hipSuccess) return VSEL_ERR_HIP;
  if (clear) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_trace)) != hipSuccess || hipMemset(p, 0, sizeof(g_trace)) != hipSuccess)
      return VSEL_ERR_HIP;
  }
  return VSEL_OK;
}
#endif

// select fused into the gather (select_gather_small_kernel) for mid-size batches of the nine-launch form.  Measured (7B geometry,
// us per call, fused vs two launches): 8 images 82.0 vs 83.3, 16 135.3 vs 137.0, 32 233.4 vs 238.8, 48 350.9 vs 347.1, 128 900.8 vs
// 877.0 -> up to 32 segments; re-measured at the end of round 3: 16 136.9 vs 138.5, 32 227.7 vs 232.9, 48 347.4 vs 353.7, 64 428.4 vs
// 428.7 -> up to 48.  VSEL_FUSED_SELECT=<n> / knob VSEL_KNOB_LIS_FUSED_SELECT.
static inline int fused_select_max_seg() { return knob(VSEL_KNOB_LIS_FUSED_SELECT); }

// (here, not in lis_small.h beside its kernel: only the training backward calls it, and bench.py prices every launch those files name)
int vsel::launch_proj_nt_small_pair(hipStream_t st, const float* partial0, const float* partial1, const SegView& sv, int S, int row_splits,
                              const uint16_t* w0, const uint16_t* w1, int N, int K, int kslice, int ks, float* part0, float* part1,
                              int64_t split_stride, int mean0, int mean1) {
  VSEL_LAUNCH(proj_nt_small_pair_kernel, dim3((unsigned)cdiv(N, 32), ks, 2), dim3(64), 0, st, partial0, partial1, sv, S, row_splits, w0, w1, N,
              K, kslice, part0, part1, split_stride, mean0, mean1);
  VSEL_AFTER_LAUNCH(st, "proj_nt_small_pair_kernel");
  return VSEL_OK;
}

int vsel::lis_scores_stage(hipStream_t st, const void* h, vsel_dtype hdtype, const vsel_segments* seg, const vsel_scorer* sc, char* ws,
                           const LisPlan& p, float* scores, const int64_t* out_map, const float* col_sums, bool small) {
  return with_dtype(hdtype, [&](auto t) {
    using T = decltype(t);
    const T* hp = (const T*)h;
    int rc;
    if (!col_sums && (rc = run_colsum<T>(st, hp, seg, (int)sc->d, ws, p))) return rc;
    if (small) {
      // a handful of segments (lis_small.h): two projection launches instead of up to five, bit-identical results
      if ((rc = run_proj_small(st, seg, sc, ws, p, col_sums))) return rc;
      return run_score_small<T>(st, hp, seg, sc, ws, p, scores, out_map);
    }
    if ((rc = run_proj(st, seg, sc, ws, p, col_sums))) return rc;
    return run_score<T>(st, hp, seg, sc, ws, p, scores, out_map);
  });
}

// scores -> hard top-k -> kept rows; l2p / p2l (both or neither) and col_sums are optional
static int lis_select_impl(void* stream, const void* h, vsel_dtype hdtype, const vsel_segments* seg, const vsel_scorer* sc, void* ws,
                           const LisPlan& p, void* out, int64_t* idx, float* scores, const int64_t* l2p = nullptr,
                           const int64_t* p2l = nullptr, const float* col_sums = nullptr) {
  hipStream_t st = (hipStream_t)stream;
  VSEL_PROF_BEGIN(st);
  const bool small = use_small_path(seg, sc, p);
  int rc = lis_scores_stage(st, h, hdtype, seg, sc, (char*)ws, p, scores, p2l, col_sums, small);
  if (rc) return rc;
  return with_dtype(hdtype, [&](auto t) {
    using T = decltype(t);
    // up to fused_select_max_seg() segments: the radix select runs inside every gather workgroup (one launch less; same indices)
    // (every gather workgroup repeats its segment's select: not when there are thousands of them -- 32 images at 50 % retain:
    // 308.0 vs 305.7 us); the small-batch form always selects there
    if (small || (seg->n_seg <= fused_select_max_seg() && seg->n_seg * cdiv(seg->k, 16) <= 1536))
      return launch_select_gather_small<T>(st, (const T*)h, (int)sc->d, seg, scores, idx, (T*)out, l2p);
    int rc2 = launch_select(st, scores, seg, idx, nullptr);
    if (rc2) return rc2;
    return launch_gather<T>(st, (const T*)h, (int)sc->d, seg, idx, (T*)out, l2p);
  });
}

extern "C" size_t vsel_lis_workspace_bytes(const vsel_segments* seg, int64_t d, int64_t hd) {
  if (!seg || seg->n_seg < 1 || d < 1 || hd < 1) return 0;
  return make_plan(seg->n_seg, seg->rows_per_seg, d, hd).total;
}

static int lis_common_checks(const void* h, const vsel_segments* seg, const vsel_scorer* sc, vsel_dtype hdtype,
                             void* ws, size_t ws_bytes, bool need_k, LisPlan* plan) {
  if (!h) return fail(VSEL_ERR_INVALID, "h is NULL");
  int st = check_segments(seg, need_k);
  if (st) return st;
  return check_scorer_workspace(h, hdtype, sc, ws, ws_bytes, [&] {
    *plan = make_plan(seg->n_seg, seg->rows_per_seg, sc->d, sc->hd);
    return plan->total;
  });
}

extern "C" int vsel_lis_scores(void* stream, const void* h, vsel_dtype hdtype, const vsel_segments* seg,
                               const vsel_scorer* sc, void* ws, size_t ws_bytes, float* scores) {
  LisPlan p;
  int st = lis_common_checks(h, seg, sc, hdtype, ws, ws_bytes, false, &p);
  if (st) return st;
  if (!scores) return fail(VSEL_ERR_INVALID, "scores is NULL");
  hipStream_t s = (hipStream_t)stream;
  VSEL_PROF_BEGIN(s);
  return lis_scores_stage(s, h, hdtype, seg, sc, (char*)ws, p, scores, nullptr, nullptr, use_small_path(seg, sc, p));
}

extern "C" int vsel_topk_select(void* stream, const float* scores, const vsel_segments* seg, int64_t* idx, float* mask) {
  int st = check_segments(seg, true);
  if (st) return st;
  if (!scores || (!idx && !mask)) return fail(VSEL_ERR_INVALID, "scores / outputs NULL");
  VSEL_PROF_BEGIN(stream);
  return launch_select((hipStream_t)stream, scores, seg, idx, mask);
}

extern "C" int vsel_gather_rows(void* stream, const void* h, vsel_dtype hdtype, int64_t d, const vsel_segments* seg,
                                const int64_t* idx, void* out) {
  int st = check_segments(seg, true);
  if (st) return st;
  if (!h || !idx || !out) return fail(VSEL_ERR_INVALID, "NULL pointer");
  if (((uintptr_t)h | (uintptr_t)out) & 15) return fail(VSEL_ERR_INVALID, "h / out must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  VSEL_PROF_BEGIN(s);
  if (hdtype != VSEL_BF16 && hdtype != VSEL_F32) return fail(VSEL_ERR_INVALID, "bad dtype");
  return with_dtype(hdtype, [&](auto t) {
    using T = decltype(t);
    if (d % Elem<T>::kVec) return fail(VSEL_ERR_UNSUPPORTED, "D must be a multiple of %d", Elem<T>::kVec);
    return launch_gather<T>(s, (const T*)h, (int)d, seg, idx, (T*)out);
  });
}

extern "C" int vsel_lis_select(void* stream, const void* h, vsel_dtype hdtype, const vsel_segments* seg,
                               const vsel_scorer* sc, void* ws, size_t ws_bytes, void* out, int64_t* idx,
                               float* scores) {
  LisPlan p;
  int st = lis_common_checks(h, seg, sc, hdtype, ws, ws_bytes, true, &p);
  if (st) return st;
  if (!out || !idx || !scores) return fail(VSEL_ERR_INVALID, "out / idx / scores is NULL");
  if ((uintptr_t)out & 15) return fail(VSEL_ERR_INVALID, "out must be 16-byte aligned");
  return lis_select_impl(stream, h, hdtype, seg, sc, ws, p, out, idx, scores);
}

// Permuted form: the token rows are stored in a PHYSICAL order (Qwen2.5-VL's window order straight out of the merger) and
// the reference semantics are defined on the LOGICAL order it creates with `hidden_states[reverse_indices, :]`
// (EV/token_compression/selector_model.py:179-181).  Scores and indices are produced in logical order, kept rows are
// gathered straight from the physical tensor, so that un-reorder pass (read + write of N x D) is never materialised.
extern "C" int vsel_lis_select_permuted(void* stream, const void* h_physical, vsel_dtype hdtype, const vsel_segments* seg,
                                        const vsel_scorer* sc, void* ws, size_t ws_bytes, const int64_t* logical_to_physical,
                                        const int64_t* physical_to_logical, void* out, int64_t* idx, float* scores) {
  LisPlan p;
  int st = lis_common_checks(h_physical, seg, sc, hdtype, ws, ws_bytes, true, &p);
  if (st) return st;
  if (!out || !idx || !scores || !logical_to_physical || !physical_to_logical) return fail(VSEL_ERR_INVALID, "NULL pointer");
  if ((uintptr_t)out & 15) return fail(VSEL_ERR_INVALID, "out must be 16-byte aligned");
  return lis_select_impl(stream, h_physical, hdtype, seg, sc, ws, p, out, idx, scores, logical_to_physical, physical_to_logical);
}

// Single-sweep form: the producer of the tokens already knows their column sums
// (vsel_gelu_colsum inside the merger + linearity of the merger's last Linear), so sweep 1 is skipped.
extern "C" int vsel_lis_select_presummed(void* stream, const void* h, vsel_dtype hdtype, const vsel_segments* seg,
                                         const vsel_scorer* sc, const float* col_sums, void* ws, size_t ws_bytes,
                                         const int64_t* logical_to_physical, const int64_t* physical_to_logical, void* out,
                                         int64_t* idx, float* scores) {
  LisPlan p;
  int st = lis_common_checks(h, seg, sc, hdtype, ws, ws_bytes, true, &p);
  if (st) return st;
  if (!out || !idx || !scores || !col_sums) return fail(VSEL_ERR_INVALID, "NULL pointer");
  if ((logical_to_physical == nullptr) != (physical_to_logical == nullptr))
    return fail(VSEL_ERR_INVALID, "give both row maps or neither");
  if (((uintptr_t)out | (uintptr_t)col_sums) & 15) return fail(VSEL_ERR_INVALID, "out / col_sums must be 16-byte aligned");
  return lis_select_impl(stream, h, hdtype, seg, sc, ws, p, out, idx, scores, logical_to_physical, physical_to_logical, col_sums);
}
