// Device side of the sequence splice (see splice.hip for the reference lines it replaces): the ordered scan that turns
// (input_ids, kept visual ranks) into the index arrays of the compressed sequence and a per-row source descriptor; the
// row copy that materialises inputs_embeds' is splice.hip's (launch_splice_embed).  Shared by splice.hip (vsel_splice,
// vsel_splice_batched) and select_splice.hip (vsel_lis_select_splice: kept rows are read straight from the token tensor H,
// never staged in a [k, D] tensor).
#pragma once
#include "common.h"

#include <algorithm>
#include <limits.h>

namespace vsel {

constexpr int kSpliceThreads = 1024;
constexpr int kMaxVisualBits = 1 << 18;   // 262 144 visual tokens -> 32 KiB bitmap

// One sequence's slice of the packed arrays: positions [p0, p0+L), its visual tokens hold local ranks [0, nvis), its kept
// visual rows are all_indices[j0 .. j0+k) (local ranks, ascending) and its output rows start at q0.
struct SpliceSeq {
  int p0, L, nvis, j0, k, q0;
};

// Ordered scan of one sequence by one 1024-thread workgroup.  Returns (visual found, rows kept, visual kept) to thread 0.
__device__ __forceinline__ void splice_index_body(
    const SpliceSeq sq, uint32_t* bitmap, const int64_t* __restrict__ ids, int64_t visual_id,
    const int64_t* __restrict__ all_indices, const int64_t* __restrict__ pos, int pos_rows, int64_t pos_stride,
    const int64_t* __restrict__ mask, int64_t* __restrict__ sel, int64_t* __restrict__ new_ids,
    int64_t* __restrict__ new_pos, int64_t* __restrict__ new_mask, int32_t* __restrict__ src, int l_out, int q_end,
    uint32_t& out_vis, uint32_t& out_keep, uint32_t& out_kv, int64_t vis_row_base = -1,
    const int64_t* __restrict__ src_map = nullptr) {
  // vis_row_base >= 0: the kept visual rows are read from the token tensor H itself -- the descriptor of a kept visual token of
  // local rank r is -(physical row of H) - 1 with physical row = src_map ? src_map[vis_row_base + r] : vis_row_base + r
  // (vsel_lis_select_splice); otherwise -(j0 + j) - 1 = its row in the staged [k, D] tensor (vsel_splice).
  __shared__ uint32_t wv[16], wk[16], wj[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int words = (sq.nvis + 31) >> 5;
  for (int i = tid; i < words; i += kSpliceThreads) bitmap[i] = 0u;
  __syncthreads();
  for (int j = tid; j < sq.k; j += kSpliceThreads) {
    const int64_t r = all_indices[sq.j0 + j];
    if (r >= 0 && r < sq.nvis) atomicOr(&bitmap[r >> 5], 1u << (r & 31));
  }
  __syncthreads();
  uint32_t run_vis = 0, run_keep = 0, run_kv = 0;   // running counts: visual tokens, kept positions, kept visual tokens
  for (int c0 = 0; c0 < sq.L; c0 += kSpliceThreads) {
    const int p = c0 + tid;
    const bool valid = p < sq.L;
    const int64_t id = valid ? ids[sq.p0 + p] : 0;
    const bool is_vis = valid && id == visual_id;
    const unsigned long long bvis = __ballot(is_vis);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (lane == 0) wv[wave] = __popcll(bvis);
    __syncthreads();
    uint32_t vis_rank = run_vis + __popcll(bvis & below), tot_vis = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) { if (w < wave) vis_rank += wv[w]; tot_vis += wv[w]; }
    const bool kept_vis = is_vis && vis_rank < (uint32_t)sq.nvis && ((bitmap[vis_rank >> 5] >> (vis_rank & 31)) & 1u);
    const bool keep = valid && (!is_vis || kept_vis);
    const unsigned long long bkeep = __ballot(keep), bkv = __ballot(kept_vis);
    if (lane == 0) { wk[wave] = __popcll(bkeep); wj[wave] = __popcll(bkv); }
    __syncthreads();
    uint32_t q = run_keep + __popcll(bkeep & below), j = run_kv + __popcll(bkv & below), tot_keep = 0, tot_kv = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      if (w < wave) { q += wk[w]; j += wj[w]; }
      tot_keep += wk[w];
      tot_kv += wj[w];
    }
    const int qo = sq.q0 + (int)q;
    if (keep && qo < q_end) {
      sel[qo] = sq.p0 + p;
      new_ids[qo] = id;
      if (mask) new_mask[qo] = mask[sq.p0 + p];
      for (int r = 0; r < pos_rows; ++r) new_pos[(int64_t)r * l_out + qo] = pos[(int64_t)r * pos_stride + sq.p0 + p];
      if (kept_vis && vis_row_base >= 0) {
        const int64_t lrow = vis_row_base + vis_rank;
        src[qo] = -(int32_t)(src_map ? src_map[lrow] : lrow) - 1;
      } else {
        src[qo] = kept_vis ? -(int32_t)(sq.j0 + j + 1) : sq.p0 + p;
      }
    }
    run_vis += tot_vis;
    run_keep += tot_keep;
    run_kv += tot_kv;
    __syncthreads();
  }
  // rows the scan did not produce (input_ids holds fewer kept positions than the descriptors promise: the reference raises
  // ValueError, FT/compression_method/selector_model.py:210-213; here stats report it): mark them so that the embedding
  // copy never dereferences an uninitialised source row
  for (int q = sq.q0 + (int)run_keep + tid; q < q_end; q += kSpliceThreads) {
    src[q] = INT32_MAX;
    sel[q] = -1;
    new_ids[q] = -1;
  }
  out_vis = run_vis;
  out_keep = run_keep;
  out_kv = run_kv;
}

// The row copy after every index scan (splice.hip): out[q] = embeds[src[q]] or vis[-src[q] - 1], rows of `dtype`; none for l_out <= 0
int launch_splice_embed(hipStream_t st, vsel_dtype dtype, const void* embeds, const void* vis, const int32_t* src, int l_out, int d,
                        int n_rows, int n_vis, void* out);

}  // namespace vsel
