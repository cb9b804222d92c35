// KV-cache append + decode attention (gfx950, bf16): the two launches behind vsel_kvcache_attn_fwd, flash-attn's
// flash_attn_with_kvcache (flash-attn 2.7.4 Python API; its docstring is the specification, restated in include/vsel.h).
//
//   1. kvcache_append_kernel: the s_new new key / value rows of every batch row go into the cache at positions
//      cache_seqlens[b] + j (rotary applied to the keys first when tables are given); q is copied -- rotated, when tables are
//      given -- into a packed workspace when the attention cannot read it as it is; and the per-row metadata the attention
//      launch reads is written into the workspace: cu_q, the visible key count, the first visible key row.  No host
//      synchronisation: everything that depends on device values (lengths, page tables, batch indices) is decided here.
//   2. varlen_attn_fwd_kernel (attn.hip) over those keys: a PAGED cache through its page-table address path, a CONTIGUOUS cache
//      [B_cache, L_cache, Hkv, d] through its contiguous-keys path with key row offset cu_k[b] = cache_batch_idx[b] * L_cache +
//      cache_leftpad[b] -- the left padding and the batch index are a start row of the keys, so the attention kernel is used as
//      it is (no new field, every existing instantiation keeps its code).
//
// Safety: a write lands only at a cache position inside the row's capacity (L_cache; for a paged cache the leading run of valid
// block-table entries -- entries in [0, n_blocks) -- times page_size), and the visible key count handed to the attention is
// clamped to the same capacity, so an overflowing row (cache_seqlens[b] + s_new past its capacity: a caller error, its result is
// unspecified) never reads or writes outside the cache.  Rotary table rows are clamped to [0, seqlen_ro).
#include "attn_common.h"

namespace vsel {

struct KvAppendArgs {
  const uint16_t* q;                  // [B, s_q, Hq, d] with the strides below
  int64_t q_bs, q_rs, q_hs;
  uint16_t* q_out;                    // packed [B * s_q, Hq, d] copy of q (rotated when tables are given), or NULL
  const uint16_t* k;                  // new rows [B, s_new, Hkv, d] (strided), or NULL when s_new == 0
  const uint16_t* v;
  int64_t k_bs, k_rs, k_hs, v_bs, v_rs, v_hs;
  uint16_t* k_cache;                  // contiguous [B_cache, L_cache, Hkv, d] or paged [n_blocks, page_size, Hkv, d]
  uint16_t* v_cache;
  int64_t cache_rows;                 // B_cache, or n_blocks
  int64_t cache_len;                  // L_cache, or page_size
  const int32_t* block_table;         // [B, max_pages] (paged), or NULL
  int64_t max_pages;
  const int32_t* cache_seqlens;       // [B], or NULL: seqlen_scalar for every row
  int seqlen_scalar;
  const int32_t* batch_idx;           // [B] cache row of batch row b (contiguous cache), or NULL: b
  const int32_t* leftpad;             // [B] first visible cache position (contiguous cache), or NULL: 0
  const void* rot_cos;                // [seqlen_ro, rotary_dim / 2] fp32 or bf16, or NULL
  const void* rot_sin;
  int rot_f32, seqlen_ro, rotary_dim, rot_interleaved;
  int batch, s_q, s_new, hq, hkv, d, causal;
  int32_t* cu_q;                      // workspace: [B + 1] query offsets b * s_q
  int32_t* seqlens_k;                 // workspace: [B] visible keys
  int32_t* cu_k;                      // workspace: [B] first visible key row (contiguous cache)
};

__device__ __forceinline__ float rot_tab(const void* t, int f32, int64_t i) {
  return f32 ? static_cast<const float*>(t)[i] : bf16_to_f32(static_cast<const uint16_t*>(t)[i]);
}

// One row of H heads x d features from `src` (row base, head stride hs) to `dst` (packed [H, d]), rotated at table row `pos` when
// tables are given.  16-byte vectors; a vector that holds rotary features computes them element by element in fp32 (the partner
// feature of a GPT-NeoX pair sits rotary_dim / 2 away, usually in another vector) and rounds once to bf16.
__device__ __forceinline__ void copy_row(const KvAppendArgs& a, const uint16_t* __restrict__ src, int64_t hs, uint16_t* __restrict__ dst,
                                         int heads, int64_t pos, bool rotate) {
  const int vecs = a.d / 8;
  const int half = a.rotary_dim / 2;
  const int64_t tab = min(max(pos, (int64_t)0), (int64_t)a.seqlen_ro - 1) * half;
  for (int i = threadIdx.x; i < heads * vecs; i += blockDim.x) {
    const int h = i / vecs, e0 = (i % vecs) * 8;
    const uint16_t* s = src + h * hs;
    u32x4 w = *reinterpret_cast<const u32x4*>(s + e0);
    if (rotate && e0 < a.rotary_dim) {
      uint16_t r[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int e = e0 + t;
        const uint32_t bits = (w[t >> 1] >> (16 * (t & 1))) & 0xffffu;
        if (e >= a.rotary_dim) { r[t] = (uint16_t)bits; continue; }
        const bool first = a.rot_interleaved ? (e & 1) == 0 : e < half;
        const int m = a.rot_interleaved ? e >> 1 : (first ? e : e - half);
        const int partner = a.rot_interleaved ? (e ^ 1) : (first ? e + half : e - half);
        const float x = bf16_to_f32(bits), xp = bf16_to_f32(s[partner]);
        const float c = rot_tab(a.rot_cos, a.rot_f32, tab + m), sn = rot_tab(a.rot_sin, a.rot_f32, tab + m);
        // (x1, x2) -> (x1 cos - x2 sin, x1 sin + x2 cos)
        const float y = first ? x * c - xp * sn : xp * sn + x * c;
        r[t] = (uint16_t)f32_to_bf16_bits(y);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) w[t] = (uint32_t)r[2 * t] | ((uint32_t)r[2 * t + 1] << 16);
    }
    *reinterpret_cast<u32x4*>(dst + (int64_t)h * a.d + e0) = w;
  }
}

// grid (B, max(s_new, s_q)), 256 threads: block (b, r) writes new row r of batch row b (r < s_new) and, when a q copy is wanted,
// query row r (r < s_q); block (b, 0) also writes b's metadata
__global__ __launch_bounds__(256) void kvcache_append_kernel(KvAppendArgs a) {
  const int b = blockIdx.x, r = blockIdx.y;
  const int end = a.cache_seqlens ? a.cache_seqlens[b] : a.seqlen_scalar;
  // capacity of the row in cache positions, and the cache row (contiguous) it lives in
  __shared__ int s_alloc;
  int64_t cap, crow = 0;
  if (a.block_table) {
    // allocated pages = the leading run of valid entries (transformers pads block tables with -1)
    const int32_t* bt = a.block_table + (int64_t)b * a.max_pages;
    if (threadIdx.x == 0) s_alloc = (int)a.max_pages;
    __syncthreads();
    for (int64_t p = threadIdx.x; p < a.max_pages; p += blockDim.x)
      if (bt[p] < 0 || bt[p] >= a.cache_rows) atomicMin(&s_alloc, (int)p);
    __syncthreads();
    cap = (int64_t)s_alloc * a.cache_len;
  } else {
    crow = a.batch_idx ? a.batch_idx[b] : b;
    cap = (crow >= 0 && crow < a.cache_rows) ? a.cache_len : 0;
  }
  if (r == 0 && threadIdx.x == 0) {
    const int64_t hi = min(max((int64_t)end + a.s_new, (int64_t)0), cap);
    const int64_t lo = a.leftpad ? min(max((int64_t)a.leftpad[b], (int64_t)0), hi) : 0;
    a.seqlens_k[b] = (int32_t)(hi - lo);
    if (!a.block_table) a.cu_k[b] = (int32_t)(cap > 0 ? crow * a.cache_len + lo : 0);
    a.cu_q[b] = b * a.s_q;
    if (b == a.batch - 1) a.cu_q[a.batch] = a.batch * a.s_q;
  }
  const bool rotate = a.rot_cos != nullptr;
  if (r < a.s_new) {
    const int64_t p = (int64_t)end + r;
    if (p >= 0 && p < cap) {
      int64_t row;                                         // cache row (in [*, Hkv, d] units) of position p
      if (a.block_table) {
        const int64_t pg = p / a.cache_len;
        row = (int64_t)a.block_table[(int64_t)b * a.max_pages + pg] * a.cache_len + (p - pg * a.cache_len);
      } else {
        row = crow * a.cache_len + p;
      }
      const int64_t dst = row * a.hkv * a.d;
      copy_row(a, a.k + b * a.k_bs + r * a.k_rs, a.k_hs, a.k_cache + dst, a.hkv, p, rotate);
      copy_row(a, a.v + b * a.v_bs + r * a.v_rs, a.v_hs, a.v_cache + dst, a.hkv, 0, false);
    }
  }
  if (a.q_out && r < a.s_q) {
    // query i is rotated at cache_seqlens + i under the causal mask, at cache_seqlens otherwise (flash-attn)
    copy_row(a, a.q + b * a.q_bs + r * a.q_rs, a.q_hs, a.q_out + ((int64_t)b * a.s_q + r) * a.hq * a.d, a.hq,
             (int64_t)end + (a.causal ? r : 0), rotate);
  }
}

// workspace: metadata ints, then the packed q copy
static size_t kv_meta_bytes(int64_t batch) { return align_up((size_t)(3 * batch + 1) * sizeof(int32_t), 256); }

}  // namespace vsel

using namespace vsel;

extern "C" size_t vsel_kvcache_attn_workspace_bytes(int64_t batch, int64_t seqlen_q, int64_t hq, int64_t d) {
  if (batch < 1 || seqlen_q < 1 || hq < 1 || d < 1) return 0;
  return kv_meta_bytes(batch) + align_up((size_t)(batch * seqlen_q * hq * d) * sizeof(uint16_t), 256);
}

extern "C" int vsel_kvcache_attn_fwd(void* stream, const void* q, int64_t q_batch_stride, int64_t q_row_stride, int64_t q_head_stride,
                                     void* k_cache, void* v_cache, int64_t cache_rows, int64_t cache_len, const int32_t* block_table,
                                     int64_t max_pages, const void* k, const void* v, int64_t seqlen_new, int64_t k_batch_stride,
                                     int64_t k_row_stride, int64_t k_head_stride, int64_t v_batch_stride, int64_t v_row_stride,
                                     int64_t v_head_stride, const int32_t* cache_seqlens, int64_t cache_seqlen, const int32_t* cache_batch_idx,
                                     const int32_t* cache_leftpad, const void* rotary_cos, const void* rotary_sin, vsel_dtype rotary_dtype,
                                     int64_t seqlen_ro, int64_t rotary_dim, int rotary_interleaved, int64_t batch, int64_t seqlen_q,
                                     int64_t hq, int64_t hkv, int64_t d, float scale, int causal, void* out, float* lse, void* workspace,
                                     size_t workspace_bytes) {
  if (!k_cache || !v_cache || !workspace || (out && !q)) return fail(VSEL_ERR_INVALID, "NULL pointer");
  if (d != 128 && d != 80 && d != 64) return fail(VSEL_ERR_UNSUPPORTED, "head_dim %lld not in {64, 80, 128}", (long long)d);
  if (batch < 1 || batch > (1 << 24) || seqlen_q < 1 || seqlen_q > 65535 || seqlen_new < 0 || seqlen_new > 65535 || hq < 1 ||
      hkv < 1 || hq % hkv != 0 || hq > 65535)
    return fail(VSEL_ERR_INVALID, "bad shape (batch=%lld seqlen_q=%lld seqlen_new=%lld hq=%lld hkv=%lld)", (long long)batch,
                (long long)seqlen_q, (long long)seqlen_new, (long long)hq, (long long)hkv);
  if (batch * seqlen_q >= (1ll << 31)) return fail(VSEL_ERR_UNSUPPORTED, "more than 2^31 - 1 query rows");
  if (seqlen_new > 0 && (!k || !v)) return fail(VSEL_ERR_INVALID, "seqlen_new > 0 needs k and v");
  if (cache_rows < 1 || cache_len < 1) return fail(VSEL_ERR_INVALID, "empty cache");
  if (int rc = attn::check_softmax_scale(scale)) return rc;
  if (block_table) {
    if (cache_batch_idx || cache_leftpad) return fail(VSEL_ERR_UNSUPPORTED, "a paged cache takes neither cache_batch_idx nor cache_leftpad");
    if (max_pages < 1 || max_pages > (1 << 24) || cache_len > (1 << 20)) return fail(VSEL_ERR_INVALID, "bad page geometry");
    if (cache_rows * cache_len >= (1ll << 31)) return fail(VSEL_ERR_UNSUPPORTED, "more than 2^31 - 1 cache positions");
  } else if (cache_rows * cache_len >= (1ll << 31)) {
    return fail(VSEL_ERR_UNSUPPORTED, "more than 2^31 - 1 cache positions");
  }
  if (!cache_seqlens && (cache_seqlen < INT32_MIN || cache_seqlen > INT32_MAX)) return fail(VSEL_ERR_INVALID, "cache_seqlen out of range");
  if ((rotary_cos == nullptr) != (rotary_sin == nullptr)) return fail(VSEL_ERR_INVALID, "give rotary_cos and rotary_sin together");
  if (rotary_cos && (rotary_dim < 2 || rotary_dim % 2 || rotary_dim > d || seqlen_ro < 1 || seqlen_ro > INT32_MAX ||
                     (rotary_dtype != VSEL_BF16 && rotary_dtype != VSEL_F32)))
    return fail(VSEL_ERR_INVALID, "bad rotary tables (rotary_dim=%lld seqlen_ro=%lld)", (long long)rotary_dim, (long long)seqlen_ro);
  // 16-byte rows: every stride a multiple of 8 elements, every base 16-byte aligned
  if ((q_batch_stride | q_row_stride | q_head_stride | k_batch_stride | k_row_stride | k_head_stride | v_batch_stride | v_row_stride |
       v_head_stride) % 8 ||
      ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)out) & 15)
    return fail(VSEL_ERR_INVALID, "q / k / v strides must be multiples of 8 elements and every tensor 16-byte aligned");
  const size_t need = vsel_kvcache_attn_workspace_bytes(batch, seqlen_q, hq, d);
  if (workspace_bytes < need) return fail(VSEL_ERR_WORKSPACE, "workspace %zu bytes, need %zu", workspace_bytes, need);
  if ((uintptr_t)workspace & 255) return fail(VSEL_ERR_INVALID, "workspace must be 256-byte aligned");

  int32_t* meta = static_cast<int32_t*>(workspace);
  KvAppendArgs a{};
  a.q = static_cast<const uint16_t*>(q);
  a.q_bs = q_batch_stride; a.q_rs = q_row_stride; a.q_hs = q_head_stride;
  // the attention reads q in place when it is packed [B, s_q, Hq, d] and not rotated, else the workspace copy
  const bool q_packed = q_head_stride == d && (seqlen_q == 1 || q_row_stride == hq * d) && (batch == 1 || q_batch_stride == seqlen_q * hq * d);
  a.q_out = out && (rotary_cos || !q_packed) ? reinterpret_cast<uint16_t*>(static_cast<char*>(workspace) + kv_meta_bytes(batch)) : nullptr;
  a.k = static_cast<const uint16_t*>(k); a.v = static_cast<const uint16_t*>(v);
  a.k_bs = k_batch_stride; a.k_rs = k_row_stride; a.k_hs = k_head_stride;
  a.v_bs = v_batch_stride; a.v_rs = v_row_stride; a.v_hs = v_head_stride;
  a.k_cache = static_cast<uint16_t*>(k_cache); a.v_cache = static_cast<uint16_t*>(v_cache);
  a.cache_rows = cache_rows; a.cache_len = cache_len;
  a.block_table = block_table; a.max_pages = max_pages;
  a.cache_seqlens = cache_seqlens; a.seqlen_scalar = (int)cache_seqlen;
  a.batch_idx = cache_batch_idx; a.leftpad = cache_leftpad;
  a.rot_cos = rotary_cos; a.rot_sin = rotary_sin;
  a.rot_f32 = rotary_dtype == VSEL_F32; a.seqlen_ro = (int)seqlen_ro; a.rotary_dim = (int)rotary_dim; a.rot_interleaved = rotary_interleaved != 0;
  a.batch = (int)batch; a.s_q = (int)seqlen_q; a.s_new = (int)seqlen_new; a.hq = (int)hq; a.hkv = (int)hkv; a.d = (int)d; a.causal = causal != 0;
  a.cu_q = meta; a.seqlens_k = meta + batch + 1; a.cu_k = meta + 2 * batch + 1;

  hipStream_t st = (hipStream_t)stream;
  VSEL_PROF_BEGIN(st);
  const int rows = (int)std::max<int64_t>(1, std::max<int64_t>(seqlen_new, a.q_out ? seqlen_q : 0));
  VSEL_LAUNCH(kvcache_append_kernel, dim3((unsigned)batch, (unsigned)rows), dim3(256), 0, st, a);
  VSEL_AFTER_LAUNCH(st, "kvcache_append_kernel");
  if (!out) return VSEL_OK;                      // append only
  attn::PagedKV pg{a.seqlens_k, block_table, block_table ? nullptr : a.cu_k, (int)(block_table ? max_pages : 0),
             (int)(block_table ? cache_len : 1), 0, 0, 0, 0, 0, 0};
  return attn::attn_launch_cache(st, a.q_out ? a.q_out : q, k_cache, v_cache, a.cu_q, batch, seqlen_q, hq, hkv, d, scale, causal, out, pg, lse);
}
