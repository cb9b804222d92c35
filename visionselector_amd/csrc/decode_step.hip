// Decode-step bookkeeping on the device (gfx950): vsel_decode_advance.  What packed_generate's eager loop does on the host after every
// selector launch -- append the token, test eos and the length limit, advance cache_seqlens and the M-RoPE positions, notice the
// sampler's -1 -- as ONE launch that reads and writes device memory only, so the loop never reads a token on the host.
//   rows    state per row: done (0 active, 1 eos, 2 length, 3 invalid logits), n_tokens, cache_seqlens, pos[3], feed (the token the next
//           LLM step embeds), tokens_out[max_new_tokens].  A row with done != 0 on entry changes nothing, ever: later replays of the
//           LLM step rewrite one cache slot of that row's own pages with the same values (the frozen-row invariant).
//   active  n_tokens > 0 on entry: the row's previous token went through the LLM since the last advance, so cache_seqlens += 1 and
//           pos += 1.  Then t = next[b]: t < 0 -> done = 3; else tokens_out[b, n_tokens] = t, n_tokens += 1, and done = 1 if t is in eos,
//           else done = 2 if n_tokens == max_new_tokens, else feed[b] = t.  An active row whose n_tokens is outside [0, max_new_tokens)
//           (a corrupt state: device values are not trusted with addresses) stops with done = 2 and writes nothing else.
//   status  {rows still active after this launch, lowest row that turned invalid in this launch or -1, that row's n_tokens or -1, 0}.
// One 256-thread workgroup, rows in a strided loop, the three status words reduced over the wave and then in LDS: B is at most a few
// hundred, the launch is latency.  Plain vector stores, no atomics, no workspace, nothing that breaks stream capture.
#include "common.h"

namespace vsel {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;

struct AdvanceArgs {
  const int64_t* next;
  const int64_t* eos;
  int64_t batch, n_eos, max_new;
  int32_t* done;
  int32_t* n_tokens;
  int32_t* seqlens;
  void* pos;
  int pos_i64;
  int64_t* feed;
  int64_t* tokens_out;
  int32_t* status;
};

__global__ __launch_bounds__(kThreads) void decode_advance_kernel(AdvanceArgs a) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  int active = 0;
  int64_t bad_row = INT64_MAX;          // lowest row of this thread that turned invalid
  int bad_step = -1;
  for (int64_t b = tid; b < a.batch; b += kThreads) {
    if (a.done[b] != 0) continue;
    int n = a.n_tokens[b];
    if (n < 0 || n >= a.max_new) {
      a.done[b] = 2;
      continue;
    }
    if (n > 0) {
      a.seqlens[b] += 1;
      if (a.pos_i64) {
        int64_t* p = static_cast<int64_t*>(a.pos);
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c * a.batch + b] += 1;
      } else {
        int32_t* p = static_cast<int32_t*>(a.pos);
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c * a.batch + b] += 1;
      }
    }
    const int64_t t = a.next[b];
    if (t < 0) {
      a.done[b] = 3;
      if (b < bad_row) { bad_row = b; bad_step = n; }
      continue;
    }
    a.tokens_out[b * a.max_new + n] = t;
    n += 1;
    a.n_tokens[b] = n;
    bool is_eos = false;
    for (int64_t e = 0; e < a.n_eos; ++e) is_eos |= a.eos[e] == t;
    if (is_eos) {
      a.done[b] = 1;
    } else if (n == a.max_new) {
      a.done[b] = 2;
    } else {
      a.feed[b] = t;
      active += 1;
    }
  }
  // workgroup reduction: sum of active, (row, step) of the lowest invalid row
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    active += __shfl_xor(active, o, kWave);
    const int64_t orow = __shfl_xor(bad_row, o, kWave);
    const int ostep = __shfl_xor(bad_step, o, kWave);
    if (orow < bad_row) { bad_row = orow; bad_step = ostep; }
  }
  __shared__ int red_active[kWaves];
  __shared__ int64_t red_row[kWaves];
  __shared__ int red_step[kWaves];
  if (lane == 0) { red_active[wave] = active; red_row[wave] = bad_row; red_step[wave] = bad_step; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kWaves; ++w) {
      active += red_active[w];
      if (red_row[w] < bad_row) { bad_row = red_row[w]; bad_step = red_step[w]; }
    }
    const bool any_bad = bad_row != INT64_MAX;
    a.status[0] = active;
    a.status[1] = any_bad ? (int32_t)bad_row : -1;
    a.status[2] = any_bad ? bad_step : -1;
    a.status[3] = 0;
  }
}

}  // namespace

}  // namespace vsel

using namespace vsel;

extern "C" int vsel_decode_advance(void* stream, const int64_t* next, int64_t batch, const int64_t* eos, int64_t n_eos,
                                   int64_t max_new_tokens, int32_t* done, int32_t* n_tokens, int32_t* cache_seqlens, void* pos,
                                   int pos_is_int64, int64_t* feed, int64_t* tokens_out, int32_t* status) {
  if (!next || !done || !n_tokens || !cache_seqlens || !pos || !feed || !tokens_out || !status)
    return fail(VSEL_ERR_INVALID, "NULL next / done / n_tokens / cache_seqlens / pos / feed / tokens_out / status");
  if (batch < 0 || n_eos < 0 || max_new_tokens < 1)
    return fail(VSEL_ERR_INVALID, "bad shape (batch=%lld n_eos=%lld max_new_tokens=%lld)", (long long)batch, (long long)n_eos,
                (long long)max_new_tokens);
  if (n_eos > 0 && !eos) return fail(VSEL_ERR_INVALID, "NULL eos with n_eos=%lld", (long long)n_eos);
  if (pos_is_int64 != 0 && pos_is_int64 != 1) return fail(VSEL_ERR_INVALID, "pos_is_int64 must be 0 or 1");
  if (batch > INT32_MAX || max_new_tokens > INT32_MAX)
    return fail(VSEL_ERR_UNSUPPORTED, "batch %lld / max_new_tokens %lld > 2^31 - 1", (long long)batch, (long long)max_new_tokens);

  AdvanceArgs a{};
  a.next = next;
  a.eos = eos;
  a.batch = batch;
  a.n_eos = n_eos;
  a.max_new = max_new_tokens;
  a.done = done;
  a.n_tokens = n_tokens;
  a.seqlens = cache_seqlens;
  a.pos = pos;
  a.pos_i64 = pos_is_int64;
  a.feed = feed;
  a.tokens_out = tokens_out;
  a.status = status;
  hipStream_t st = (hipStream_t)stream;
  // batch == 0 still launches: status must say "no row active"
  VSEL_LAUNCH(decode_advance_kernel, dim3(1), dim3(kThreads), 0, st, a);
  VSEL_AFTER_LAUNCH(st, "decode_advance_kernel");
  return VSEL_OK;
}
