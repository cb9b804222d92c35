"""Decode on a KV cache: flash_attn_with_kvcache at kernel level, packed_generate at model level.  One JSON line per measurement.

    python tools/bench_generate.py [--kernel] [--model] [--graph] [--batches 1,8,32] [--new-tokens 64] [--repeats 3] [--lookaheads 1,2,4,8]

Kernel level (7B heads: 28 q / 4 kv, d 128, s_q = s_new = 1): B in {1, 8, 32, 64, 256} x cache length in {524, 2368}, three
layouts -- paged (page 64, scattered pages), contiguous, contiguous with left padding (cache_leftpad + cache_batch_idx) --
against ops.paged_attn over the same number of keys on the same kind of pages (the attention launch alone).  The append launch
is timed on its own (append-only call) and, from the library's per-kernel profile (device time, host gaps excluded), priced by
the bytes it moves: the new K / V rows read and written, 2 x 2 x B x Hkv x d x 2 bytes, plus 16 bytes of metadata per row.
Model level: the Qwen2.5-VL-7B-geometry selector model with random bf16 weights of tools/generate_common.py, B prompts
of 2304 visual tokens + 64 text tokens, budget 0.2, N new tokens: packed_generate tokens/s against B sequential batch-1
model.generate() calls (greedy, min_new_tokens = max_new_tokens so that both produce the same count).
--graph: the same model and prompts, packed_generate(graph=False) against packed_generate(graph=DecodeGraphs) in one process,
alternating, warmed up, best of --repeats each, the captured graphs reused across repeats and the capture time reported apart; then the
lookahead sweep (graph mode only) at the smallest and the largest batch.  ms per decode step = (best time - best prefill-only time) /
(new tokens - 1); tok/s counts the whole call, prefill included, as the --model leg does.
Every line carries the box (host, device) and the commit (VSEL_COMMIT, since the tree may travel without its .git)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from generate_common import IMG, _stamp, _time_us, model_and_prompts  # noqa: E402
from visionselector_amd import _native as N  # noqa: E402
from visionselector_amd import ops  # noqa: E402
from visionselector_amd.flash_attn_compat import flash_attn_with_kvcache  # noqa: E402

HQ, HKV, D, PAGE = 28, 4, 128, 64


def kernel_level():
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).bfloat16()  # noqa: E731
    for b in (1, 8, 32, 64, 256):
        for lk in (524, 2368):
            q, k, v = rnd(b, 1, HQ, D), rnd(b, 1, HKV, D), rnd(b, 1, HKV, D)
            end = torch.full((b,), lk - 1, dtype=torch.int32, device="cuda")          # lk visible keys after the append
            # paged: scattered pages, -1-padded tables
            per = -(-lk // PAGE)
            n_pages = b * per
            kp, vp = rnd(n_pages, PAGE, HKV, D), rnd(n_pages, PAGE, HKV, D)
            bt = torch.full((b, per + 1), -1, dtype=torch.int32, device="cuda")
            bt[:, :per] = torch.randperm(n_pages, device="cuda", generator=g).to(torch.int32).view(b, per)
            # contiguous: [B, L_cache, Hkv, d]; left-padded: 64 leading pad positions, rows permuted through cache_batch_idx
            kc, vc = rnd(b, lk, HKV, D), rnd(b, lk, HKV, D)
            pad = 64
            kl, vl = rnd(b + 1, lk + pad, HKV, D), rnd(b + 1, lk + pad, HKV, D)
            bidx = torch.randperm(b + 1, device="cuda", generator=g)[:b].to(torch.int32)
            lp = torch.full((b,), pad, dtype=torch.int32, device="cuda")
            cu_q = torch.arange(0, b + 1, dtype=torch.int32, device="cuda")
            klens = torch.full((b,), lk, dtype=torch.int32, device="cuda")
            base = _time_us(lambda: ops.paged_attn(q.view(b, HQ, D), kp, vp, cu_q, klens, bt, 1))
            rec = {"bench": "kvcache_decode", "batch": b, "cache_len": lk, "heads": f"{HQ}/{HKV}", "d": D,
                   "paged_attn_us": round(base, 2)}
            for tag, fn in (("paged64", lambda: flash_attn_with_kvcache(q, kp, vp, k, v, cache_seqlens=end, block_table=bt, causal=True)),
                            ("contiguous", lambda: flash_attn_with_kvcache(q, kc, vc, k, v, cache_seqlens=end, causal=True)),
                            ("contiguous_leftpad", lambda: flash_attn_with_kvcache(q, kl, vl, k, v, cache_seqlens=end + pad, cache_leftpad=lp,
                                                                                   cache_batch_idx=bidx, causal=True))):
                rec[f"{tag}_us"] = round(_time_us(fn), 2)
                rec[f"{tag}_vs_paged_attn"] = round(rec[f"{tag}_us"] / base, 3)
            app = _time_us(lambda: ops.kvcache_attn(None, kp, vp, k=k, v=v, cache_seqlens=end, block_table=bt))
            rec["append_only_call_us"] = round(app, 2)
            # device time per launch (libvsel's event brackets around each kernel, host gaps excluded): the wall times above are
            # host-bound at small B (one Python call per launch)
            for tag, fn in (("paged_attn", lambda: ops.paged_attn(q.view(b, HQ, D), kp, vp, cu_q, klens, bt, 1)),
                            ("paged64", lambda: flash_attn_with_kvcache(q, kp, vp, k, v, cache_seqlens=end, block_table=bt, causal=True)),
                            ("contiguous_leftpad", lambda: flash_attn_with_kvcache(q, kl, vl, k, v, cache_seqlens=end + pad, cache_leftpad=lp,
                                                                                   cache_batch_idx=bidx, causal=True))):
                fn()
                torch.cuda.synchronize()
                N.profile_start()
                for _ in range(20):
                    fn()
                prof = N.profile_stop()
                ms, calls = prof["varlen_attn_fwd_kernel"]
                rec[f"{tag}_attn_kernel_us"] = round(ms / calls * 1e3, 2)
                if "kvcache_append_kernel" in prof:
                    ms, calls = prof["kvcache_append_kernel"]
                    rec[f"{tag}_append_kernel_us"] = round(ms / calls * 1e3, 2)
            moved = 2 * 2 * b * HKV * D * 2 + 4 * 4 * b
            ak = rec["paged64_append_kernel_us"]
            rec.update(append_bytes=moved, append_GBps=round(moved / ak / 1e3, 2),
                       append_share_of_paged64_device=round(ak / (ak + rec["paged64_attn_kernel_us"]), 3),
                       leftpad_attn_vs_paged_attn_device=round(rec["contiguous_leftpad_attn_kernel_us"] / rec["paged_attn_attn_kernel_us"], 3))
            _stamp(rec)


def model_level(batches, new_tokens):
    from visionselector_amd.generate import packed_generate
    model, prompts, pix, grid_t, n_vis, n_text = model_and_prompts(max(batches))

    def packed(b, n=new_tokens):
        out = packed_generate(model, prompts[:b], torch.cat(pix[:b]).cuda(), grid_t.repeat(b, 1), [1] * b, max_new_tokens=n)
        assert all(len(t) == n for t in out["tokens"])

    def sequential(b):
        for i in range(b):
            ids = prompts[i][None].cuda()
            model.model.rope_deltas = None
            with torch.no_grad():
                model.generate(input_ids=ids, attention_mask=torch.ones_like(ids), pixel_values=pix[i].cuda(), image_grid_thw=grid_t,
                               mm_token_type_ids=(ids == IMG).int(), max_new_tokens=new_tokens, min_new_tokens=new_tokens, do_sample=False)

    sequential(1)                                                   # warm-up (kernels, allocator, library heuristics)
    for b in batches:
        packed(b, 2)            # warm-up at this batch's shapes (the tower's first call at a new image count costs seconds)
        res = {"bench": "packed_generate", "batch": b, "visual_tokens": n_vis, "text_tokens": n_text, "budget": 0.2,
               "new_tokens": new_tokens, "model": "Qwen2.5-VL-7B geometry, random-init bf16"}
        for tag, fn in (("packed_generate", packed), ("sequential_generate", sequential)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(b)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
            res[f"{tag}_s"] = round(s, 3)
            res[f"{tag}_tok_per_s"] = round(b * new_tokens / s, 1)
        res["speedup"] = round(res["sequential_generate_s"] / res["packed_generate_s"], 2)
        _stamp(res)


def graph_level(batches, new_tokens, repeats, lookaheads):
    from visionselector_amd.generate import DEFAULT_LOOKAHEAD, DecodeGraphs, PagedKVPool, packed_generate
    model, prompts, pix, grid_t, n_vis, n_text = model_and_prompts(max(batches))
    lm = model.model.language_model
    length = n_text + max(1, int(n_vis * 0.2))
    width = -(-(length + new_tokens - 1) // PAGE)
    pool = PagedKVPool(len(lm.layers), max(batches) * width, PAGE, HKV, D, "cuda")
    graphs = DecodeGraphs(model, pool, width)

    def run(b, n=new_tokens, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = packed_generate(model, prompts[:b], torch.cat(pix[:b]).cuda(), grid_t.repeat(b, 1), [1] * b, max_new_tokens=n, pool=pool, **kw)
        torch.cuda.synchronize()
        assert all(len(t) == n for t in out["tokens"])
        return time.perf_counter() - t0, out["tokens"]

    def line(b, best, prefill):
        return {"s": round(best, 4), "tok_per_s": round(b * new_tokens / best, 1),
                "ms_per_decode_step": round((best - prefill) / (new_tokens - 1) * 1e3, 3)}

    for b in batches:
        run(b, 2)                   # warm-up at this batch's shapes (the tower's first call at a new image count costs seconds)
        before = graphs.capture_ms
        run(b, 2, graph=graphs)     # captures this batch's graph
        res = {"bench": "packed_generate_graph", "batch": b, "visual_tokens": n_vis, "text_tokens": n_text, "budget": 0.2,
               "new_tokens": new_tokens, "repeats": repeats, "lookahead": DEFAULT_LOOKAHEAD, "model": "Qwen2.5-VL-7B geometry, random-init bf16",
               "capture_ms": round(graphs.capture_ms - before, 1)}
        prefill = min(run(b, 1)[0] for _ in range(repeats))
        best = {"eager": float("inf"), "graph": float("inf")}
        for _ in range(repeats):     # alternating
            for tag, kw in (("eager", dict()), ("graph", dict(graph=graphs))):
                s, toks = run(b, **kw)
                best[tag] = min(best[tag], s)
                res.setdefault("tokens_equal", True)
                if tag == "eager":
                    ref = toks
                elif toks != ref:
                    res["tokens_equal"] = False
        res["prefill_only_s"] = round(prefill, 4)
        res["eager"], res["graph"] = line(b, best["eager"], prefill), line(b, best["graph"], prefill)
        res["graph_vs_eager"] = round(best["eager"] / best["graph"], 3)
        res["captures"] = graphs.captures
        _stamp(res)
    for b in sorted({batches[0], batches[-1]}) if lookaheads else ():
        res = {"bench": "packed_generate_graph_lookahead", "batch": b, "new_tokens": new_tokens, "repeats": repeats}
        prefill = min(run(b, 1)[0] for _ in range(repeats))
        for la in lookaheads:
            res[f"lookahead_{la}"] = line(b, min(run(b, graph=graphs, lookahead=la)[0] for _ in range(repeats)), prefill)
        _stamp(res)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lookaheads", default="1,2,4,8", help="the sweep of --graph ('' to skip it)")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--new-tokens", type=int, default=64)
    a = ap.parse_args()
    if not a.kernel and not a.model and not a.graph:
        a.kernel = a.model = True
    if a.kernel:
        kernel_level()
    if a.model:
        model_level([int(x) for x in a.batches.split(",")], a.new_tokens)
    if a.graph:
        graph_level([int(x) for x in a.batches.split(",")], a.new_tokens, a.repeats, [int(x) for x in a.lookaheads.split(",") if x])
