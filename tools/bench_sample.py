"""Top-k / top-p sampling: vsel_sample_tokens at kernel level, sampled packed_generate at model level.  One JSON line per measurement.

    python tools/bench_sample.py [--kernel] [--model] [--batches 1,8,32] [--new-tokens 64]

Kernel level: V = 152 064 (Qwen2.5-VL), B in {1, 8, 32, 64}, bf16 and fp32, four settings (unfiltered, top_k 50, top_p 0.9, both) at
T = 0.7: ops.sample_tokens against HF's chain on the same tensors (TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper ->
softmax -> torch.multinomial).  Wall time per call from device events around 50 back-to-back calls; the library's device time from
its per-kernel profile (vsel_profile_*: host gaps excluded); the bytes one pass over the logits reads, and the passes the settings
take (1 + levels of the descents + 1).
Model level: the Qwen2.5-VL-7B-geometry selector model with random bf16 weights as tools/bench_generate.py builds it, B prompts of
2304 visual + 64 text tokens, budget 0.2, N new tokens; packed_generate greedy against do_sample (T 0.7, top_p 0.9; and with
top_k 50), no eos so that every run produces B x N tokens; runs alternate, best of two each."""
import argparse
import json
import os
import socket
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visionselector_amd import _native as N  # noqa: E402
from visionselector_amd import ops  # noqa: E402

V = 152_064
SETTINGS = {"unfiltered": dict(top_k=0, top_p=1.0), "top_k50": dict(top_k=50, top_p=1.0), "top_p0.9": dict(top_k=0, top_p=0.9),
            "top_k50_top_p0.9": dict(top_k=50, top_p=0.9)}


def _stamp(rec):
    rec.update(box=f"{socket.gethostname()} / {torch.cuda.get_device_name(0)}", commit=os.environ.get("VSEL_COMMIT", "unknown"))
    print(json.dumps(rec), flush=True)


def _time_us(fn, iters=50, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def hf_chain(x, temperature, top_k, top_p, gen):
    from transformers import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = TemperatureLogitsWarper(temperature)(None, x)
    if top_k > 0:
        s = TopKLogitsWarper(top_k)(None, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(top_p)(None, s)
    return torch.multinomial(torch.softmax(s.float(), dim=-1), 1, generator=gen)[:, 0]


def kernel_level():
    g = torch.Generator(device="cuda").manual_seed(0)
    hg = torch.Generator(device="cuda").manual_seed(1)
    t = 0.7
    for dt, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        levels = 2 if dt == "bf16" else 4
        for b in (1, 8, 32, 64):
            x = (torch.randn(b, V, device="cuda", generator=g) * 2.5).to(dtype)
            for name, kw in SETTINGS.items():
                passes = 2 + (levels if kw["top_k"] else 0) + ((levels - 1 if kw["top_k"] else levels) if kw["top_p"] < 1 else 0)
                step = [0]

                def ours():
                    step[0] += 1
                    return ops.sample_tokens(x, t, seed=5, step=step[0], **kw)

                wall = _time_us(ours)
                hf = _time_us(lambda: hf_chain(x, t, kw["top_k"], kw["top_p"], hg), iters=20)
                ours()
                torch.cuda.synchronize()
                N.profile_start()
                for _ in range(20):
                    ours()
                ms, calls = N.profile_stop()["sample_tokens_kernel"]
                dev_us = ms / calls * 1e3
                _stamp({"bench": "sample_kernel", "dtype": dt, "batch": b, "vocab": V, "setting": name, "temperature": t, **kw,
                        "sample_tokens_us": round(wall, 2), "kernel_device_us": round(dev_us, 2), "hf_chain_us": round(hf, 2),
                        "speedup_vs_hf": round(hf / wall, 2), "row_bytes": V * x.element_size(), "passes": passes})


def build_model():
    """tools/bench_generate.py's model: Qwen2.5-VL-7B geometry, random bf16 weights, B prompts of 2304 visual + 64 text tokens"""
    from transformers import Qwen2_5_VLConfig
    from visionselector_amd.attention import ATTN_NAME, ATTN_NAME_PACKED, replace_qwen2_vl_attention_class
    from visionselector_amd.hf_qwen25vl import Qwen2_5_VLForConditionalGeneration_Selector
    IMG, VID, VSTART, VEND = 151655, 151656, 151652, 151653
    replace_qwen2_vl_attention_class()
    cfg = Qwen2_5_VLConfig(
        text_config=dict(hidden_size=3584, intermediate_size=18944, num_hidden_layers=28, num_attention_heads=28,
                         num_key_value_heads=4, vocab_size=152064, max_position_embeddings=32768,
                         rope_parameters=dict(rope_type="default", mrope_section=[16, 24, 24], rope_theta=1000000.0)),
        vision_config=dict(depth=32, hidden_size=1280, num_heads=16, intermediate_size=3420, out_hidden_size=3584, patch_size=14,
                           spatial_merge_size=2, temporal_patch_size=2, window_size=112, fullatt_block_indexes=[7, 15, 23, 31],
                           in_channels=3),
        image_token_id=IMG, video_token_id=VID, vision_start_token_id=VSTART, vision_end_token_id=VEND)
    torch.manual_seed(0)
    torch.set_default_dtype(torch.bfloat16)
    with torch.device("cuda"):
        model = Qwen2_5_VLForConditionalGeneration_Selector(cfg).eval()
    torch.set_default_dtype(torch.float32)
    model.model.language_model.config._attn_implementation = ATTN_NAME
    model.model.visual.config._attn_implementation = ATTN_NAME_PACKED
    with torch.no_grad():
        for p in model.visual.importance_scorer.parameters():
            p.copy_(0.02 * torch.randn_like(p))
    model.visual.budgets = 0.2
    n_vis, n_text = 96 * 96 // 4, 64
    g = torch.Generator().manual_seed(1)
    prompts, pix = [], []
    return model, prompts, pix, (IMG, VSTART, VEND, n_vis, n_text, g)


def model_level(batches, new_tokens):
    from visionselector_amd.generate import packed_generate
    model, prompts, pix, (IMG, VSTART, VEND, n_vis, n_text, g) = build_model()
    for _ in range(max(batches)):
        pre = torch.randint(1000, 5000, (n_text // 2,), generator=g)
        post = torch.randint(1000, 5000, (n_text - n_text // 2 - 2,), generator=g)
        prompts.append(torch.cat((pre, torch.tensor([VSTART]), torch.full((n_vis,), IMG), torch.tensor([VEND]), post)))
        pix.append(torch.randn(96 * 96, 3 * 2 * 14 * 14, generator=g).bfloat16())
    grid_t = torch.tensor([[1, 96, 96]]).cuda()
    modes = {"greedy": dict(), "sample_t0.7_p0.9": dict(do_sample=True, temperature=0.7, top_p=0.9, seed=1),
             "sample_t0.7_p0.9_k50": dict(do_sample=True, temperature=0.7, top_p=0.9, top_k=50, seed=1)}

    def run(b, n, kw):
        out = packed_generate(model, prompts[:b], torch.cat(pix[:b]).cuda(), grid_t.repeat(b, 1), [1] * b, max_new_tokens=n, **kw)
        assert all(len(t) == n for t in out["tokens"])

    for b in batches:
        for kw in modes.values():
            run(b, 2, kw)                       # warm-up at this batch's shapes
        best = {m: float("inf") for m in modes}
        for _ in range(2):
            for m, kw in modes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(b, new_tokens, kw)
                torch.cuda.synchronize()
                best[m] = min(best[m], time.perf_counter() - t0)
        rec = {"bench": "sample_generate", "batch": b, "visual_tokens": n_vis, "text_tokens": n_text, "budget": 0.2,
               "new_tokens": new_tokens, "model": "Qwen2.5-VL-7B geometry, random-init bf16"}
        for m in modes:
            rec[f"{m}_s"] = round(best[m], 3)
            rec[f"{m}_tok_per_s"] = round(b * new_tokens / best[m], 1)
        for m in list(modes)[1:]:
            rec[f"{m}_vs_greedy"] = round(best["greedy"] / best[m], 3)
        _stamp(rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--new-tokens", type=int, default=64)
    a = ap.parse_args()
    if not a.kernel and not a.model:
        a.kernel = a.model = True
    if a.kernel:
        kernel_level()
    if a.model:
        model_level([int(x) for x in a.batches.split(",")], a.new_tokens)
