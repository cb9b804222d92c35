"""Repetition penalty: vsel_repetition_penalty at kernel level, packed_generate with repetition_penalty at model level.  One JSON line per
measurement.

    python tools/bench_penalty.py [--kernel] [--model] [--batches 1,8,32] [--new-tokens 64]

Kernel level: V = 152 064 (Qwen2.5-VL), B in {1, 8, 32, 64}, bf16 and fp32 logits; each row's set holds 2 400 prompt ids plus 0-256
generated ids.  The greedy mode (penalty + argmax -> tokens) and the fp32-out mode (y for the sampler) against HF's chain on the same
logits (float(), RepetitionPenaltyLogitsProcessor on the [B, L + s] id matrix, argmax).  Wall time per call from device events around 50
back-to-back calls; the library's device time from its per-kernel profile (vsel_profile_*: host gaps excluded).
Model level: tools/generate_common.py's 7B-geometry selector model (random bf16 weights, B prompts of 2304 visual + 64 text tokens,
budget 0.2, N new tokens); packed_generate with repetition_penalty 1.05 against 1.0, greedy and sampled (T 0.7, top_p 0.9, top_k 50),
no eos so that every run produces B x N tokens; runs alternate, best of two each."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from generate_common import _stamp, _time_us, model_and_prompts  # noqa: E402
from visionselector_amd import _native as N  # noqa: E402
from visionselector_amd import ops  # noqa: E402

V = 152_064
PROMPT_IDS = 2400
THETA = 1.05


def hf_chain(x, ids, proc):
    return proc(ids, x.float()).argmax(-1)


def kernel_level():
    from transformers import RepetitionPenaltyLogitsProcessor
    proc = RepetitionPenaltyLogitsProcessor(penalty=THETA)
    g = torch.Generator(device="cuda").manual_seed(0)
    for dt, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        for b in (1, 8, 32, 64):
            x = (torch.randn(b, V, device="cuda", generator=g) * 2.5).to(dtype)
            rid = torch.arange(b, dtype=torch.int64, device="cuda")
            for gen in (0, 256):
                ids = torch.randint(0, V, (b, PROMPT_IDS + gen), device="cuda", generator=g)
                sets = ops.token_sets(list(ids.cpu()), V, "cuda")
                prev = ids[:, -1].contiguous()
                out = torch.empty(b, V, device="cuda")
                greedy = lambda: ops.repetition_penalty(x, THETA, sets, row_ids=rid, prev_tokens=prev, return_tokens=True)  # noqa: E731
                fp32 = lambda: ops.repetition_penalty(x, THETA, sets, row_ids=rid, prev_tokens=prev, out=out)  # noqa: E731
                assert torch.equal(greedy(), hf_chain(x, ids, proc))
                rec = {"bench": "penalty_kernel", "dtype": dt, "batch": b, "vocab": V, "set_ids": PROMPT_IDS + gen, "penalty": THETA}
                hf = _time_us(lambda: hf_chain(x, ids, proc), iters=20)
                rec["hf_chain_us"] = round(hf, 2)
                for mode, fn in (("greedy", greedy), ("fp32_out", fp32)):
                    wall = _time_us(fn)
                    N.profile_start()
                    for _ in range(20):
                        fn()
                    ms, calls = N.profile_stop()["repetition_penalty_kernel"]
                    rec[f"{mode}_us"] = round(wall, 2)
                    rec[f"{mode}_device_us"] = round(ms / calls * 1e3, 2)
                    rec[f"{mode}_speedup_vs_hf"] = round(hf / wall, 2)
                rec["row_bytes"] = V * x.element_size()
                _stamp(rec)


def model_level(batches, new_tokens):
    from visionselector_amd.generate import packed_generate
    model, prompts, pix, grid_t, n_vis, n_text = model_and_prompts(max(batches))
    sample = dict(do_sample=True, temperature=0.7, top_p=0.9, top_k=50, seed=1)
    modes = {"greedy": dict(), "greedy_rp1.05": dict(repetition_penalty=THETA), "sample": sample,
             "sample_rp1.05": dict(sample, repetition_penalty=THETA)}

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
        rec = {"bench": "penalty_generate", "batch": b, "visual_tokens": n_vis, "text_tokens": n_text, "budget": 0.2,
               "new_tokens": new_tokens, "model": "Qwen2.5-VL-7B geometry, random-init bf16", "sample": "T 0.7, top_p 0.9, top_k 50"}
        for m in modes:
            rec[f"{m}_s"] = round(best[m], 3)
            rec[f"{m}_tok_per_s"] = round(b * new_tokens / best[m], 1)
        rec["greedy_rp_vs_plain"] = round(best["greedy"] / best["greedy_rp1.05"], 3)
        rec["sample_rp_vs_plain"] = round(best["sample"] / best["sample_rp1.05"], 3)
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
