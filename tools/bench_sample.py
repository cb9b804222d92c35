"""Top-k / top-p sampling: vsel_sample_tokens at kernel level, sampled packed_generate at model level.  One JSON line per measurement.

    python tools/bench_sample.py [--kernel] [--model] [--rows] [--batches 1,8,32] [--new-tokens 64]

Kernel level: V = 152 064 (Qwen2.5-VL), B in {1, 8, 32, 64}, bf16 and fp32, four settings (unfiltered, top_k 50, top_p 0.9, both) at
T = 0.7: ops.sample_tokens against HF's chain on the same tensors (TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper ->
softmax -> torch.multinomial).  Wall time per call from device events around 50 back-to-back calls; the library's device time from
its per-kernel profile (vsel_profile_*: host gaps excluded); the bytes one pass over the logits reads, and the passes the settings
take (1 + levels of the descents + 1).
Model level: the Qwen2.5-VL-7B-geometry selector model with random bf16 weights of tools/generate_common.py, B prompts of
2304 visual + 64 text tokens, budget 0.2, N new tokens; packed_generate greedy against do_sample (T 0.7, top_p 0.9; and with
top_k 50), no eos so that every run produces B x N tokens; runs alternate, best of two each.
--rows: ops.sample_tokens_rows (per-row parameters) at V = 152 064, bf16, B in {1, 8, 32, 64}, T = 0.7, unfiltered and
top_k 50 + top_p 0.9: (1) equal parameters on every row against ops.sample_tokens on the same logits, five alternating rounds of 50
calls each -- the spread of the scalar entry's own rounds is what a difference between the two has to exceed; (2) every other row greedy;
(3) with the log-probabilities, uniform and half-greedy -- profiles/sample_rows.jsonl."""
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
SETTINGS = {"unfiltered": dict(top_k=0, top_p=1.0), "top_k50": dict(top_k=50, top_p=1.0), "top_p0.9": dict(top_k=0, top_p=0.9),
            "top_k50_top_p0.9": dict(top_k=50, top_p=0.9)}


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


def rows_level():
    g = torch.Generator(device="cuda").manual_seed(0)
    t = 0.7
    for b in (1, 8, 32, 64):
        x = (torch.randn(b, V, device="cuda", generator=g) * 2.5).bfloat16()
        for name in ("unfiltered", "top_k50_top_p0.9"):
            kw = SETTINGS[name]
            uniform = dict(temperature=torch.full((b,), t, device="cuda"), top_p=torch.full((b,), kw["top_p"], device="cuda"),
                           top_k=torch.full((b,), kw["top_k"], dtype=torch.int32, device="cuda"), min_p=torch.zeros(b, device="cuda"))
            half = dict(uniform, temperature=uniform["temperature"] * (torch.arange(b, device="cuda") % 2 == 0))     # odd rows greedy
            step = [0]

            def scalar():
                step[0] += 1
                return ops.sample_tokens(x, t, seed=5, step=step[0], **kw)

            def rows(par=uniform, lp=False):
                step[0] += 1
                return ops.sample_tokens_rows(x, seed=5, step=step[0], return_logprobs=lp, **par)

            sc, ro = [], []
            for _ in range(5):                       # alternating rounds of the same run
                sc.append(_time_us(scalar))
                ro.append(_time_us(rows))
            rec = {"bench": "sample_rows", "dtype": "bf16", "batch": b, "vocab": V, "setting": name, "temperature": t, **kw,
                   "scalar_us_rounds": [round(u, 2) for u in sc], "rows_uniform_us_rounds": [round(u, 2) for u in ro],
                   "scalar_us": round(min(sc), 2), "scalar_spread_us": round(max(sc) - min(sc), 2), "rows_uniform_us": round(min(ro), 2),
                   "rows_vs_scalar": round(min(ro) / min(sc), 3),
                   "rows_uniform_logprob_us": round(min(_time_us(lambda: rows(uniform, True)) for _ in range(3)), 2),
                   "rows_half_greedy_us": round(min(_time_us(lambda: rows(half)) for _ in range(3)), 2),
                   "rows_half_greedy_logprob_us": round(min(_time_us(lambda: rows(half, True)) for _ in range(3)), 2)}
            _stamp(rec)


def model_level(batches, new_tokens):
    from visionselector_amd.generate import packed_generate
    model, prompts, pix, grid_t, n_vis, n_text = model_and_prompts(max(batches))
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
    ap.add_argument("--rows", action="store_true")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--new-tokens", type=int, default=64)
    a = ap.parse_args()
    if not a.kernel and not a.model and not a.rows:
        a.kernel = a.model = True
    if a.rows:
        rows_level()
    if a.kernel:
        kernel_level()
    if a.model:
        model_level([int(x) for x in a.batches.split(",")], a.new_tokens)
