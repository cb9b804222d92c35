#!/usr/bin/env python3
"""LM loss leg of the training forward on one MI355X: visionselector_amd.loss.causal_lm_loss (fused HIP cross-entropy)
against transformers' ForCausalLMLoss on the same tensors.  V = 152 064 bf16 logits of one packed sample, rows 512 / 2 048 / 8 192, with
every row valid and with the last quarter valid (an SFT sample: prompt and image placeholders carry -100).  Forward and forward +
backward, HIP-event timed, the two paths alternating in rounds inside one process; peak-memory deltas of one call of each; the
library's own per-kernel times from one instrumented call.  One JSON line per shape (default profiles/lm_loss.jsonl).

Compulsory bytes: the valid rows read once in the forward and once in the backward, the gradient written once.  `hbm_frac_*` is those
bytes over the time over 8 TB/s."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformers.loss.loss_utils import ForCausalLMLoss  # noqa: E402

from visionselector_amd import _native  # noqa: E402
from visionselector_amd.loss import causal_lm_loss  # noqa: E402

HBM = 8e12


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                          # us per call


def peak_delta(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[512, 2048, 8192])
    ap.add_argument("--valid", type=float, nargs="*", default=[1.0, 0.25])
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=150.0, help="work per timed window")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lm_loss.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_loss.py needs the GPU: there is nothing to time without one")
    v = a.vocab
    lines = []
    for rows in a.rows:
        g = torch.Generator(device="cuda").manual_seed(rows)
        logits = torch.randn(1, rows, v, device="cuda", generator=g).bfloat16().requires_grad_(True)
        ids = torch.randint(0, v, (1, rows), device="cuda", generator=g)
        for frac in a.valid:
            labels = ids.clone()
            labels[:, :rows - int(rows * frac)] = -100
            n_valid = int((labels[:, 1:] != -100).sum())

            def fwd(loss_fn):
                with torch.no_grad():
                    return loss_fn(logits, labels, v)

            def both(loss_fn):
                logits.grad = None
                loss_fn(logits, labels, v).backward()

            arms = {"fused_fwd": lambda: fwd(causal_lm_loss), "hf_fwd": lambda: fwd(ForCausalLMLoss),
                    "fused_fwd_bwd": lambda: both(causal_lm_loss), "hf_fwd_bwd": lambda: both(ForCausalLMLoss)}
            iters = {}
            for k, fn in arms.items():                                # warm-up, then a pilot that sizes the window
                fn()
                fn()
                iters[k] = max(3, min(200, int(a.window_ms * 1e3 / max(timed(fn, 3), 1.0))))
            us = {k: [] for k in arms}
            for _ in range(a.rounds):                                 # the arms alternate inside every round
                for k, fn in arms.items():
                    us[k].append(timed(fn, iters[k]))
            loss_f, loss_h = float(fwd(causal_lm_loss)), float(fwd(ForCausalLMLoss))
            mem = {k: peak_delta(fn) for k, fn in arms.items()}
            logits.grad = None
            _native.profile_start()
            both(causal_lm_loss)
            torch.cuda.synchronize()
            kern = {k: round(ms / n * 1e3, 1) for k, (ms, n) in _native.profile_stop().items()}
            logits.grad = None
            med = {k: statistics.median(x) for k, x in us.items()}
            row_bytes = v * 2
            b_fwd, b_both = n_valid * row_bytes, 2 * n_valid * row_bytes + rows * row_bytes
            line = {"rows": rows, "vocab": v, "dtype": "bf16", "valid_frac": frac, "valid_rows": n_valid, "rounds": a.rounds, "iters": iters,
                    "us_median": {k: round(x, 1) for k, x in med.items()}, "us_min": {k: round(min(x), 1) for k, x in us.items()},
                    "speedup_fwd": round(med["hf_fwd"] / med["fused_fwd"], 2),
                    "speedup_fwd_bwd": round(med["hf_fwd_bwd"] / med["fused_fwd_bwd"], 2),
                    "compulsory_bytes": {"fwd": b_fwd, "fwd_bwd": b_both},
                    "hbm_frac_fwd": round(b_fwd / (med["fused_fwd"] * 1e-6) / HBM, 3),
                    "hbm_frac_fwd_bwd": round(b_both / (med["fused_fwd_bwd"] * 1e-6) / HBM, 3),
                    "kernel_us_instrumented": kern,
                    "hbm_frac_kernels": {"fwd": round(b_fwd / (kern["token_logprob_fwd_kernel"] * 1e-6) / HBM, 3),
                                         "bwd": round((b_fwd + rows * row_bytes) / (kern["token_logprob_bwd_kernel"] * 1e-6) / HBM, 3)},
                    "peak_bytes": mem, "logits_bytes": rows * row_bytes, "loss": {"fused": loss_f, "hf": loss_h}}
            print(json.dumps(line), flush=True)
            lines.append(line)
        del logits, ids
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
