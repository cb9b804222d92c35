#!/usr/bin/env python3
"""Same-process A/B of the bf16x3 projection forms (knob lis_proj_sum, include/vsel_debug.h): 0 = slab GEMM + finish kernel twice,
1 = split-K summed in LDS (two launches).  Forms alternated, two passes; per row: whole-step time from events, per-kernel time of the
projection launches from the library's HIP-event marks, bit identity of the outputs.
    python tools/ab_proj.py [--iters 20] [--rows 7b,3b,ov]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visionselector_amd import _native as N, ops  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


iters = int(arg("--iters", 20))
want = arg("--rows", "7b,3b,ov").split(",")
PROJ = ("gemm_nt_bf16x3_kernel", "kbar_finish_split_kernel", "gemm_nn_bf16x3_kernel", "w_finish_kernel")
# (row, d, hd, n, batches): the 7B geometry over the batch sweep, the 3B and LLaVA-OV rows of bench.bench_config_sweep
ROWS = [r for r in (("7b", 3584, 1792, 2304, (8, 16, 32, 64, 128)), ("3b", 2048, 1024, 576, (512,)), ("ov", 4096, 2048, 5832, (48,)))
        if r[0] in want]
for row, d, hd, n, batches in ROWS:
    g = torch.Generator(device="cuda").manual_seed(1234)
    wq, wk = [(0.02 * torch.randn(hd, d, device="cuda", generator=g)).bfloat16() for _ in range(2)]
    bq, bk = [(0.02 * torch.randn(hd, device="cuda", generator=g)).bfloat16() for _ in range(2)]
    k = max(1, int(n * 0.2))
    for b in batches:
        h = torch.randn(b, n, d, device="cuda", generator=g).bfloat16()
        ref = None
        for rnd in range(2):                     # two passes over the forms: order effects (clock, cache state) show as a spread
            for f in (0, 1):
                with N.debug_knob(lis_proj_sum=f, lis_small_path=0):
                    for _ in range(3):
                        out, idx, sc = ops.lis_select(h, wq, bq, wk, bk, k)
                    torch.cuda.synchronize()
                    if ref is None:
                        ref = (out.clone(), idx.clone(), sc.clone())
                    same = bool(torch.equal(out, ref[0]) and torch.equal(idx, ref[1]) and torch.equal(sc, ref[2]))
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        ops.lis_select(h, wq, bq, wk, bk, k)
                    e1.record()
                    torch.cuda.synchronize()
                    N.profile_start()
                    for _ in range(iters):
                        ops.lis_select(h, wq, bq, wk, bk, k)
                    torch.cuda.synchronize()
                    prof = N.profile_stop()
                    per = {kn: round(prof[kn][0] / max(1, prof[kn][1]) * 1e3, 1) for kn in PROJ if kn in prof}
                    print(json.dumps({"row": row, "images": b, "form": f, "pass": rnd, "step_us": round(e0.elapsed_time(e1) / iters * 1e3, 1),
                                      "proj_us": per, "proj_sum_us": round(sum(per.values()), 1), "identical": same}), flush=True)
        del h
        torch.cuda.empty_cache()
