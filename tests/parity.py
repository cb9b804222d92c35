"""Parity bookkeeping shared by the -m gpu tests: error measures in bf16 ulps and a JSONL log of the observed margins.

north_star states "attention outputs within 1e-3 bf16".  A bf16 STORE alone is off by up to 2^-9 = 1.95e-3 relative, so
the comparison is made where that statement is meaningful: the kernel's bf16 output against the fp64 oracle ROUNDED TO
bf16, counted in bf16 ulps (1 ulp = 2^-8 relative).  The gated ulp is taken at the scale of the element's output ROW
(largest |ref| of that (token, head) vector): an attention output is a convex combination of V rows whose probabilities
are rounded to bf16 before P.V (as flash-attn does), so its error is bounded by 2^-9 * max|V| -- it scales with the
summands, not with an element that happens to cancel towards 0.  Also logged, not gated: ulps at the element's own
magnitude and with the floor rowmax / 8, the fraction of bit-equal elements, max / mean |err| against the un-rounded oracle.
Every call appends the observed numbers to gpurun_out/parity/<round>.jsonl (merged into profiles/ by tools/merge_parity.py).
"""
from __future__ import annotations

import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND = "r04"
LOG = os.path.join(ROOT, "gpurun_out", "parity", f"{ROUND}_parity.jsonl")

MAX_ULP_FWD = 1.0        # gate: every element within 1 bf16 ulp (ulp at its row's scale) of the bf16-rounded oracle
MAX_ULP_ROW8_FWD = 8.0   # gate: the same error counted with the ulp floor at rowmax / 8 (an element 8x below its row's
                         # largest may be off by 1 row-scale ulp = 8 of its own; beyond that the error model is violated)
MIN_FRAC_1ULP_ROW8 = 0.93  # gate: share of elements within ONE ulp at that finer scale (observed minimum 0.954, round 2)
MEAN_ABS_FWD = 1e-3      # gate: mean |err| vs the un-rounded fp64 oracle

# The reference's own bf16 run (tests/golden/lisbf16_*.npz: modules and tokens in bfloat16, every op rounding to bf16)
# against the build's bf16-storage / fp32-accumulate path.  north_star: "soft scores ... within 1e-3 bf16".
BF16_SCORE_TOL = 1e-3    # |score - reference bf16 score| <= 1e-3 * max(1, max|score|)
BF16_IDX_FRAC = 0.01     # |idx (sym.diff) reference bf16 idx| <= max(2 * ties at the k-th value, 1 % of k)
# (the DEFAULT soft top-k returns the fp32 root; the opt-in vsel_soft_topk_fwd_bf16ref restates the reference's bf16 arithmetic and matches
# its fixtures bit for bit on the same scores -- tests/test_lis_gpu.py, tests/test_oracle_golden.py)
BF16_PS_TOL = 3e-3       # soft mask: the reference's bf16 bisection stalls at bf16 spacing of t (|dt| <= 2^-7 -> |dp| <= 2e-3)
                         # and its p is rounded to bf16 (<= 2^-9 relative = 2e-3 near 1); observed worst 2.2e-3
                         # (profiles/r03_parity.json), logged every run

# The reference's bf16 BACKWARD (lisbf16_*.npz `topk_grad_bf16`, `bwd_*`: TopK.backward and the training block's autograd with
# bf16 modules / tokens, every op and every accumulated gradient rounded to bf16) against the build's bf16-storage /
# fp32-accumulate backward.  Errors are max |got - ref| / max |ref| per quantity; the reference's own bf16 run sits 0.5-3 %
# (one projection of the rank-1 dWq at N = 5832: 15 %) from its fp32 run, which is what these gates have to admit.
# Gates = 2 x the worst margin observed on MI355X over the five shapes (profiles/r04_parity.json: topk_grad 0.0093, dbk 0.0087,
# dWq.u 0.029, v.dWq 0.142, dWk.u 0.015, v.dWk 0.038, dx.u 0.0090, v.dx 0.0063, dense dWq / dWk / dx (tiny) 0.0043 / 0.0055 / 0.0098,
# |dbq| / max|dbk| 0.0008); the fp64 closed form sits at the same distances (tests/test_oracle_golden.py), i.e. the margins ARE
# the reference's bf16 rounding.
# NOT a parity gate: a NOISE BOUND.  A 30 % bound (v_dwq) only catches gross errors on that projection; the gate proper of the
# backward is the fp32 golden test (tests/test_train_gpu.py::test_train_backward_golden, <= 1e-5 / 2e-5) on the same kernels.
BF16_BWD_TOL = {"topk_grad": 0.02, "dbk": 0.02, "dwq_u": 0.06, "v_dwq": 0.30, "dwk_u": 0.03, "v_dwk": 0.08, "dx_u": 0.02,
                "v_dx": 0.015, "dwq": 0.01, "dwk": 0.012, "dx": 0.02, "dbq_over_dbk": 0.002}


def bf16_round(x: np.ndarray) -> np.ndarray:
    """fp64 -> nearest bf16 (ties to even) -> fp64."""
    f = np.asarray(x, dtype=np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def bf16_ulp(mag: np.ndarray) -> np.ndarray:
    """Spacing of bf16 numbers at magnitude `mag` (8 significand bits): 2^(floor(log2 mag) - 7)."""
    mag = np.maximum(np.asarray(mag, dtype=np.float64), 2.0 ** -100)
    return 2.0 ** (np.floor(np.log2(mag)) - 7)


def fwd_metrics(got: np.ndarray, ref64: np.ndarray) -> dict:
    """got: kernel output (bf16 values as float), ref64: fp64 oracle; trailing axis = head_dim."""
    got = np.asarray(got, dtype=np.float64)
    ref64 = np.asarray(ref64, dtype=np.float64)
    rb = bf16_round(ref64)
    d = np.abs(got - rb)
    rowmax = np.abs(rb).max(axis=-1, keepdims=True)
    out = {"max_abs_err": float(np.abs(got - ref64).max()), "mean_abs_err": float(np.abs(got - ref64).mean()),
           "max_abs_ref": float(np.abs(ref64).max()), "n": int(got.size),
           "frac_bit_equal": float((d == 0).mean())}
    for tag, floor in (("elem", 0.0), ("row8", 1.0 / 8), ("row", 1.0)):
        ulps = d / bf16_ulp(np.maximum(np.abs(rb), floor * rowmax))
        out[f"max_ulp_{tag}"] = float(ulps.max())
        if tag == "row8":
            out["frac_within_1ulp"] = float((ulps <= 1.0).mean())
    return out


def grad_metrics(got: np.ndarray, ref64: np.ndarray) -> dict:
    got = np.asarray(got, dtype=np.float64)
    ref64 = np.asarray(ref64, dtype=np.float64)
    scale = max(float(np.abs(ref64).max()), 1e-3)       # floor: a single-key row has dS == 0 exactly
    e = np.abs(got - ref64)
    return {"max_abs_err_over_max": float(e.max() / scale), "mean_abs_err_over_max": float(e.mean() / scale),
            "max_abs_ref": scale, "n": int(got.size)}


# Gradients PER (sequence, head) SLICE of a packed tensor (tests/test_attn_numerics_gpu.py).  The tensor-level 2^-6 gate is one ratio for the
# whole batch: a sequence or head whose gradients are 10x smaller than the largest may be 15 % wrong and pass.  A fixed per-slice ratio
# is no answer either: on a short sequence with peaked rows dS is pure cancellation and a CORRECT kernel's slice ratio reaches 0.2 - 1.7.
# So the slice gate is derived from the arithmetic: e_model = what tests/attn_model_ref.py (the flash algorithm with only the kernels'
# documented bf16 roundings) itself shows against the fp64 oracle on that slice for that input;
#   max|err_slice| <= GRAD_SLICE_MODEL_FACTOR * e_model_slice + GRAD_SLICE_ABS * max|ref_tensor|.
# The factor covers what the model leaves out (fp32 accumulation order, device exp2 vs libm); the additive term is one bf16 half-ulp of
# the tensor, for slices whose reference is exactly 0 (single-key rows).  So that the gate cannot go vacuous unnoticed, the share of slices
# on which the model itself is beyond 2^-6 of the slice (e_model_slice > GRAD_SLICE_HARD * max|ref_slice|) is capped per tensor.
GRAD_SLICE_MODEL_FACTOR = 2.0
GRAD_SLICE_ABS = 2.0 ** -9
GRAD_SLICE_HARD = 2.0 ** -6
GRAD_SLICE_MAX_HARD_SHARE = 0.25
MAX_REL_GRAD = 2.0 ** -6          # the tensor-level gate of tests/test_attn_bwd_gpu.py (_rel), named for the callers that reuse it
LSE_TOL = 1e-4                    # |lse - fp64 log-sum-exp| <= LSE_TOL * max(1, max|lse|)


def slice_absmax(x: np.ndarray, cu_seqlens) -> np.ndarray:
    """x [T, H, d] -> [n_seq, H]: max |x| over each (sequence, head) slice; NaN for an empty sequence."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    cu = [int(c) for c in cu_seqlens]
    out = np.full((len(cu) - 1, x.shape[1]), np.nan)
    for s, (a, b) in enumerate(zip(cu[:-1], cu[1:])):
        if b > a:
            out[s] = x[a:b].max(axis=(0, 2))
    return out


def grad_slice_metrics(got: np.ndarray, ref64: np.ndarray, model: np.ndarray, cu_seqlens) -> dict:
    """got: kernel gradient, ref64: fp64 oracle, model: tests/attn_model_ref.py on the same input; all [T, H, d]."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    e_got = slice_absmax(np.asarray(got, dtype=np.float64) - ref64, cu_seqlens)
    e_model = slice_absmax(np.asarray(model, dtype=np.float64) - ref64, cu_seqlens)
    r_slice = slice_absmax(ref64, cu_seqlens)
    live = ~np.isnan(r_slice)
    r_tensor = float(np.abs(ref64).max())
    gate = GRAD_SLICE_MODEL_FACTOR * e_model + GRAD_SLICE_ABS * r_tensor
    ratio = np.where(live, e_got / np.where(gate > 0, gate, 1.0), 0.0)
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    hard = live & (e_model > GRAD_SLICE_HARD * r_slice)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_model = np.where(live & (r_slice > 0), e_model / r_slice, 0.0)
        rel_got = np.where(live & (r_slice > 0), e_got / r_slice, 0.0)
    return {"max_err_over_gate": float(ratio.max()), "worst_slice": [int(worst[0]), int(worst[1])], "n_slices": int(live.sum()),
            "hard_share": float(hard.sum() / max(int(live.sum()), 1)), "max_model_err_over_slice_max": float(rel_model.max()),
            "max_err_over_slice_max": float(rel_got.max()), "max_abs_ref": r_tensor}


def check_grad_slices(case: str, got: np.ndarray, ref64: np.ndarray, model: np.ndarray, cu_seqlens) -> dict:
    m = grad_slice_metrics(got, ref64, model, cu_seqlens)
    record(case, "attn_grad_slice", m)
    assert m["hard_share"] <= GRAD_SLICE_MAX_HARD_SHARE, (case, m)     # the INPUT's fault: the model alone leaves too many slices ungated
    assert m["max_err_over_gate"] <= 1.0, (case, m)
    return m


def check_grad(case: str, got: np.ndarray, ref64: np.ndarray) -> dict:
    """The tensor-level gate of tests/test_attn_bwd_gpu.py (max |err| / max(max |ref|, 1e-3) <= 2^-6), logged like there."""
    m = grad_metrics(got, ref64)
    record(case, "attn_grad", m)
    assert m["max_abs_err_over_max"] <= MAX_REL_GRAD, (case, m)
    return m


def check_lse(case: str, got: np.ndarray, ref64: np.ndarray) -> float:
    """|err| <= LSE_TOL * max(1, max |lse|) on the rows that see a key; rows that see none are -inf on both sides."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    none = np.isneginf(ref64)
    assert np.array_equal(np.isneginf(got), none), case
    if none.all():
        return 0.0
    err = float(np.abs(got[~none] - ref64[~none]).max())
    assert err <= LSE_TOL * max(1.0, float(np.abs(ref64[~none]).max())), (case, err)
    return err


def record(case: str, kind: str, metrics: dict) -> None:
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps({"case": case, "kind": kind, **metrics}) + "\n")
    except OSError:
        pass


def check_fwd(case: str, got: np.ndarray, ref64: np.ndarray, max_ulp: float = MAX_ULP_FWD) -> dict:
    m = fwd_metrics(got, ref64)
    record(case, "attn_fwd", m)
    assert m["max_ulp_row"] <= max_ulp, (case, m)
    assert m["max_ulp_row8"] <= MAX_ULP_ROW8_FWD * max_ulp, (case, m)
    assert m["frac_within_1ulp"] >= MIN_FRAC_1ULP_ROW8 or m["n"] < 4096, (case, m)
    assert m["mean_abs_err"] <= MEAN_ABS_FWD * max(1.0, m["max_abs_ref"]), (case, m)
    return m


def lis_bf16_metrics(scores, idx_by_budget: dict, g) -> dict:
    """scores fp32 [N] and {tag: idx} of the build against one lisbf16_*.npz (the reference's bf16 run)."""
    ref = np.asarray(g["scores_bf16"], dtype=np.float64)
    scores = np.asarray(scores, dtype=np.float64)
    out = {"n": int(ref.size), "max_abs_dscore": float(np.abs(scores - ref).max()), "max_abs_ref": float(np.abs(ref).max())}
    for tag, idx in idx_by_budget.items():
        ridx = g[f"idx_bf16_{tag}"]
        sym = sorted(set(idx.tolist()) ^ set(ridx.tolist()))
        kth = np.sort(ref)[::-1][len(ridx) - 1]
        out[f"k_{tag}"] = int(len(ridx))
        out[f"symdiff_{tag}"] = len(sym)
        out[f"ties_at_kth_{tag}"] = int(g[f"ties_at_kth_{tag}"])
        out[f"symdiff_max_dist_to_kth_{tag}"] = float(max((abs(ref[i] - kth) for i in sym), default=0.0))
    return out


def check_lis_bf16(case: str, scores, idx_by_budget: dict, g) -> dict:
    m = lis_bf16_metrics(scores, idx_by_budget, g)
    record(case, "lis_bf16", m)
    scale = max(1.0, m["max_abs_ref"])
    assert m["max_abs_dscore"] <= BF16_SCORE_TOL * scale, (case, m)
    for tag in idx_by_budget:
        k = m[f"k_{tag}"]
        assert m[f"symdiff_{tag}"] <= max(2 * m[f"ties_at_kth_{tag}"], 2, int(BF16_IDX_FRAC * k)), (case, tag, m)
        # every disagreement sits at the k boundary: within the score tolerance of the reference's k-th bf16 score
        assert m[f"symdiff_max_dist_to_kth_{tag}"] <= 2 * BF16_SCORE_TOL * scale, (case, tag, m)
    return m


def bf16_bwd_metrics(got: dict, g) -> dict:
    """got: {'topk_grad' [N], 'dwq' [H,D], 'dbq' [H], 'dwk', 'dbk', 'dx' [N,D]} (any float arrays) of the build, g: one
    lisbf16_*.npz.  The dense gradients are compared through the same seeded projections the fixtures store."""
    from oracle import inputs as oin
    d, hd, n, seed = int(g["d"]), int(g["hd"]), int(g["n"]), int(g["seed"])
    u_d = oin.make_vec(d, seed + 3000).astype(np.float64)
    v_h = oin.make_vec(hd, seed + 3001).astype(np.float64)
    v_n = oin.make_vec(n, seed + 3002).astype(np.float64)
    a = {k: np.asarray(v, dtype=np.float64) for k, v in got.items()}

    def rel(x, ref):
        ref = np.asarray(ref, dtype=np.float64)
        return float(np.abs(x - ref).max() / max(np.abs(ref).max(), 1e-30))

    out = {"n": n, "topk_grad": rel(a["topk_grad"], g["topk_grad_bf16"]), "dbk": rel(a["dbk"], g["bwd_dbk"]),
           "dwq_u": rel(a["dwq"] @ u_d, g["bwd_dwq_u"]), "v_dwq": rel(v_h @ a["dwq"], g["bwd_v_dwq"]),
           "dwk_u": rel(a["dwk"] @ u_d, g["bwd_dwk_u"]), "v_dwk": rel(v_h @ a["dwk"], g["bwd_v_dwk"]),
           "dx_u": rel(a["dx"] @ u_d, g["bwd_dx_u"]), "v_dx": rel(v_n @ a["dx"], g["bwd_v_dx"]),
           # dbq is ~0 analytically (rs * kbar * sum(dscores), the soft top-k gradient sums to 0): both sides hold rounding noise
           "dbq_over_dbk": float(max(np.abs(a["dbq"]).max(), np.abs(g["bwd_dbq"]).max()) / max(np.abs(g["bwd_dbk"]).max(), 1e-30))}
    if "bwd_dwq" in getattr(g, "files", ()):
        out.update(dwq=rel(a["dwq"], g["bwd_dwq"]), dwk=rel(a["dwk"], g["bwd_dwk"]), dx=rel(a["dx"], g["bwd_dx"]))
    return out


def check_bf16_bwd(case: str, got: dict, g, kind: str = "lis_bwd_bf16") -> dict:
    m = bf16_bwd_metrics(got, g)
    record(case, kind, m)
    for key, tol in BF16_BWD_TOL.items():
        if key in m:
            assert m[key] <= tol, (case, key, m)
    return m
