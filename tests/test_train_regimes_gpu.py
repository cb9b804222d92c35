"""Value tests of the training LIS block (visionselector_amd/csrc/train.hip) on every path its host code can take, against the numpy
oracle (oracle/lis.py: train_forward / train_backward, float64 closed form) -- the golden shapes reach only some of them.

The path of a case follows from (token dtype, weight dtype, d, hd, n); expected_paths() restates the host code's choice and every case
asserts it against the kernels that actually ran (profile_start / profile_stop):
  forward   n <= 4096: train_tail_kernel<4> (n <= 1024) / <16>            | n > 4096: soft_topk_fwd, select, mask_apply<false>, bce_kernel
  scores    small form (bf16 weights, d % 16 == 0, hd % 16 == 0): proj_nt_small_kernel | else gemm_nt_kernel
  backward  fused (bf16 weights, n <= 4096, small form): outer_finish_pair_kernel (hd <= 4096) or train_bwd_finish_kernel +
            outer_pair_kernel (hd > 4096)                                 | else the ten-launch chain: soft_topk_bwd_kernel, dk_finish_kernel
  row kernels (mask_apply, rowdot, dh) launch min(ceil(n / 4), 4096) workgroups: n > 16384 makes each loop over rows.
The inputs of oracle.inputs.make_case are bf16-representable, so every storage sees the same values and one oracle evaluation per shape
serves all of them."""
import functools

import numpy as np
import pytest
import torch

import parity
import soft_topk_ref
from oracle import inputs as oin
from oracle import lis as olis

pytestmark = pytest.mark.gpu
REG_W = 0.7
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def wcolsum_words(d, n, elem_bytes):
    """launch_wcolsum, restated: 32-bit words per lane (4 / 2 / 1 = 4 / 2 / 1 "waves" of column tiles) from d, the row chunks and the
    token size."""
    e = 4 // elem_bytes
    wsplits = max(1, -(-n // 128))
    nw = 4
    while nw > 1 and (-(-d // (64 * nw * e)) * wsplits < 200 or d % (nw * e) != 0):
        nw >>= 1
    return nw


# one d for each width of launch_wcolsum at n = 300 (3 row chunks: a width needs ceil(d / (64 words elems-per-word)) >= 67 column tiles)
#   d = 34816: 4 words for both token types (bf16: 68 tiles of 512; fp32: 136 of 256)
#   d = 17408: bf16 tokens 2 words (34 tiles of 512 < 67 <= 68 of 256); fp32 tokens still 4 (68 of 256)
#   d =  8704: fp32 tokens 2 words (34 of 256 < 67 <= 68 of 128); bf16 tokens 1
#   d =  1280: 1 word for both
WCOLSUM_D = {34816: {"bf16": 4, "f32": 4}, 17408: {"bf16": 2, "f32": 4}, 8704: {"bf16": 1, "f32": 2}, 1280: {"bf16": 1, "f32": 1}}

SAME = [("f32", "f32"), ("bf16", "bf16")]
MIXED = [("bf16", "f32"), ("f32", "bf16")]                   # (tokens, weights)
SHAPES = ([(512, 256, n) for n in (3, 37, 1023, 1024, 1025, 4095, 4096, 4097, 16385, 20001)]
          + [(512, 100, 130), (512, 100, 4097)]             # bf16 weights off the small form: hd % 8 != 0
          + [(64, 4112, 130)]                                # hd > 64 x 64 inside the fused form (4104 % 16 != 0 would leave the small form)
          + [(d, 32, 300) for d in WCOLSUM_D])
CASES = [(d, hd, n, t, w) for d, hd, n in SHAPES for t, w in SAME] + [(512, 256, n, t, w) for n in (37, 4097) for t, w in MIXED]
FACTOR_NS = (37, 4097, 20001)


def expected_paths(d, hd, n, tok, wgt):
    small = wgt == "bf16" and d % 16 == 0 and hd % 16 == 0
    fused = small and n <= 4096
    return {"tail": n <= 4096, "small": small, "fused": fused, "fused_pair": fused and hd <= 64 * 64}


def test_case_table_reaches_every_path():
    paths = [expected_paths(*c) for c in CASES]
    assert {(p["tail"], p["small"]) for p in paths} == {(a, b) for a in (True, False) for b in (True, False)}
    assert any(p["fused"] and p["fused_pair"] for p in paths) and any(p["fused"] and not p["fused_pair"] for p in paths)
    assert any(w == "bf16" and not p["small"] and n <= 4096 for (d, hd, n, t, w), p in zip(CASES, paths))      # hd % 8 != 0
    assert {n for _, _, n, _, _ in CASES} >= {1024, 1025, 4096, 4097} and any(n % 4 for _, _, n, _, _ in CASES)
    assert any(n > 16384 for _, _, n, _, _ in CASES)                                                            # row kernels loop
    for d, want in WCOLSUM_D.items():
        assert {t: wcolsum_words(d, 300, 2 if t == "bf16" else 4) for t in want} == want
    assert {v for want in WCOLSUM_D.values() for t, v in want.items() if t == "bf16"} == {4, 2, 1}
    assert {v for want in WCOLSUM_D.values() for t, v in want.items() if t == "f32"} == {4, 2, 1}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from visionselector_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()                  # (a copy: the cached reference arrays are read-only)
    return t.to(dtype) if dtype is not None else t


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


@functools.lru_cache(maxsize=None)
def reference(d, hd, n):
    """The case's inputs and the oracle on them, once per shape.  k = max(1, n // 5); the upstream gradient as in
    tests/test_train_gpu.py::test_train_backward_golden, rounded to bf16 so that bf16 tokens carry the same values."""
    seed = d + hd + n
    c = oin.make_case(d, hd, n, seed)
    k = max(1, n // 5)
    budgets = (k + 0.5) / n                                   # int(n * budgets) == k  (oracle.lis.budget_k_train)
    assert olis.budget_k_train(n, budgets) == k
    gmat = olis.bf16_round(np.random.default_rng(seed + 2000).standard_normal((n, d), dtype=np.float32) / np.float32(d) ** 0.5)
    w = (c["h"], c["wq"], c["bq"], c["wk"], c["bk"])
    scores64 = olis.scorer_collapsed(c["h"][None], *w[1:])[0]
    fwd = olis.train_forward(*w, budgets)
    bwd = olis.train_backward(*w, budgets, gmat, REG_W)
    for a in list(c.values()) + [gmat]:
        a.setflags(write=False)                               # shared by every storage of the shape
    return dict(c=c, k=k, gmat=gmat, scores64=scores64, ps=fwd[1], y=fwd[2], bwd=bwd)


# Backward gate vs the float64 oracle: 3e-4 of each tensor's maximum (tests/test_train_gpu.py::test_train_backward_golden, set at
# n <= 5832).  For the two cases with n > 16384 the oracle's closed form was evaluated in float32 numpy on the CPU before any GPU run;
# its own distance from float64, relative to each tensor's maximum, was
#   n = 16385: dWq 7.4e-7, dWk 9.8e-7, dbk 9.1e-7, dx 7.2e-8        n = 20001: dWq 9.8e-7, dWk 1.0e-6, dbk 9.8e-7, dx 7.4e-8
# -- far below the 1.5e-4 at which those cases would need a gate of their own, so 3e-4 holds for every case.
BWD_GATE = 3e-4
BWD_GATE_DH_BF16 = 1e-2                                      # bf16 token gradient: tests/test_train_gpu.py::test_scores_backward_standalone


def profiled(fn):
    from visionselector_amd import _native as N
    N.profile_start()
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        names = set(N.profile_stop())
    return out, names


@pytest.mark.parametrize("d,hd,n,tok,wgt", CASES)
def test_train_block_vs_oracle(ops, d, hd, n, tok, wgt):
    r = reference(d, hd, n)
    c, k = r["c"], r["k"]
    paths = expected_paths(d, hd, n, tok, wgt)
    h = dev(c["h"], DT[tok])
    wq, bq, wk, bk = (dev(c[x], DT[wgt]) for x in ("wq", "bq", "wk", "bk"))
    case = f"lis_train_regimes[{d},{hd},{n},{tok},{wgt}]"

    # ---- forward -------------------------------------------------------------------------------------------------------------
    (h_new, ps, y, scores, ts, bce), names = profiled(lambda: ops.lis_train_fwd(h, wq, bq, wk, bk, k))
    assert ("train_tail_kernel" in names) == paths["tail"] and ("bce_kernel" in names) == (not paths["tail"]), names
    assert ("soft_topk_fwd_kernel" in names) == (not paths["tail"]) and "mask_apply_kernel" in names, names
    assert ("proj_nt_small_kernel" in names) == paths["small"] and ("gemm_nt_kernel" in names) == (not paths["small"]), names
    s_gpu, ps_gpu, y_gpu = scores.cpu().numpy(), ps.cpu().numpy(), y.cpu().numpy()
    m = {"scores": float(np.abs(s_gpu - r["scores64"]).max() / max(1.0, np.abs(r["scores64"]).max()))}
    assert m["scores"] <= 4e-6, m                              # the bound of tests/test_lis_gpu.py::test_lis_generic_shapes
    t64, ps64 = soft_topk_ref.root64(s_gpu, k)                 # each later stage against the oracle ON THE STAGE'S OWN INPUT
    m["ps_vs_root64"] = float(np.abs(ps_gpu - ps64).max())
    m["ts_vs_root64"] = abs(float(ts[0]) - float(t64))
    assert m["ps_vs_root64"] <= 1e-5 and m["ts_vs_root64"] <= 2e-5, m
    assert np.array_equal(y_gpu, olis.constraint_mask(s_gpu, k)), "constraint mask = hard top-k of the same scores"
    m["bce"] = abs(float(bce[0]) - float(olis.bce_mean(ps_gpu, y_gpu)))
    assert m["bce"] <= 1e-5, m
    if tok == "bf16":
        assert torch.equal(h_new, (ps[:, None] * h.float()).bfloat16()), "h_new = (ps * h).type(bf16) with round-to-nearest-even"
    else:
        m["h_new"] = float(np.abs(h_new.cpu().numpy() - ps_gpu[:, None] * c["h"]).max())
        assert m["h_new"] <= 1e-5, m
    if tok == "f32" and wgt == "f32":
        m["ps_end_to_end"] = float(np.abs(ps_gpu - r["ps"]).max())
        assert m["ps_end_to_end"] <= 1e-5, m
    # (the backward's oracle reads its OWN mask: where the two scores' rounding orders a near-tie at the k boundary differently, one
    # element of dps moves by ~ 0.7 / (0.16 n) -- far inside the backward gates at the n where the scores are dense enough for that)
    m["y_flips_vs_oracle"] = int((y_gpu != r["y"]).sum())

    # ---- backward: BCE fused with weight 0.7, then the same gradient handed in as d_ps_ext --------------------------------------
    gmat = dev(r["gmat"], DT[tok])
    p = ps.clone().requires_grad_(True)
    (REG_W * torch.nn.functional.binary_cross_entropy(p, y)).backward()
    ref = r["bwd"]
    for tag, ext, w in (("fused_bce", None, REG_W), ("d_ps_ext", p.grad.contiguous(), 0.0)):
        outs, names = profiled(lambda: ops.lis_train_bwd(gmat, h, wq, bq, wk, bk, ps, y, scores, ts, ext, w, need_dh=True))
        fused, pair = paths["fused"], paths["fused_pair"]
        assert ("outer_finish_pair_kernel" in names) == (fused and pair), names
        assert ("train_bwd_finish_kernel" in names) == (fused and not pair), names
        assert ("outer_pair_kernel" in names) == (not (fused and pair)), names
        assert ("soft_topk_bwd_kernel" in names) == (not fused) and ("dk_finish_kernel" in names) == (not fused), names
        assert ("proj_nt_small_pair_kernel" in names) == fused, names
        assert ("proj_nt_small_kernel" in names) == (paths["small"] and not fused), names
        assert ("gemm_nt_kernel" in names) == (not paths["small"]), names
        assert {"rowdot_kernel", "wcolsum_partial_kernel", "dh_kernel"} <= names, names
        dwq, dbq, dwk, dbk, dh = (t.double().cpu().numpy() for t in outs)
        b = {"dwq": rel(dwq, ref["dwq"]), "dwk": rel(dwk, ref["dwk"]), "dbk": rel(dbk, ref["dbk"]), "dh": rel(dh, ref["dx"]),
             "dbq_abs": float(np.abs(dbq).max())}
        print(f"{case} {tag}: fwd {m}  bwd {b}")
        parity.record(f"{case}[{tag}]", "lis_train_fp64", {**m, **b})
        assert b["dwq"] <= BWD_GATE and b["dwk"] <= BWD_GATE and b["dbk"] <= BWD_GATE, b
        assert b["dh"] <= (BWD_GATE_DH_BF16 if tok == "bf16" else BWD_GATE), b
        assert b["dbq_abs"] <= 1e-4 * max(np.abs(ref["dwq"]).max(), 1e-12) * d + 1e-6, b                  # dbq = kbar rs sum(g) ~ 0

    # ---- the rank-1-factor form rebuilds the dense gradients bit for bit ----------------------------------------------------------
    if (d, hd) == (512, 256) and n in FACTOR_NS:
        dense = ops.lis_train_bwd(gmat, h, wq, bq, wk, bk, ps, y, scores, ts, None, REG_W, need_dh=True)
        payload, dh2 = ops.lis_train_bwd_factors(gmat, h, wq, bq, wk, bk, ps, y, scores, ts, None, REG_W, need_dh=True)
        a, gx, dk, xs, dbq2, dbk2 = ops.factor_payload_split(payload, hd, d)
        assert torch.equal(torch.outer(a, gx), dense[0]) and torch.equal(torch.outer(dk, xs), dense[2])
        assert torch.equal(dbq2, dense[1]) and torch.equal(dbk2, dense[3]) and torch.equal(dh2, dense[4])
