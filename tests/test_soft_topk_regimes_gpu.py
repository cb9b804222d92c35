"""Value tests of the differentiable top-k kernels (visionselector_amd/csrc/softtopk.hip, softtopk.h) in every size regime, against the
float64 oracle of tests/soft_topk_ref.py (pinned to the reference's own lines by tests/test_soft_topk_ref_cpu.py).

Which n of the shared matrix reaches which form of the forward (launch_soft_topk_fwd, soft_topk_row_256x16; one kernel name for all):
  256 threads x  4 registers   n = 2, 3, 64, 255, 256, 257, 1024      (1024: every register full, no -inf padding)
  256 threads x  8 registers   n = 1025, 2048
  256 threads x 12 registers   n = 2049, 3072
  256 threads x 16 registers   n = 3073, 4096                         (4096: full)
  1024 threads x 16 registers  n = 4097, 16384                        (16384: full)
  row re-read from global      n = 16385, 40000                       (its own 48-step loop, no fast-sigmoid stage)
The backward switches from 256 to 1024 threads at n = 4096 / 4097."""
import numpy as np
import pytest
import torch

import parity
import soft_topk_ref as ref
from oracle import inputs as oin
from oracle import lis as olis

pytestmark = pytest.mark.gpu
CASES = list(ref.cases())
FORM_OF_N = {2: "256x4", 3: "256x4", 64: "256x4", 255: "256x4", 256: "256x4", 257: "256x4", 1024: "256x4", 1025: "256x8", 2048: "256x8",
             2049: "256x12", 3072: "256x12", 3073: "256x16", 4096: "256x16", 4097: "1024x16", 16384: "1024x16", 16385: "global",
             40000: "global"}


def fwd_form(n):
    """launch_soft_topk_fwd + soft_topk_row_256x16, restated."""
    if n <= 4096:
        return "256x%d" % (4 if n <= 1024 else 8 if n <= 2048 else 12 if n <= 3072 else 16)
    return "1024x16" if n <= 16384 else "global"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from visionselector_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def row(n, scale, seed):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def profiled(fn):
    """fn() between profile_start / profile_stop -> (result, {kernel name: launches})."""
    from visionselector_amd import _native as N
    N.profile_start()
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        names = N.profile_stop()
    return out, {k: v[1] for k, v in names.items()}


def test_matrix_covers_every_forward_form():
    assert set(FORM_OF_N) == set(ref.NS) and all(fwd_form(n) == f for n, f in FORM_OF_N.items())
    assert set(FORM_OF_N.values()) == {"256x4", "256x8", "256x12", "256x16", "1024x16", "global"}
    for full in (1024, 2048, 3072, 4096, 16384):                  # both sides of every switch
        assert fwd_form(full) != fwd_form(full + 1) and full in FORM_OF_N and full + 1 in FORM_OF_N


@pytest.mark.parametrize("n", ref.NS)
def test_forward_every_regime_vs_fp64(ops, n):
    """Every case of the matrix: the (scale) rows that share a k are the rows of one [B, n] call (distinct rows: row indexing counts).
    Gates (tests/test_soft_topk_ref_cpu.py: the reference's own fp32 lines sit 2.9x .. 12x inside them): |ps - ps64| <= 1e-5,
    |t - t64| <= 2e-5; and |sum ps - k| <= max(2e-2, 3e-5 n) as in tests/test_property_gpu.py."""
    worst = {"max_abs_dps": 0.0, "max_abs_dt": 0.0, "max_abs_sum_minus_k": 0.0}
    for k in sorted({c[1] for c in CASES if c[0] == n}):
        rows = [c for c in CASES if c[0] == n and c[1] == k]
        assert len(rows) == len(ref.SCALES)
        x = np.stack([row(n, scale, seed) for _, _, scale, seed in rows])
        (ps, ts), launched = profiled(lambda: ops.soft_topk_fwd(dev(x), k))
        assert launched == {"soft_topk_fwd_kernel": 1}, launched
        ps, ts = ps.cpu().numpy(), ts.cpu().numpy()
        assert ps.shape == x.shape and ts.shape == (len(rows),)
        t64, ps64 = ref.root64(x, k)
        m = {"max_abs_dps": float(np.abs(ps - ps64).max()), "max_abs_dt": float(np.abs(ts - t64).max()),
             "max_abs_sum_minus_k": float(np.abs(ps.sum(axis=1, dtype=np.float64) - k).max())}
        print(f"soft_topk_fwd n={n} k={k} form={FORM_OF_N[n]}: {m}")
        worst = {key: max(worst[key], m[key]) for key in worst}
        assert m["max_abs_dps"] <= 1e-5 and m["max_abs_dt"] <= 2e-5, (n, k, m)
        assert m["max_abs_sum_minus_k"] <= max(2e-2, 3e-5 * n), (n, k, m)
    parity.record(f"soft_topk_fwd_regimes[n={n},{FORM_OF_N[n]}]", "soft_topk_fp64", worst)


def hard_rows(n, rng):
    """The five rows of tests/test_train_gpu.py::test_soft_topk_saturated_and_wide_spread_scores_converge (n = 2304, clusters of 300 and
    460) at n, the cluster sizes scaled in proportion.  -> (rows float32 [5, n], c1, c2)"""
    c1, c2 = round(300 * n / 2304), round(460 * n / 2304)
    rows = [np.concatenate((np.full(c1, 30.0), np.full(n - c1, -30.0))) + 0.01 * rng.standard_normal(n),      # two saturated clusters
            rng.uniform(-200, 200, n)]                                                                      # wide spread
    b = 0.05 * rng.standard_normal(n)
    b[7] = 500.0                                                                                            # one huge outlier
    rows.append(b)
    rows.append(np.full(n, 0.25))                                                                           # constant row
    rows.append(np.concatenate((np.full(c2, 80.0), np.full(n - c2, -80.0))))                                # k exactly at the cluster edge
    return np.stack(rows).astype(np.float32), c1, c2


@pytest.mark.parametrize("n", [16384, 20000])
def test_forward_hard_rows_in_the_large_forms(ops, n):
    """Rows on which a Newton step is useless far from the root, in the two forms no test reached: 1024 threads x 16 registers with
    every register full (n = 16384) and the global re-read loop (n = 20000: no fast-sigmoid stage, 48-step cap, a bracket of its own).
    Same assertions as the n = 2304 test: finite, |sum ps - k| <= 5e-3 max(1, k / 460), |ps - find_ts| <= 2e-4."""
    assert fwd_form(n) == {16384: "1024x16", 20000: "global"}[n]
    xs, c1, c2 = hard_rows(n, np.random.default_rng(11))
    worst = {"max_abs_dps_vs_find_ts": 0.0, "max_sum_err_over_bound": 0.0}
    for k in (1, c1, c1 + 1, c2, c2 + 1, n // 2, n - 1):
        ps, ts = ops.soft_topk_fwd(dev(xs), k)
        ps = ps.cpu().numpy()
        assert np.isfinite(ps).all() and np.isfinite(ts.cpu().numpy()).all()
        bound = 5e-3 * max(1.0, k / 460)
        serr = float(np.abs(ps.sum(axis=1, dtype=np.float64) - k).max())
        _, ps_ref = olis.find_ts(xs, k)
        # (a plateau of f -- the cluster-edge rows -- leaves t undetermined over an interval: compare ps, not t)
        dps = float(np.abs(ps - ps_ref).max())
        print(f"soft_topk_fwd hard rows n={n} k={k}: |sum - k| {serr:.3e} (bound {bound:.3e})  |ps - find_ts| {dps:.3e}")
        worst = {"max_abs_dps_vs_find_ts": max(worst["max_abs_dps_vs_find_ts"], dps),
                 "max_sum_err_over_bound": max(worst["max_sum_err_over_bound"], serr / bound)}
        assert serr <= bound, (k, ps.sum(axis=1, dtype=np.float64))
        assert dps <= 2e-4, (k, dps)
    parity.record(f"soft_topk_fwd_hard_rows[n={n}]", "soft_topk_hard", worst)


@pytest.mark.parametrize("n", ref.NS)
def test_backward_batched_vs_fp64(ops, n):
    """soft_topk_bwd_kernel with B = 4 distinct rows and a ts per row (the kernel's own forward ts), against the float64 closed form at
    that same ts (so the root's error is not in the comparison): <= 2e-5 of each row's maximum; the gradient sums to zero
    (|sum| <= 1e-5 sum |g v|); each row of the batch equals that row run alone, bit for bit."""
    rows = [c for c in CASES if c[0] == n]
    rows = rows[::2][:4] if len(rows) >= 8 else rows[:4]         # two k of each scale
    while len(rows) < 4:                                         # n = 2 has two (k, scale) cases: two more seeds of the first
        rows.append((n, rows[0][1], 0.5, 900 + len(rows)))
    x = np.stack([row(n, scale, seed) for _, _, scale, seed in rows])
    g = np.stack([oin.make_vec(n, seed + 1000) for _, _, _, seed in rows])
    xd, gd = dev(x), dev(g)
    ts = torch.cat([ops.soft_topk_fwd(xd[i:i + 1], rows[i][1])[1] for i in range(4)])        # a k, hence a ts, per row
    assert len(set(ts.cpu().tolist())) == 4
    grad, launched = profiled(lambda: ops.soft_topk_bwd(gd, xd, ts))
    assert launched == {"soft_topk_bwd_kernel": 1}, launched
    for i in range(4):
        assert torch.equal(grad[i:i + 1], ops.soft_topk_bwd(gd[i:i + 1].contiguous(), xd[i:i + 1].contiguous(), ts[i:i + 1].contiguous())), i
    got = grad.double().cpu().numpy()
    t = ts.double().cpu().numpy()
    want = ref.bwd64(g, x, t)
    p = 1.0 / (1.0 + np.exp(-(x.astype(np.float64) + t[:, None])))
    gv = np.abs(g * p * (1.0 - p)).sum(axis=1)
    m = {"max_err_over_rowmax": float((np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)).max()),
         "max_abs_sum_over_sum_abs_gv": float((np.abs(got.sum(axis=1)) / gv).max())}
    print(f"soft_topk_bwd n={n} threads={256 if n <= 4096 else 1024}: {m}")
    parity.record(f"soft_topk_bwd_regimes[n={n}]", "soft_topk_fp64", m)
    assert m["max_err_over_rowmax"] <= 2e-5, m
    assert m["max_abs_sum_over_sum_abs_gv"] <= 1e-5, m


@pytest.mark.parametrize("n,k,seed", ref.BF16REF_CASES)
def test_bf16_reference_mode_batched(ops, n, k, seed):
    """vsel_soft_topk_fwd_bf16ref on B = 3 distinct rows of bf16 scores ~ N(0, 0.1^2): each row of the batch equals its own single-row
    call bit for bit; ts is oracle.lis.find_ts_bf16_reference's or the bf16 value next to it; ps differs on at most 2 elements per row
    by at most one bf16 step (the allowance of tests/test_lis_gpu.py::test_lis_select_vs_reference_bf16_run: libm vs device expf at a
    bf16 rounding boundary) when ts agrees.  The rows' oracle ts does not depend on the accumulation order of the bf16 sum
    (tests/test_soft_topk_ref_cpu.py)."""
    x = olis.bf16_round((np.random.default_rng(seed).standard_normal((3, n)) * 0.1).astype(np.float32))
    xd = dev(x)
    (ps, ts), launched = profiled(lambda: ops.soft_topk_fwd(xd, k, bf16_reference=True))
    assert launched == {"soft_topk_fwd_bf16ref_kernel": 1}, launched
    for i in range(3):
        p1, t1 = ops.soft_topk_fwd(xd[i:i + 1].contiguous(), k, bf16_reference=True)
        assert torch.equal(p1, ps[i:i + 1]) and torch.equal(t1, ts[i:i + 1]), i
    ts_ref, ps_ref = olis.find_ts_bf16_reference(x, k)
    ps, ts = ps.cpu().numpy(), ts.cpu().numpy()
    assert np.array_equal(olis.bf16_round(ps), ps) and np.array_equal(olis.bf16_round(ts), ts)       # bf16 values
    m = {"ts_steps": [], "ps_diff_elems": [], "ps_max_diff": 0.0}
    for i in range(3):
        step = float(parity.bf16_ulp(abs(float(ts_ref[i, 0]))))
        m["ts_steps"].append(abs(float(ts[i]) - float(ts_ref[i, 0])) / step)
        assert abs(float(ts[i]) - float(ts_ref[i, 0])) <= step, (i, ts[i], ts_ref[i, 0])
        # ps against the oracle's lines evaluated at the ts the kernel returned (identical to ps_ref when ts agrees)
        want = ps_ref[i] if ts[i] == ts_ref[i, 0] else olis.bf16_round(olis._sigmoid32(olis.bf16_round(x[i] + ts[i])))
        bad = np.flatnonzero(ps[i] != want)
        m["ps_diff_elems"].append(int(len(bad)))
        if len(bad):
            m["ps_max_diff"] = max(m["ps_max_diff"], float(np.abs(ps[i][bad] - want[bad]).max()))
        assert len(bad) <= 2 and (len(bad) == 0 or np.abs(ps[i][bad] - want[bad]).max() <= 2.0 ** -8), (i, len(bad))
    print(f"soft_topk_fwd_bf16ref n={n}: {m}")
    parity.record(f"soft_topk_bf16ref_regimes[n={n}]", "soft_bf16", m)
