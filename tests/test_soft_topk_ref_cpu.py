"""The fp64 helper of the soft top-k regime tests (tests/soft_topk_ref.py) against the oracle's restatement of the reference's own
lines (oracle/lis.py::find_ts, soft_topk_backward: fp32, 64 bisection steps), over the whole shared matrix, with the gates the GPU
tests then apply to the kernels: |dps| <= 1e-5, |dt| <= 2e-5, backward <= 2e-5 of the tensor's maximum.  Measured here over the
matrix: 8.0e-7, 3.5e-6, 6.8e-6 -- the reference's fp32 noise leaves 2.9x .. 12x of each gate to the kernels."""
import numpy as np
import pytest

import soft_topk_ref as ref
from oracle import inputs as oin
from oracle import lis as olis

CASES = list(ref.cases())


def test_matrix_is_the_one_the_issue_states():
    assert sorted({c[0] for c in CASES}) == sorted(ref.NS) and len(set(CASES)) == len(CASES)
    for n, k, scale, _ in CASES:
        assert 0 < k < n and min(k, n - k) >= max(1, n // 50) and scale in (0.1, 1.0)
    assert {k for n, k, _, _ in CASES if n == 2} == {1} and {k for n, k, _, _ in CASES if n == 3} == {1, 2}
    assert {k for n, k, _, _ in CASES if n == 4097} == {81, 819, 2048, 4016}


@pytest.mark.parametrize("n", ref.NS)
def test_oracle_within_the_gates_of_fp64(n):
    worst = [0.0, 0.0, 0.0]
    for n_, k, scale, seed in CASES:
        if n_ != n:
            continue
        x = (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)
        t64, ps64 = ref.root64(x, k)
        assert abs(ps64.sum() - k) <= 1e-9 * n
        ts32, ps32 = olis.find_ts(x[None], k)
        dps, dt = np.abs(ps32[0] - ps64).max(), abs(float(ts32[0, 0]) - t64)
        assert dps <= 1e-5 and dt <= 2e-5, (n, k, scale, dps, dt)
        g = oin.make_vec(n, seed + 1000)
        want = ref.bwd64(g, x, t64)
        gv = np.abs(g.astype(np.float64) * ps64 * (1.0 - ps64)).sum()
        assert abs(want.sum()) <= 1e-12 * gv, (n, k, scale, want.sum(), gv)
        got = olis.soft_topk_backward(g[None], x[None], ts32)[0]
        db = np.abs(got - want).max() / np.abs(want).max()
        assert db <= 2e-5, (n, k, scale, db)
        worst = [max(a, b) for a, b in zip(worst, (dps, dt, db))]
    print(f"n={n}: max |dps| {worst[0]:.2e}  |dt| {worst[1]:.2e}  backward / max {worst[2]:.2e}")


def _find_ts_bf16_sum64(xs, k):
    """oracle.lis.find_ts_bf16_reference with the one change that its .sum() accumulates in float64 before the bf16 rounding."""
    r = olis.bf16_round
    xs = r(np.asarray(xs, np.float32))
    lo = r(r(-xs.max(axis=1, keepdims=True)) - np.float32(10))
    hi = r(r(-xs.min(axis=1, keepdims=True)) + np.float32(10))
    for _ in range(64):
        mid = r(r(hi + lo) / np.float32(2))
        s = r(r(olis._sigmoid32(r(xs + mid))).sum(axis=1, dtype=np.float64).astype(np.float32))
        mask = s < np.float32(k)
        lo[mask] = mid[mask]
        hi[~mask] = mid[~mask]
    return r(r(lo + hi) / np.float32(2))


@pytest.mark.parametrize("n,k,seed", ref.BF16REF_CASES)
def test_bf16_reference_rows_do_not_hinge_on_the_summation_order(n, k, seed):
    x = olis.bf16_round((np.random.default_rng(seed).standard_normal((3, n)) * 0.1).astype(np.float32))
    ts, _ = olis.find_ts_bf16_reference(x, k)
    assert np.array_equal(ts, _find_ts_bf16_sum64(x, k)), (n, seed, ts.ravel())
    assert len({tuple(row) for row in x}) == 3
