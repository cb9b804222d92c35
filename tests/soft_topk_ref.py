"""numpy fp64 oracle of the differentiable top-k (reference: FT/compression_method/selector_model.py:53-88, restated in fp32 by
oracle/lis.py::find_ts / soft_topk_backward) and the matrix of cases the CPU and GPU tests of its size regimes share.  Nothing here
imports the package."""
import numpy as np

# every n at which visionselector_amd/csrc/softtopk.hip / softtopk.h / train.hip change form, both sides of each switch:
#   256 threads x 4 / 8 / 12 / 16 registers (switches at 1024, 2048, 3072), 1024 threads x 16 registers (4097 .. 16384), the row
#   re-read from global memory (> 16384); 2 / 3 / 64 / 255 .. 257: less than one element per thread, one wave, one full pass
NS = (2, 3, 64, 255, 256, 257, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 16384, 16385, 40000)
SCALES = (0.1, 1.0)


def _sigmoid64(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def root64(x, k):
    """x [n] or [B, n] -> (t [] or [B], ps like x), float64: the root of sum_i sigmoid(x_i + t) = k by 200 bisection steps of the
    reference's own bracket [-max - 10, -min + 10] (:78-79) -- far past float64 resolution, so t is the root and ps = sigmoid(x + t)."""
    x = np.asarray(x, np.float64)
    lo = -x.max(axis=-1) - 10.0
    hi = -x.min(axis=-1) + 10.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        below = _sigmoid64(x + mid[..., None]).sum(axis=-1) < k
        lo = np.where(below, mid, lo)
        hi = np.where(below, hi, mid)
    t = 0.5 * (lo + hi)
    return t, _sigmoid64(x + t[..., None])


def bwd64(g, x, t):
    """TopK.backward (:60-70) in float64 at the given t: g v - (sum g v) v / sum v with v = p (1 - p), p = sigmoid(x + t).
    g, x [n] or [B, n]; t scalar or [B]."""
    g = np.asarray(g, np.float64)
    p = _sigmoid64(np.asarray(x, np.float64) + np.asarray(t, np.float64)[..., None])
    v = p * (1.0 - p)
    gv = g * v
    return gv - gv.sum(axis=-1, keepdims=True) * v / v.sum(axis=-1, keepdims=True)


def cases():
    """-> (n, k, scale, seed) over NS x SCALES x the k below.  The row of a case is
    (numpy.random.default_rng(seed).standard_normal(n) * scale).astype(float32).
    k: max(2, n // 50) (1 for n < 50), n // 5, n // 2, n - max(1, n // 50), kept when 0 < k < n.  So min(k, n - k) >= max(1, n // 50)
    and the spread is at most a few sigmoid widths: sum sigmoid(x + t) has a slope of order min(k, n - k) at the root and every
    case is well conditioned in fp32 -- none needs a looser gate."""
    for n in NS:
        ks = sorted({k for k in (1 if n < 50 else max(2, n // 50), n // 5, n // 2, n - max(1, n // 50)) if 0 < k < n})
        for si, scale in enumerate(SCALES):
            for k in ks:
                yield n, k, scale, 100003 * si + 7 * n + k


# bf16-reference mode (vsel_soft_topk_fwd_bf16ref): (n, k, seed); the rows are
# oracle.lis.bf16_round(numpy.random.default_rng(seed).standard_normal((3, n)) * 0.1).  tests/test_soft_topk_ref_cpu.py holds every
# seed to the condition that makes the comparison meaningful: the oracle's ts is the same whether its bf16 sum is accumulated in
# float32 or in float64, i.e. no bisection step of these rows is decided by the accumulation order.
BF16REF_CASES = ((40, 8, 1), (1023, 204, 2), (1025, 205, 3), (5000, 1000, 4), (20000, 4000, 5))
