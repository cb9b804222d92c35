"""numpy fp64 oracle of the fused LM cross-entropy (include/vsel.h, vsel_token_logprob_fwd / _bwd) on the inputs as
stored, plus the error measures the tests share.  Nothing here imports the package."""
import numpy as np

TINY = 2.0 ** -126


def as_f64(x):
    """torch tensor (bf16 / fp32 / fp64, any device) or array -> float64 ndarray, exact."""
    if hasattr(x, "detach"):
        x = x.detach().double().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def lse_logprob(x, targets, ignore_index=-100):
    """x [rows, V], targets int [rows] -> (lse, logprob) float64 [rows].  Ignored row: 0, 0.  Target outside [0, V): NaN, NaN.
    Row with a NaN, a +inf or no finite entry: NaN, NaN.  -inf entries are legal; a target on -inf gives -inf."""
    x = as_f64(x)
    t = np.asarray(targets, dtype=np.int64)
    rows, v = x.shape
    lse = np.zeros(rows)
    lp = np.zeros(rows)
    for r in range(rows):
        if t[r] == ignore_index:
            continue
        row = x[r]
        if t[r] < 0 or t[r] >= v or np.isnan(row).any() or np.isposinf(row).any() or not np.isfinite(row).any():
            lse[r] = lp[r] = np.nan
            continue
        m = row.max()
        with np.errstate(divide="ignore"):
            lse[r] = m + np.log(np.exp(row - m).sum())
        lp[r] = row[t[r]] - lse[r]
    return lse, lp


def grad(x, targets, c, ignore_index=-100, lse=None):
    """d/dx of sum_r c_r logprob_r: c_r ([j == t] - exp(x_j - lse_r)), float64 [rows, V]; zeros for ignored rows and for rows whose
    target is outside [0, V).  lse: the per-row value the backward is given (as stored); default: this oracle's own."""
    x = as_f64(x)
    t = np.asarray(targets, dtype=np.int64)
    rows, v = x.shape
    c = np.broadcast_to(as_f64(c), (rows,))
    if lse is None:
        lse = lse_logprob(x, t, ignore_index)[0]
    lse = as_f64(lse)
    g = np.zeros((rows, v))
    for r in range(rows):
        if t[r] == ignore_index or t[r] < 0 or t[r] >= v:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            p = np.exp(x[r] - lse[r])
            onehot = np.zeros(v)
            onehot[t[r]] = 1.0
            g[r] = c[r] * (onehot - p)
    return g


def hf_shift(labels, ignore_index=-100):
    """ForCausalLMLoss's label shift: [..., L] -> flat [prod * L]; position n holds label n + 1, the last one ignore_index."""
    lab = np.asarray(labels, dtype=np.int64)
    out = np.full(lab.shape, ignore_index, dtype=np.int64)
    out[..., :-1] = lab[..., 1:]
    return out.reshape(-1)


def fixed_order_sum(logprob_f32):
    """The order include/vsel.h documents for sum_out: 1024 strided fp64 partials (k ascending), folded in halves; one fp32 rounding."""
    lp = np.asarray(logprob_f32, dtype=np.float32).astype(np.float64)
    p = np.zeros(1024)
    for k in range(0, len(lp), 1024):
        chunk = lp[k:k + 1024]
        p[:len(chunk)] = p[:len(chunk)] + chunk
    h = 512
    while h:
        p[:h] = p[:h] + p[h:2 * h]
        h //= 2
    return np.float32(p[0])


def mant_bits(dtype_name):
    return {"bf16": 8, "f32": 24}[dtype_name]


def ulp(v, dtype_name):
    """spacing of the format at |v| (normal range; below 2^-126 the spacing at 2^-126)"""
    a = np.maximum(np.abs(as_f64(v)), TINY)
    return 2.0 ** (np.floor(np.log2(a)) - (mant_bits(dtype_name) - 1))


def round_to(v, dtype_name):
    """fp64 -> the format, round to nearest even, ONE rounding (normal range; inf / NaN pass through)"""
    v = as_f64(v)
    if dtype_name == "f32":
        with np.errstate(over="ignore"):
            return v.astype(np.float32).astype(np.float64)
    out = v.copy()
    fin = np.isfinite(v)
    m, e = np.frexp(v[fin])
    out[fin] = np.ldexp(np.round(m * 256.0), e - 8)
    return out


def grad_gate(got, want64, dtype_name):
    """Backward gate: every element of `got` within one ulp of the format (at the oracle value's magnitude) of the oracle rounded once
    to the format; magnitudes below 2^-126 exempt on both sides; NaN exactly where the oracle has NaN.  -> (ok, worst error in ulps)."""
    got = as_f64(got)
    want64 = as_f64(want64)
    if not np.array_equal(np.isnan(got), np.isnan(want64)):
        return False, np.inf
    fin = ~np.isnan(want64)
    g, w = got[fin], want64[fin]
    with np.errstate(invalid="ignore"):
        err = np.abs(g - round_to(w, dtype_name)) / ulp(w, dtype_name)
        err = np.where(g == round_to(w, dtype_name), 0.0, err)           # equal infinities
    exempt = (np.abs(g) < TINY) & (np.abs(w) < TINY)
    err = np.where(exempt, 0.0, err)
    worst = float(err.max()) if err.size else 0.0
    return bool(worst <= 1.0), worst
