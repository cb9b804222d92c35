"""numpy oracle of vsel_sample_tokens_rows ("per-row parameters"): tests/sampling_ref.py's kept set and Gumbel scores with
one row's own parameters, plus the min-p threshold on the float32 d = (x - m) * c, the greedy rule (temperature 0) and the drawn token's
log-probability in float64.  Imported by tests/test_sample_rows_*.py and tests/test_generate_rows_gpu.py."""
import math

import numpy as np

from sampling_ref import LOG2E, gumbel_scores, kept_set, keys, masses, uniforms  # noqa: F401  (re-exported for the tests)


def d_values(x, temperature: float) -> np.ndarray:
    """float32 d = (x - m) * float32(log2e / T), the exponent sampling_ref.masses takes the mass from (-inf entries -> -inf)"""
    x = np.asarray(x, dtype=np.float32)
    c = np.float32(LOG2E / float(np.float32(temperature)))
    fin = np.isfinite(x)
    m = x[fin].max()
    with np.errstate(invalid="ignore"):
        return np.where(fin, (x - m).astype(np.float32) * c, np.float32(-np.inf)).astype(np.float32)


def min_p_threshold(min_p: float) -> np.float32:
    """lmin = float32(log2(float64(float32(min_p)))); min_p 0 -> -inf (off)"""
    with np.errstate(divide="ignore"):
        return np.float32(np.log2(np.float64(np.float32(min_p))))


def valid_row(x) -> bool:
    x = np.asarray(x, dtype=np.float32)
    return not (np.isnan(x).any() or np.isposinf(x).any() or not np.isfinite(x).any())


def valid_parameters(temperature, top_p, top_k, min_p) -> bool:
    t, p, mp = np.float32(temperature), np.float32(top_p), np.float32(min_p)
    if not (np.isfinite(t) and t >= 0):
        return False
    if t == 0:
        return True                                                # a greedy row's other parameters are ignored
    return bool(0 < p <= 1 and top_k >= 0 and 0 <= mp <= 1)


def final_set(x, temperature: float, top_p: float = 1.0, top_k: int = 0, min_p: float = 0.0):
    """-> (kept bool [V] = top-k & top-p & min-p, info of sampling_ref.kept_set); kept None for an invalid row.  Z and the top-p target
    are taken before min-p (HF applies MinPLogitsWarper after the other two)."""
    kept, info = kept_set(x, temperature, top_p, top_k)
    if kept is None:
        return None, info
    return kept & (d_values(x, temperature) >= min_p_threshold(min_p)), info


def logprob(x, temperature: float, kept: np.ndarray, token: int, d=None) -> float:
    """float64 d_t ln2 - log(sum over kept of exp2(d)) from the float32 d (or from a given d, for checks of the formula itself)"""
    d = (d_values(x, temperature) if d is None else np.asarray(d)).astype(np.float64)
    return float(d[token] * math.log(2.0) - np.log(np.exp2(d[kept]).sum()))


def sample_row(x, temperature=1.0, top_p=1.0, top_k=0, min_p=0.0, seed=0, row_id=0, step=0):
    """One row of vsel_sample_tokens_rows -> dict(token, kept (count), mask, scores, info, logprob, greedy).  token -1, kept 0, logprob
    NaN for an invalid row or out-of-range parameters."""
    x = np.asarray(x, dtype=np.float32)
    bad = dict(token=-1, kept=0, mask=None, scores=None, info={}, logprob=float("nan"), greedy=False)
    if not valid_parameters(temperature, top_p, top_k, min_p) or not valid_row(x):
        return bad
    if np.float32(temperature) == 0:
        fin = np.isfinite(x)
        tok = int(np.argmax(np.where(fin, x, -np.inf)))            # lowest index among equal values, +0 == -0
        return dict(token=tok, kept=1, mask=None, scores=None, info={}, logprob=logprob(x, 1.0, fin, tok), greedy=True)
    mask, info = final_set(x, temperature, top_p, top_k, min_p)
    s = gumbel_scores(x, temperature, seed, row_id, step, mask)
    tok = int(np.argmax(s))
    return dict(token=tok, kept=int(mask.sum()), mask=mask, scores=s, info=info, logprob=logprob(x, temperature, mask, tok), greedy=False)
