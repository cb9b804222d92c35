"""numpy oracle of vsel_sample_tokens: Philox4x32-10, the kept set by the fixed-point mass rules, the Gumbel scores
in float64.  Imported by tests/test_sample_*.py."""
import numpy as np

M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
LOG2E = 1.4426950408889634
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr uint32 [..., 4], key uint32 [..., 2] (broadcast) -> uint32 [..., 4]"""
    c = [np.asarray(ctr, dtype=np.uint32)[..., j].astype(np.uint64) for j in range(4)]
    k0 = np.asarray(key, dtype=np.uint32)[..., 0].copy()
    k1 = np.asarray(key, dtype=np.uint32)[..., 1].copy()
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0, p1 = M0 * c[0], M1 * c[2]
            c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0.astype(np.uint64), p1 & MASK32,
                 (p0 >> np.uint64(32)) ^ c[3] ^ k1.astype(np.uint64), p0 & MASK32]
            k0 = k0 + W0
            k1 = k1 + W1
    return np.stack([x.astype(np.uint32) for x in c], axis=-1)


def uniforms(vocab: int, seed: int, row_id: int, step: int):
    """u_i for i in [0, vocab) in float64, exactly ((word >> 8) + 0.5) * 2^-24"""
    blocks = np.arange((vocab + 3) // 4, dtype=np.uint64)
    ctr = np.zeros((blocks.size, 4), dtype=np.uint32)
    ctr[:, 0] = blocks.astype(np.uint32)
    ctr[:, 1] = np.uint32(row_id & 0xFFFFFFFF)
    ctr[:, 2] = np.uint32(step & 0xFFFFFFFF)
    ctr[:, 3] = np.uint32((step >> 32) & 0xFFFFFFFF)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    words = philox4x32_10(ctr, key).reshape(-1)[:vocab]
    return ((words >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def keys(x32: np.ndarray) -> np.ndarray:
    """order-preserving uint64 keys of float32 values (-0 folded onto +0); bf16 values, widened to float32, order the same way"""
    b = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = np.where(b == 0x80000000, 0, b)
    return np.where(b & 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000)


def masses(x32: np.ndarray, temperature: float) -> np.ndarray:
    """uint64 fixed-point masses floor(exp2((x - m) * float32(log2e / T)) * 2^40) in float32 arithmetic (finite entries; -inf -> 0)"""
    t32 = float(np.float32(temperature))
    c = np.float32(LOG2E / t32)
    fin = np.isfinite(x32)
    m = x32[fin].max()
    d = np.where(fin, (x32 - m).astype(np.float32) * c, np.float32(-np.inf)).astype(np.float32)
    return np.floor(np.exp2(d).astype(np.float32).astype(np.float64) * 2.0 ** 40).astype(np.uint64)


def kept_set(x, temperature: float, top_p: float = 1.0, top_k: int = 0):
    """x float32 [V] (bf16 rows widened) -> (kept bool [V], info) by DESIGN.md §13; kept is None for an invalid row.
    info: Z, the top-p target and the distance of the target from the nearest cumulative-mass step (in mass units)."""
    x = np.asarray(x, dtype=np.float32)
    if np.isnan(x).any() or np.isposinf(x).any() or not np.isfinite(x).any():
        return None, {}
    fin = np.isfinite(x)
    k = keys(x)
    w = masses(x, temperature)
    nfin = int(fin.sum())
    kf = np.sort(k[fin])[::-1]
    tau_k = kf[top_k - 1] if 0 < top_k < nfin else np.uint64(0)
    in_k = fin & (k >= tau_k)
    z = int(w[in_k].sum(dtype=np.uint64))                 # < V * 2^40: no wrap for V < 2^24
    info = {"Z": z, "margin": float("inf")}
    tau = tau_k
    p32 = float(np.float32(top_p))
    if p32 < 1.0:
        target = min(z, max(1, int(np.ceil(np.float64(p32) * np.float64(z)))))
        # distinct keys descending, with the cumulative mass at or above each
        uk, inv = np.unique(k[in_k], return_inverse=True)
        mass_per = np.zeros(uk.size, dtype=np.uint64)
        np.add.at(mass_per, inv, w[in_k])
        order = np.arange(uk.size)[::-1]
        cum = np.cumsum(mass_per[order])
        j = int(np.argmax(cum >= target))
        tau = uk[order][j]
        steps = np.concatenate(([0.0], cum.astype(np.float64)))
        info["margin"] = float(np.abs(steps - target).min())
        info["target"] = target
    return fin & (k >= tau), info


def gumbel_scores(x, temperature: float, seed: int, row_id: int, step: int, kept: np.ndarray):
    """float64 (x - m) / T - log(-log u) on the kept entries, -inf elsewhere"""
    x = np.asarray(x, dtype=np.float32)
    t32 = float(np.float32(temperature))
    m = float(x[np.isfinite(x)].max())
    u = uniforms(x.size, seed, row_id, step)
    s = (x.astype(np.float64) - m) / t32 - np.log(-np.log(u))
    return np.where(kept, s, -np.inf)


def sample(x, temperature: float, top_p: float = 1.0, top_k: int = 0, seed: int = 0, row_id: int = 0, step: int = 0):
    """-> (token, kept count, scores, info); token -1 for an invalid row"""
    kept, info = kept_set(x, temperature, top_p, top_k)
    if kept is None:
        return -1, 0, None, info
    s = gumbel_scores(x, temperature, seed, row_id, step, kept)
    return int(np.argmax(s)), int(kept.sum()), s, info
