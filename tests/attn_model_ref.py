"""Error model of the attention kernels (plain numpy, fp64; TEST INFRASTRUCTURE ONLY) and the input families of the numerics tests.

NOT a second oracle.  oracle/attention.py says what attention IS; this file says how far a CORRECT kernel may sit from it for a given
input.  It is the flash algorithm with only the rounding points the kernels document (csrc/attn.hip, csrc/attn_bwd.hip) and everything
else exact:

  forward    S = scale Q K^T exact; un-normalised P = exp(S - r) ROUNDED TO bf16 before P V, r = the forward's lazy reference exponent of
             the key's 64-key tile (kLazyTau: it decides WHICH bf16 grid P is rounded on); the row sum l taken over the un-rounded P;
             O = (P_bf16 V) / l STORED AS bf16; lse = rowmax + log l exact.
  backward   P = exp(S - lse) exact; D = rowsum(dO * O_bf16) with the forward's stored output; dP = dO V^T exact;
             dS = P (dP - D); P and dS ROUNDED TO bf16 before the second contractions (dV = P^T dO, dQ = scale dS K, dK = scale dS^T Q,
             the scale applied to the fp32 sums); a kv head's group summed un-rounded; dQ / dK / dV STORED AS bf16.

Left out on purpose: the order of the fp32 accumulations, the device's exp2 against libm, and the tilings of the forms that do not walk
64-key tiles from key 0 in one stream (two KV streams, key-range parts).  The gates built on this model carry a factor 2 for those
(tests/parity.py, check_grad_slices).  The lazy reference exponent is NOT left out: on peaked rows dS = P (dP - D) cancels against
D = rowsum(dO * O_bf16), so a slice's gradient error follows which way each O element was rounded, i.e. the grid P was rounded on.

Second half: FAMILIES / make_inputs -- the seeded inputs shared by tests/test_attn_model_cpu.py (which proves on the CPU that each family
leaves this model inside every gate the GPU tests apply) and tests/test_attn_numerics_gpu.py.
"""
from __future__ import annotations

import math

import numpy as np

from parity import bf16_round


def _scores(qh, kh, scale, causal, shift=0):
    w = (qh @ kh.T) * scale
    if causal:
        nq, nk = w.shape
        w = np.where(np.arange(nk)[None, :] <= np.arange(nq)[:, None] + shift, w, -np.inf)
    return w


TILE_K = 64                     # csrc/attn_common.h kTileK: keys per K / V tile, tiles counted from key 0
LAZY_TAU = 8.0 * math.log(2.0)  # csrc/attn_common.h kLazyTau (8 log2 units), in natural-log units


def _lazy_reference(w):
    """Reference exponent each un-normalised P is ROUNDED in, [nq, nk]: the forward keeps a row's exponent until a 64-key tile's maximum
    exceeds it by more than kLazyTau (csrc/attn.hip), so p = exp(w - r) may exceed 1 and the bf16 grid it is rounded on is the tile's,
    not the row maximum's.  The first tile with a visible key sets it to that tile's maximum (a row of <= 64 keys: the row maximum)."""
    nq, nk = w.shape
    r = np.empty_like(w)
    run = np.full(nq, -np.inf)
    for t0 in range(0, nk, TILE_K):
        mx = w[:, t0:t0 + TILE_K].max(axis=1)
        run = np.where(np.maximum(run, mx) > run + LAZY_TAU, np.maximum(run, mx), run)
        r[:, t0:t0 + TILE_K] = np.where(np.isfinite(run), run, 0.0)[:, None]
    return r


def lse_reference(q, k, cu_seqlens, causal=True, softmax_scale=None):
    """fp64 log-sum-exp of the scaled scores over the visible keys, [T, Hq] (natural log); a row without a visible key -> -inf."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    t, hq, d = q.shape
    rep = hq // k.shape[1]
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(d)
    lse = np.full((t, hq), -np.inf)
    cu = [int(c) for c in cu_seqlens]
    for a, b in zip(cu[:-1], cu[1:]):
        for h in range(hq if b > a else 0):
            w = _scores(q[a:b, h], k[a:b, h // rep], scale, causal)
            m = w.max(axis=1)
            lse[a:b, h] = m + np.log(np.exp(w - m[:, None]).sum(axis=1))
    return lse


def varlen_attention_model(q, k, v, cu_seqlens, causal=True, softmax_scale=None):
    """-> (out [T, Hq, d]: bf16 values in fp64, lse [T, Hq] fp64); arguments as oracle.attention.varlen_attention."""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    t, hq, d = q.shape
    rep = hq // k.shape[1]
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(d)
    out = np.zeros_like(q)
    lse = np.full((t, hq), -np.inf)
    cu = [int(c) for c in cu_seqlens]
    for a, b in zip(cu[:-1], cu[1:]):
        for h in range(hq if b > a else 0):
            w = _scores(q[a:b, h], k[a:b, h // rep], scale, causal)
            m = w.max(axis=1, keepdims=True)
            l = np.exp(w - m).sum(axis=1, keepdims=True)
            r = _lazy_reference(w)
            pb = bf16_round(np.exp(w - r)) * np.exp(r - m)             # rounded in the frame of its tile, rescaled exactly
            out[a:b, h] = bf16_round((pb @ v[a:b, h // rep]) / l)
            lse[a:b, h] = (m + np.log(l))[:, 0]
    return out, lse


def varlen_attention_backward_model(q, k, v, cu_seqlens, dout, causal=True, softmax_scale=None):
    """-> (dq, dk, dv): bf16 values in fp64; arguments as oracle.attention.varlen_attention_backward.  out / lse are this model's own
    forward at the same scale, as the GPU tests take them from varlen_attn_fwd_lse."""
    q, k, v, dout = (np.asarray(x, np.float64) for x in (q, k, v, dout))
    t, hq, d = q.shape
    rep = hq // k.shape[1]
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(d)
    out, lse = varlen_attention_model(q, k, v, cu_seqlens, causal, softmax_scale)
    dq, dk, dv = np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)
    cu = [int(c) for c in cu_seqlens]
    for a, b in zip(cu[:-1], cu[1:]):
        for h in range(hq if b > a else 0):
            g = h // rep
            p = np.exp(_scores(q[a:b, h], k[a:b, g], scale, causal) - lse[a:b, h, None])
            do = dout[a:b, h]
            dvec = (do * out[a:b, h]).sum(axis=1, keepdims=True)
            ds = bf16_round(p * (do @ v[a:b, g].T - dvec))
            dv[a:b, g] += bf16_round(p).T @ do
            dq[a:b, h] = bf16_round(ds @ k[a:b, g] * scale)
            dk[a:b, g] += ds.T @ q[a:b, h] * scale
    return dq, bf16_round(dk), bf16_round(dv)


# ---- input families ------------------------------------------------------------------------------------------------------------------
# name -> (softmax_scale or None = d^-0.5, |q|, |k|, |v|, shape of k: None | "spike" | "ramp").  What each reaches:
#   default        control: the numbers of the existing tests through the new gates
#   small_scale    nearly flat rows
#   scale_0p25 / scale_1p0   logits ~N(0, 2.8^2) / N(0, 11^2): peaked rows, the forward's reference exponent moves every tile
#   loud_qk        the logits of scale ~1.4, but through the OPERANDS
#   quiet_qk_loud_v  uniform softmax, output magnitude from V
#   tiny_v         outputs near 1e-2: absolute-tolerance shortcuts fail here
#   spike* / ramp*   late jumps of the running maximum (two loud keys; logits creeping up along the sequence and one jump), at the default
#                  scale and at 0.25
FAMILIES = {
    "default": (None, 1.0, 1.0, 1.0, None),
    "small_scale": (0.02, 1.0, 1.0, 1.0, None),
    "scale_0p25": (0.25, 1.0, 1.0, 1.0, None),
    "scale_1p0": (1.0, 1.0, 1.0, 1.0, None),
    "loud_qk": (None, 4.0, 4.0, 1.0, None),
    "quiet_qk_loud_v": (None, 0.05, 0.05, 30.0, None),
    "tiny_v": (0.5, 1.0, 1.0, 0.01, None),
    "spike": (None, 1.0, 1.0, 1.0, "spike"),
    "spike_0p25": (0.25, 1.0, 1.0, 1.0, "spike"),
    "ramp": (None, 1.0, 1.0, 1.0, "ramp"),
    "ramp_0p25": (0.25, 1.0, 1.0, 1.0, "ramp"),
}
VISION_SCALE = 0.2            # head_dim 64 / 80 forwards: neither 64^-0.5 = 0.125 nor 80^-0.5 = 0.112


def family_scale(family):
    return FAMILIES[family][0]


def make_inputs(family, total_q, hq, hkv, seed, d=128, total_k=None):
    """-> q [total_q, hq, d], k, v [total_k, hkv, d], dout [total_q, hq, d]: float32 arrays holding bf16 values, drawn in this order
    from one seeded generator (for |q| = |k| = |v| = 1 these are the numbers of the existing tests' make_qkv / _case).  The spike and
    the ramp act on the packed key rows like test_attention_rescale_path / test_attention_lazy_exponent_ramp: rows total / 2 and
    total - 3 times 6 and 9; rows scaled by linspace(0.2, 2.5) and one row at 57 % of the way times 5."""
    _, mq, mk, mv, shape = FAMILIES[family]
    total_k = total_q if total_k is None else total_k
    rng = np.random.default_rng(seed)
    f = lambda n, h, mag: bf16_round(rng.standard_normal((n, h, d), dtype=np.float32) * np.float32(mag))  # noqa: E731
    q, k, v, do = f(total_q, hq, mq), f(total_k, hkv, mk), f(total_k, hkv, mv), f(total_q, hq, 1.0)
    if shape == "ramp":
        k = bf16_round(k * np.linspace(0.2, 2.5, total_k)[:, None, None])
        k[(57 * total_k) // 100] = bf16_round(k[(57 * total_k) // 100] * 5)
    elif shape == "spike":
        k[total_k // 2] = bf16_round(k[total_k // 2] * 6)
        k[max(total_k - 3, 0)] = bf16_round(k[max(total_k - 3, 0)] * 9)
    return tuple(x.astype(np.float32) for x in (q, k, v, do))
