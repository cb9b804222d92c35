"""CPU checks of the attention error model (tests/attn_model_ref.py) on every input family and every BACKWARD shape of
tests/test_attn_numerics_gpu.py: the inputs must leave the fp64 oracle finite and the MODEL -- a correct kernel by construction -- inside
every gate the GPU tests then apply to the kernels:
  (a) the oracle's forward and backward are finite;
  (b) the model's forward is within the forward gate (parity.fwd_metrics: max_ulp_row <= 1, max_ulp_row8 <= 8), its mean error within the
      floor-less mean bound the tiny-v family adds, its log-sum-exp exact;
  (c) the model's gradients are within the tensor-level 2^-6 gate;
  (d) the share of (sequence, head) slices on which the model itself is beyond 2^-6 of the slice stays under the cap of the slice gate
      (parity.GRAD_SLICE_MAX_HARD_SHARE): the slice gate is twice the model's error, so it gates tightly wherever the model is tight.
A family / shape that fails here is the wrong INPUT for the GPU tests, never a reason to move a gate.
Also here, because it needs no GPU: the slice gate catches a 10 % error in one kv head of the shortest sequence that the tensor-level gate
lets through (the reason it exists), and the scale appears exactly once in each gradient of the oracle and of the model."""
import numpy as np
import pytest

import attn_model_ref as amr
import parity
from oracle import attention as oattn

# the backward shapes of tests/test_attn_numerics_gpu.py (BWD_SHAPE, PARTS_SHAPE)
SHAPES = {"ragged": ([64, 65, 3, 200], 4, 2), "parts": ([1025, 129, 64, 2000], 8, 2)}


def _cu(lens):
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int32)


_cache = {}


def _run(family, shape, causal):
    key = (family, shape, causal)
    if key not in _cache:
        lens, hq, hkv = SHAPES[shape]
        q, k, v, do = amr.make_inputs(family, sum(lens), hq, hkv, seed=sum(lens) + hq)
        cu, sc = _cu(lens), amr.family_scale(family)
        ref_o = oattn.varlen_attention(q, k, v, cu, causal=causal, softmax_scale=sc)
        ref_g = oattn.varlen_attention_backward(q, k, v, cu, do, causal=causal, softmax_scale=sc)
        mod_o, mod_lse = amr.varlen_attention_model(q, k, v, cu, causal, sc)
        mod_g = amr.varlen_attention_backward_model(q, k, v, cu, do, causal, sc)
        _cache.clear()                                  # (one entry: the parts shape holds ~100 MB)
        _cache[key] = (q, k, v, do, cu, sc, ref_o, ref_g, mod_o, mod_lse, mod_g)
    return _cache[key]


CASES = [(f, s, c) for f in amr.FAMILIES for s, c in (("ragged", True), ("ragged", False), ("parts", True))]


@pytest.mark.parametrize("family,shape,causal", CASES)
def test_model_sits_inside_every_gate_of_the_gpu_tests(family, shape, causal):
    q, k, v, do, cu, sc, ref_o, ref_g, mod_o, mod_lse, mod_g = _run(family, shape, causal)
    case = f"{family}-{shape}-{'causal' if causal else 'full'}"
    assert np.isfinite(ref_o).all() and all(np.isfinite(g).all() for g in ref_g)                       # (a)
    m = parity.fwd_metrics(mod_o, ref_o)                                                               # (b)
    print(case, "fwd", {x: round(m[x], 5) for x in ("max_ulp_row", "max_ulp_row8", "frac_within_1ulp", "mean_abs_err", "max_abs_ref")})
    if shape != "parts":        # the GPU tests gate no forward OUTPUT at the parts shape (backward only); there the model's stale exponents
        assert m["max_ulp_row"] <= parity.MAX_ULP_FWD and m["max_ulp_row8"] <= parity.MAX_ULP_ROW8_FWD, (case, m)     # reach 2 ulps at row scale
        assert m["frac_within_1ulp"] >= parity.MIN_FRAC_1ULP_ROW8, (case, m)
    assert m["mean_abs_err"] <= parity.MEAN_ABS_FWD * m["max_abs_ref"], (case, m)
    assert np.abs(mod_lse - amr.lse_reference(q, k, cu, causal, sc)).max() <= 1e-9
    for name, got, ref in zip(("dq", "dk", "dv"), mod_g, ref_g):
        gm = parity.grad_metrics(got, ref)                                                             # (c)
        sm = parity.grad_slice_metrics(got, ref, got, cu)                                              # (d)
        print(case, name, "tensor", round(gm["max_abs_err_over_max"], 5), "worst slice", round(sm["max_model_err_over_slice_max"], 4),
              "hard share", sm["hard_share"])
        assert gm["max_abs_err_over_max"] <= parity.MAX_REL_GRAD, (case, name, gm)
        assert sm["hard_share"] <= parity.GRAD_SLICE_MAX_HARD_SHARE, (case, name, sm)
        assert sm["max_err_over_gate"] <= 0.5 + 1e-12        # the model against its own gate: at most 1 / GRAD_SLICE_MODEL_FACTOR


@pytest.mark.parametrize("d", [64, 80])
@pytest.mark.parametrize("causal", [True, False])
def test_model_forward_at_vision_tower_head_dims(d, causal):
    lens, hq, hkv = [100, 64, 3, 333], 4, 2
    q, k, v, _ = amr.make_inputs("default", sum(lens), hq, hkv, seed=d, d=d)
    ref = oattn.varlen_attention(q, k, v, _cu(lens), causal=causal, softmax_scale=amr.VISION_SCALE)
    got, _ = amr.varlen_attention_model(q, k, v, _cu(lens), causal, amr.VISION_SCALE)
    m = parity.fwd_metrics(got, ref)
    assert np.isfinite(ref).all()
    assert m["max_ulp_row"] <= parity.MAX_ULP_FWD and m["max_ulp_row8"] <= parity.MAX_ULP_ROW8_FWD, m
    assert m["mean_abs_err"] <= parity.MEAN_ABS_FWD * m["max_abs_ref"], m


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("family", list(amr.FAMILIES))
def test_model_forward_on_the_head_major_inputs(family, causal):
    """The inputs of test_attn_numerics_gpu.py::test_forward_head_major (2 x 130 tokens, 8 / 2 heads) leave the model inside the forward gate,
    the share-within-one-ulp term included (2 x 200 tokens did not: 92.8 % at scale 0.02 without a mask)."""
    b, hq, hkv, lq = 2, 8, 2, 130
    q, k, v, _ = amr.make_inputs(family, b * lq, hq, hkv, seed=b + lq)
    cu, sc = _cu([lq] * b), amr.family_scale(family)
    m = parity.fwd_metrics(amr.varlen_attention_model(q, k, v, cu, causal, sc)[0], oattn.varlen_attention(q, k, v, cu, causal=causal, softmax_scale=sc))
    assert m["max_ulp_row"] <= parity.MAX_ULP_FWD and m["max_ulp_row8"] <= parity.MAX_ULP_ROW8_FWD, m
    assert m["frac_within_1ulp"] >= 0.95 and m["mean_abs_err"] <= parity.MEAN_ABS_FWD * m["max_abs_ref"], m


@pytest.mark.parametrize("family", ["default", "scale_1p0", "tiny_v"])
def test_slice_gate_catches_a_wrong_head_of_the_shortest_sequence(family):
    """One kv head's dV of the SHORTEST sequence times 1.1 (a wrong-item / wrong-head bug of a ragged scheduler, in miniature), applied to
    the model's own gradients: the per-slice gate trips on exactly that slice.  (With N(0, 1) dO a short sequence's dV is among the
    LARGEST of the batch -- few keys share each row's whole probability mass -- so the tensor-level gate sees this one too, at 0.07 - 0.09;
    the slices it cannot see are the small ones, next test.)"""
    q, k, v, do, cu, sc, ref_o, ref_g, mod_o, mod_lse, mod_g = _run(family, "ragged", True)
    s = int(np.argmin(SHAPES["ragged"][0]))
    bad = mod_g[2].copy()
    bad[cu[s]:cu[s + 1], 1] *= 1.1
    m = parity.grad_slice_metrics(bad, ref_g[2], mod_g[2], cu)
    assert m["max_err_over_gate"] > 1.0 and m["worst_slice"] == [s, 1], m
    with pytest.raises(AssertionError):
        parity.check_grad_slices("mutation", bad, ref_g[2], mod_g[2], cu)


def test_slice_gate_catches_what_the_tensor_gate_lets_through():
    """The gap the slice gate closes: a slice whose gradient is ~10x below the tensor's largest (uniform softmax, no mask: dV of the LONGEST
    sequence, ~1 / sqrt(L) of the shortest's) 10 % wrong in one kv head.  The tensor-level 2^-6 gate passes it; the slice gate does not."""
    q, k, v, do, cu, sc, ref_o, ref_g, mod_o, mod_lse, mod_g = _run("quiet_qk_loud_v", "ragged", False)
    mag = parity.slice_absmax(ref_g[2], cu)
    s, h = (int(x) for x in np.unravel_index(int(np.argmin(mag)), mag.shape))
    assert s == int(np.argmax(SHAPES["ragged"][0])) and mag[s, h] <= 0.1 * mag.max()
    bad = mod_g[2].copy()
    bad[cu[s]:cu[s + 1], h] *= 1.1
    assert parity.grad_metrics(bad, ref_g[2])["max_abs_err_over_max"] <= parity.MAX_REL_GRAD
    m = parity.grad_slice_metrics(bad, ref_g[2], mod_g[2], cu)
    assert m["max_err_over_gate"] > 1.0 and m["worst_slice"] == [s, h], m


def test_scale_enters_each_gradient_once():
    """dQ and dK carry the softmax scale once (and the logits once more): with q' = q / a and scale' = a * scale the logits are the same, so
    dV and dK are unchanged and dQ' = a dQ -- in the oracle exactly, which is what makes it a reference for a dropped or doubled scale."""
    lens, hq, hkv = [40, 3, 70], 4, 2
    q, k, v, do = amr.make_inputs("default", sum(lens), hq, hkv, seed=3)
    cu = _cu(lens)
    g1 = oattn.varlen_attention_backward(q, k, v, cu, do, softmax_scale=0.25)
    g2 = oattn.varlen_attention_backward(q / 4.0, k, v, cu, do, softmax_scale=1.0)
    assert np.allclose(g2[0], 4.0 * g1[0], rtol=1e-12, atol=1e-15)
    assert np.allclose(g2[1], g1[1], rtol=1e-12, atol=1e-15) and np.allclose(g2[2], g1[2], rtol=1e-12, atol=1e-15)
    m1 = amr.varlen_attention_backward_model(q, k, v, cu, do, softmax_scale=0.25)
    m2 = amr.varlen_attention_backward_model(q / 4.0, k, v, cu, do, softmax_scale=1.0)       # (a power of two: the roundings coincide)
    assert np.array_equal(m2[0], 4.0 * m1[0]) and np.array_equal(m2[1], m1[1]) and np.array_equal(m2[2], m1[2])


def test_slice_helpers_on_empty_and_zero_slices():
    """An empty sequence is no slice; a slice whose reference is exactly 0 (single-key rows: dS == 0) is gated by the additive term."""
    cu = np.array([0, 1, 1, 4])
    ref = np.zeros((4, 2, 8))
    ref[1:, :, :] = 1.0
    m = parity.grad_slice_metrics(ref, ref, ref, cu)
    assert m["n_slices"] == 4 and m["max_err_over_gate"] == 0.0 and m["hard_share"] == 0.0
    got = ref.copy()
    got[0, 0, 0] = 2.0 ** -9 * 1.01                       # the one-token sequence: reference 0, error just past the half-ulp term
    m = parity.grad_slice_metrics(got, ref, ref, cu)
    assert m["max_err_over_gate"] > 1.0 and m["worst_slice"] == [0, 0]
