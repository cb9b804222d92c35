"""GPU parity of every attention forward / backward form at NON-DEFAULT softmax scales and hard numerics, against the fp64 oracle
(oracle/attention.py).  tests/test_attn_gpu.py and tests/test_attn_bwd_gpu.py vary shapes and schedules on N(0, 1) inputs at
scale = d^-0.5; this file varies the numbers -- the input families of tests/attn_model_ref.py (FAMILIES: small / 0.25 / 1.0 scales, loud
and quiet operands, tiny V, spiked and ramped keys at two scales; head_dim 64 / 80 at scale 0.2) -- through every kernel form, each
forced with the existing knobs and CONFIRMED BY KERNEL NAME from the library's profiler (a case that fell back to another form fails).

Gates (none taken from the code under test):
  forward    parity.check_fwd unchanged (1 bf16 ulp at row scale, 8 at rowmax / 8, >= 93 % within one, mean <= 1e-3 max(1, |O|max)), plus the
             mean bound WITHOUT its floor (mean |err| <= 1e-3 |O|max: the floor would hide everything in the tiny-v family); the bit
             identities the other files assert between forms (4 / 8 waves, 64 rows per wave, group-shared vs per head) again per family.
  lse        |err| <= 1e-4 max(1, |lse|max) against the fp64 log-sum-exp at the same scale; rows without a visible key -inf on both sides.
  backward   max |err| / max |ref| <= 2^-6 per tensor (unchanged), and per (sequence, head) slice max |err_slice| <= 2 e_model_slice +
             2^-9 max |ref_tensor| (parity.check_grad_slices), e_model = the error of tests/attn_model_ref.py itself on that slice;
             tests/test_attn_model_cpu.py proves on the CPU that every family at both backward shapes keeps the model inside these gates and
             the share of slices the model misses by > 2^-6 under 25 %.
Every comparison is logged through parity.record (kinds attn_fwd, attn_grad, attn_grad_slice).

Cuts, to keep the host-side fp64 work near what the other files already pay: the group-in-parts backward runs the families in
PARTS_FAMILIES (the P / dS arithmetic of its kernel is the grouped dkdv64 form's, which runs every family; what is its own -- fp32 partials
and the scaled group sum -- is reached by a default, a peaked, a scaled-small-V and a ramped family); non-causal cases of the key-range
parts forward do not exist (the form is causal only).

Observed on MI355X, worst per family over all forms: forward max_ulp_row 1.0 (gate 1) and max_ulp_row8 5.0 - 7.5 (gate 8) in every
family; tensor-level gradient ratio 0.0040 (small_scale) ... 0.0139 (ramp) (gate 0.0156); slice error over slice gate 0.40 (small_scale)
... 0.47 (ramp) (gate 1) -- the kernels sit on the model, the margin is the gate's factor 2; share of slices the model itself misses
0 ... 0.25 (loud_qk, the 3-token sequence; cap 0.25).  The per-case records go to the parity log (tools/merge_parity.py knows the kind
attn_grad_slice); the merged per-case file is not committed for its size (14 k lines).
Mutation check (off-tree builds, not committed): 128^-0.5 baked into the dK epilogue of the 4-wave dK / dV kernel -> 12 cases of
test_backward_forms red (every family whose scale is not the default), tests/test_attn_bwd_gpu.py green (95 passed); 128^-0.5 baked into
attn_fwd_gqa_kernel's exponent -> 12 cases of test_forward_group_shared_forms red, tests/test_attn_gpu.py green (125 passed).
"""
import functools
import os

import numpy as np
import pytest
import torch

import attn_model_ref as amr
import parity
from oracle import attention as oattn

pytestmark = pytest.mark.gpu

FAMILY_NAMES = list(amr.FAMILIES)
FWD_SHAPE = ([300, 129, 64], 4, 2)                                  # 4 / 8 waves, two KV streams, 64 rows per wave (test_rows64_*)
GQA_SHAPE = ([31, 32, 33, 64, 65, 1, 127, 300], 28, 4)              # group-shared forms (test_gqa_shared_*)
KEY_PARTS_SHAPE = ([2368], 4, 4)                                    # key-range parts (test_key_range_parts_*)
BWD_SHAPE = ([64, 65, 3, 200], 4, 2)                                # test_attention_backward_matches_oracle's ragged batch
PARTS_SHAPE = ([1025, 129, 64, 2000], 8, 2)                         # test_dkdv_group_in_parts_*
PARTS_FAMILIES = ["default", "scale_1p0", "tiny_v", "ramp_0p25"]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from visionselector_amd import ops as _ops
    return _ops


def _case():
    return os.environ.get("PYTEST_CURRENT_TEST", "?").split("::")[-1].split(" ")[0]


def _cu(lens):
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int32)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).bfloat16().cuda()


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _profiled(fn, knobs, want):
    """Run fn() under the knobs; the attention kernels the profiler saw must be exactly `want`."""
    from visionselector_amd import _native as N
    with N.debug_knob(**knobs):
        N.profile_start()
        res = fn()
        prof = N.profile_stop()
    ran = {n for n in prof if n.startswith("attn_") or n.startswith("varlen_attn")}
    assert ran == set(want), (knobs, prof)
    return res


def check_fwd(got, ref, tag=""):
    """parity.check_fwd, and the mean bound without the max(1, .) floor."""
    m = parity.check_fwd(_case() + tag, _np(got) if torch.is_tensor(got) else got, ref)
    assert m["mean_abs_err"] <= parity.MEAN_ABS_FWD * m["max_abs_ref"], (tag, m)
    return m


@functools.lru_cache(maxsize=4)
def _fwd_case(family, shape, causal, d=128, scale=None):
    lens, hq, hkv = shape
    q, k, v, do = amr.make_inputs(family, sum(lens), hq, hkv, seed=sum(lens) + hq + d, d=d)
    cu = _cu(lens)
    sc = scale if scale is not None else amr.family_scale(family)
    ref = oattn.varlen_attention(q, k, v, cu, causal=causal, softmax_scale=sc)
    lse = amr.lse_reference(q, k, cu, causal, sc)
    return q, k, v, cu, sc, ref, lse


def _as_shape(shape):
    return (tuple(shape[0]), shape[1], shape[2])


# ---- forward: per-head forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_forward_per_head_forms(ops, family, causal):
    """4 waves, 8 waves, 64 rows per wave: bit-identical outputs and log-sum-exps; two KV streams: another summation order, within a bf16
    rounding.  All four against the oracle."""
    q, k, v, cu, sc, ref, lse_ref = _fwd_case(family, _as_shape(FWD_SHAPE), causal)
    L = max(FWD_SHAPE[0])
    qd, kd, vd, cud = _dev(q), _dev(k), _dev(v), torch.from_numpy(cu).cuda()
    run = lambda: ops.varlen_attn_fwd_lse(qd, kd, vd, cud, L, causal=causal, softmax_scale=sc)  # noqa: E731
    base = dict(attn_gqa=0, attn_key_parts=0)
    w4 = _profiled(run, dict(base, attn_waves=4, attn_split=0, attn_rows64=0), ["varlen_attn_fwd_kernel"])
    w8 = _profiled(run, dict(base, attn_waves=8, attn_split=0, attn_rows64=0), ["varlen_attn_fwd_kernel"])
    r64 = _profiled(run, dict(base, attn_waves=0, attn_split=0, attn_rows64=1), ["attn_fwd64_kernel"])
    two = _profiled(run, dict(base, attn_waves=0, attn_split=1, attn_rows64=0), ["varlen_attn_fwd_kernel"])
    plain = _profiled(lambda: ops.varlen_attn(qd, kd, vd, cud, L, causal=causal, softmax_scale=sc),
                      dict(base, attn_waves=4, attn_split=0, attn_rows64=0), ["varlen_attn_fwd_kernel"])
    for tag, (o, l) in (("[w4]", w4), ("[w8]", w8), ("[r64]", r64), ("[two]", two)):
        check_fwd(o, ref, tag)
        parity.check_lse(_case() + tag, _np(l), lse_ref)
    for o, l in (w8, r64):
        assert torch.equal(o, w4[0]) and torch.equal(l, w4[1])
    assert torch.equal(plain, w4[0])
    assert float((two[0].float() - w4[0].float()).abs().max()) <= 2 ** -6 * float(w4[0].float().abs().max())


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_forward_group_shared_forms(ops, family, causal):
    """attn_fwd_gqa_kernel and attn_fwd_gqa64_kernel (generated body) against the per-head kernel: bit-identical, and against the oracle."""
    q, k, v, cu, sc, ref, lse_ref = _fwd_case(family, _as_shape(GQA_SHAPE), causal)
    L = max(GQA_SHAPE[0])
    qd, kd, vd, cud = _dev(q), _dev(k), _dev(v), torch.from_numpy(cu).cuda()
    run = lambda: ops.varlen_attn_fwd_lse(qd, kd, vd, cud, L, causal=causal, softmax_scale=sc)  # noqa: E731
    per_head = _profiled(run, dict(attn_gqa=0, attn_split=0, attn_rows64=0), ["varlen_attn_fwd_kernel"])
    g8 = _profiled(run, dict(attn_gqa=1, attn_gqa_form=0, attn_split=0, attn_rows64=0), ["attn_fwd_gqa_kernel"])
    g64 = _profiled(run, dict(attn_gqa=1, attn_gqa_form=1, attn_split=0, attn_rows64=0), ["attn_fwd_gqa64_kernel"])
    check_fwd(g8[0], ref, "[gqa]")
    parity.check_lse(_case(), _np(g8[1]), lse_ref)
    for o, l in (g8, g64):
        assert torch.equal(o, per_head[0]) and torch.equal(l, per_head[1])


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_forward_key_range_parts(ops, family):
    """attn_fwd64_parts_kernel (generated body, raw partials) + attn_fwd64_merge_kernel: against the oracle, within a bf16 rounding of the
    unsplit form, log-sum-exp through vsel_varlen_attn_fwd_ws."""
    from visionselector_amd import _native as N
    lens, hq, hkv = KEY_PARTS_SHAPE
    q, k, v, cu, sc, ref, lse_ref = _fwd_case(family, _as_shape(KEY_PARTS_SHAPE), True)
    qd, kd, vd, cud = _dev(q), _dev(k), _dev(v), torch.from_numpy(cu).cuda()
    got = _profiled(lambda: ops.varlen_attn(qd, kd, vd, cud, lens[0], softmax_scale=sc, key_parts=True), dict(attn_key_parts=-1),
                    ["attn_fwd64_parts_kernel", "attn_fwd64_merge_kernel"])
    check_fwd(got, ref)
    with N.debug_knob(attn_key_parts=0):
        base, lse0 = ops.varlen_attn_fwd_lse(qd, kd, vd, cud, lens[0], softmax_scale=sc)
    assert float((got.float() - base.float()).abs().max()) <= 2 ** -7 * float(base.float().abs().max())
    parity.check_lse(_case() + "[unsplit]", _np(lse0), lse_ref)
    lib = N.lib()
    need = lib.vsel_varlen_attn_fwd_workspace_bytes(1, lens[0], lens[0], hq, hkv, 128, 1)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out, lse = torch.empty_like(qd), torch.empty(lens[0], hq, dtype=torch.float32, device="cuda")
    N.check(lib.vsel_varlen_attn_fwd_ws(None, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), cud.data_ptr(), 1, lens[0], lens[0], hq, hkv, 128,
                                        sc if sc is not None else 128 ** -0.5, 1, out.data_ptr(), lse.data_ptr(), ws.data_ptr(), ws.numel()))
    assert torch.equal(out, got)
    parity.check_lse(_case() + "[parts]", _np(lse), lse_ref)


# ---- forward: other entries ----------------------------------------------------------------------------------------------------------
def _one_page_per_sequence(k, v, klens):
    n, page = len(klens), max(klens)
    kp, vp = np.zeros((n, page) + k.shape[1:], np.float32), np.zeros((n, page) + k.shape[1:], np.float32)
    cu_k = _cu(klens)
    for s in range(n):
        kp[s, :klens[s]], vp[s, :klens[s]] = k[cu_k[s]:cu_k[s + 1]], v[cu_k[s]:cu_k[s + 1]]
    return kp, vp, np.arange(n, dtype=np.int32)[:, None]


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_forward_separate_query_and_key_packings(ops, family, causal):
    """varlen_attn_kv, queries shorter than keys (bottom-right aligned mask): per-head kernel and the 64-rows-per-wave form, bit-identical."""
    qlens, klens, hq, hkv = [70, 200, 33], [300, 200, 1000], 4, 2
    q, k, v, _ = amr.make_inputs(family, sum(qlens), hq, hkv, seed=41, total_k=sum(klens))
    sc = amr.family_scale(family)
    cq, ck = torch.from_numpy(_cu(qlens)).cuda(), torch.from_numpy(_cu(klens)).cuda()
    qd, kd, vd = _dev(q), _dev(k), _dev(v)
    run = lambda: ops.varlen_attn_kv(qd, kd, vd, cq, ck, max(qlens), causal=causal, softmax_scale=sc)  # noqa: E731
    a = _profiled(run, dict(attn_split=0, attn_pack=0, attn_rows64=0), ["varlen_attn_fwd_kernel"])
    kp, vp, bt = _one_page_per_sequence(k, v, klens)
    ref = oattn.paged_attention(q, kp, vp, _cu(qlens), np.array(klens), bt, causal=causal, softmax_scale=sc)
    check_fwd(a, ref)
    if causal:                      # (the form test_rows64_forward_with_longer_key_sequences reaches)
        assert torch.equal(a, _profiled(run, dict(attn_split=0, attn_pack=0, attn_rows64=1), ["attn_fwd64_kernel"]))


@pytest.mark.parametrize("page_size", [16, 100])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_forward_paged(ops, family, causal, page_size):
    """paged_attn on scattered pages: chunked prefill, plain prefill, decode and a q > k sequence (leading rows see no key -> zeros)."""
    hq, hkv, qlens, klens = 8, 2, [70, 200, 1, 40], [300, 200, 517, 25]
    pages_per = [-(-kl // page_size) for kl in klens]
    n_pages = sum(pages_per) + 3
    rng = np.random.default_rng(page_size)
    perm = rng.permutation(n_pages)
    bt = np.zeros((len(qlens), max(pages_per)), np.int32)
    cur = 0
    for s, pp in enumerate(pages_per):
        bt[s, :pp] = perm[cur:cur + pp]
        cur += pp
    q, kc, vc, _ = amr.make_inputs(family, sum(qlens), hq, hkv, seed=page_size + 1, total_k=n_pages * page_size)
    kc, vc = kc.reshape(n_pages, page_size, hkv, 128), vc.reshape(n_pages, page_size, hkv, 128)
    sc = amr.family_scale(family)
    cu_q = _cu(qlens)
    args = (_dev(q), _dev(kc), _dev(vc), torch.from_numpy(cu_q).cuda(), torch.tensor(klens, dtype=torch.int32).cuda(), torch.from_numpy(bt).cuda(),
            max(qlens))
    one = _profiled(lambda: ops.paged_attn(*args, causal=causal, softmax_scale=sc), dict(attn_split=0, attn_pack=0), ["varlen_attn_fwd_kernel"])
    two = _profiled(lambda: ops.paged_attn(*args, causal=causal, softmax_scale=sc), dict(attn_split=1, attn_pack=0), ["varlen_attn_fwd_kernel"])
    ref = oattn.paged_attention(q, kc, vc, cu_q, np.array(klens), bt, causal=causal, softmax_scale=sc)
    check_fwd(one, ref, "[one]")
    check_fwd(two, ref, "[two]")
    if causal:
        a = int(cu_q[3])
        assert float(one[a:a + 15].float().abs().max()) == 0.0 and float(two[a:a + 15].float().abs().max()) == 0.0


@pytest.mark.parametrize("b,hq,hkv,lq,lk,causal", [(2, 8, 2, 130, 130, True), (2, 8, 2, 130, 130, False), (2, 4, 2, 5, 300, True)])
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_forward_head_major(ops, family, b, hq, hkv, lq, lk, causal):
    """attn_head_major on [B, H, L, d] tensors, V as a transposed view of the packed tensor.  (130 tokens, not 200: on 2 x 200 unmasked tokens
    at scale 0.02 the error MODEL itself has 92.8 % of its elements within one ulp, under the forward gate's 93 %; at 130 it has >= 95.7 %
    in every family -- tests/test_attn_model_cpu.py::test_model_forward_on_the_head_major_inputs.)"""
    q, k, v, _ = amr.make_inputs(family, b * lq, hq, hkv, seed=b + lq, total_k=b * lk)          # packed [B L, H, d]
    sc = amr.family_scale(family)
    qh = _dev(q).view(b, lq, hq, 128).transpose(1, 2).contiguous()
    kh = _dev(k).view(b, lk, hkv, 128).transpose(1, 2).contiguous()
    vh = _dev(v).view(b, lk, hkv, 128).transpose(1, 2)                                          # a view
    out = _profiled(lambda: ops.attn_head_major(qh, kh, vh, causal=causal, softmax_scale=sc),
                    dict(attn_gqa=0, attn_split=0, attn_pack=0, attn_rows64=0), ["varlen_attn_fwd_kernel"])
    assert out.shape == (b, lq, hq, 128)
    kp, vp, bt = _one_page_per_sequence(k, v, [lk] * b)
    ref = oattn.paged_attention(q, kp, vp, _cu([lq] * b), np.array([lk] * b), bt, causal=causal, softmax_scale=sc)
    check_fwd(out.reshape(b * lq, hq, 128), ref)


@pytest.mark.parametrize("s_q", [1, 3])
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_forward_kvcache(ops, family, s_q):
    """kvcache_attn: s_q new tokens appended in place to a contiguous cache, then causal attention over cache + new keys (decode: s_q = 1)."""
    from visionselector_amd import _native as N
    batch, hq, hkv, l_cache, ends = 3, 8, 2, 160, [100, 1, 157]
    q, kc, vc, _ = amr.make_inputs(family, batch * s_q, hq, hkv, seed=7 + s_q, total_k=batch * l_cache)
    _, kn, vn, _ = amr.make_inputs(family, 1, 1, hkv, seed=9 + s_q, total_k=batch * s_q)
    if amr.FAMILIES[family][4] is not None:                 # spike / ramp act on packed rows: give the NEW keys the jump
        kn = parity.bf16_round(kn * 6).astype(np.float32)
    sc = amr.family_scale(family)
    kc, vc = kc.reshape(batch, l_cache, hkv, 128), vc.reshape(batch, l_cache, hkv, 128)
    kcd, vcd = _dev(kc), _dev(vc)
    N.profile_start()
    out, lse = ops.kvcache_attn(_dev(q).view(batch, s_q, hq, 128), kcd, vcd, k=_dev(kn).view(batch, s_q, hkv, 128),
                                v=_dev(vn).view(batch, s_q, hkv, 128), cache_seqlens=torch.tensor(ends, dtype=torch.int32).cuda(),
                                softmax_scale=sc, causal=True, return_softmax_lse=True)
    prof = N.profile_stop()
    assert {n for n in prof if not n.startswith("<")} == {"kvcache_append_kernel", "varlen_attn_fwd_kernel"}, prof
    kc2, vc2 = kc.copy(), vc.copy()
    for b_ in range(batch):
        kc2[b_, ends[b_]:ends[b_] + s_q] = kn[b_ * s_q:(b_ + 1) * s_q]
        vc2[b_, ends[b_]:ends[b_] + s_q] = vn[b_ * s_q:(b_ + 1) * s_q]
    assert np.array_equal(_np(kcd), kc2) and np.array_equal(_np(vcd), vc2)
    klens = [e + s_q for e in ends]
    ref = oattn.paged_attention(q, kc2, vc2, _cu([s_q] * batch), np.array(klens), np.arange(batch)[:, None], causal=True, softmax_scale=sc)
    check_fwd(out.reshape(batch * s_q, hq, 128), ref)
    scale = sc if sc is not None else 128 ** -0.5
    for b_ in range(batch):
        for i in range(s_q):
            for h in range(hq):
                w = kc2[b_, :klens[b_] - (s_q - 1 - i), h // (hq // hkv)].astype(np.float64) @ q[b_ * s_q + i, h].astype(np.float64) * scale
                want = w.max() + np.log(np.exp(w - w.max()).sum())
                assert abs(float(lse[b_, h, i]) - want) <= parity.LSE_TOL * max(1.0, abs(want)), (b_, i, h)


@pytest.mark.parametrize("lens,hq,hkv,causal", [([100, 64, 3, 333], 4, 2, True), ([100, 64, 3, 333], 4, 2, False), ([64, 64, 16, 48], 2, 2, False)])
@pytest.mark.parametrize("d", [64, 80])
def test_forward_vision_tower_head_dims_off_their_default_scale(ops, d, lens, hq, hkv, causal):
    """head_dim 64 / 80 at scale 0.2 (neither 64^-0.5 nor 80^-0.5): 4 and 8 waves, bit-identical."""
    q, k, v, cu, sc, ref, lse_ref = _fwd_case("default", (tuple(lens), hq, hkv), causal, d, amr.VISION_SCALE)
    qd, kd, vd, cud = _dev(q), _dev(k), _dev(v), torch.from_numpy(cu).cuda()
    outs = [_profiled(lambda: ops.varlen_attn_fwd_lse(qd, kd, vd, cud, max(lens), causal=causal, softmax_scale=sc), dict(attn_waves=nw),
                      ["varlen_attn_fwd_kernel"]) for nw in (4, 8)]
    check_fwd(outs[0][0], ref)
    parity.check_lse(_case(), _np(outs[0][1]), lse_ref)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- backward ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _bwd_case(family, shape, causal):
    lens, hq, hkv = shape
    q, k, v, do = amr.make_inputs(family, sum(lens), hq, hkv, seed=sum(lens) + hq)
    cu, sc = _cu(lens), amr.family_scale(family)
    ref = oattn.varlen_attention_backward(q, k, v, cu, do, causal=causal, softmax_scale=sc)
    model = amr.varlen_attention_backward_model(q, k, v, cu, do, causal, sc)
    return q, k, v, do, cu, sc, ref, model, amr.lse_reference(q, k, cu, causal, sc)


def _check_grads(tag, got, ref, model, cu):
    for name, g, r, m in zip(("dq", "dk", "dv"), got, ref, model):
        g = _np(g)
        tm = parity.grad_metrics(g, r)
        sm = parity.grad_slice_metrics(g, r, m, cu)
        print(_case(), tag, name, "tensor", round(tm["max_abs_err_over_max"], 5), "slice/gate", round(sm["max_err_over_gate"], 3),
              "slice/slicemax", round(sm["max_err_over_slice_max"], 4), "model", round(sm["max_model_err_over_slice_max"], 4))
        parity.check_grad(f"{_case()}{tag}[{name}]", g, r)
        parity.check_grad_slices(f"{_case()}{tag}[{name}]", g, r, m, cu)


BWD_FORMS = {      # knobs, kernels
    "w4": (dict(attn_bwd_waves=4, attn_bwd_split=0, attn_bwd_dq64=0, attn_bwd_dkdv64=0), ["attn_bwd_dq_kernel", "attn_bwd_dkdv_kernel"]),
    "w8": (dict(attn_bwd_waves=8, attn_bwd_split=0, attn_bwd_dq64=0, attn_bwd_dkdv64=0), ["attn_bwd_dq_kernel", "attn_bwd_dkdv_kernel"]),
    "w4split": (dict(attn_bwd_waves=4, attn_bwd_split=1, attn_bwd_dq64=0, attn_bwd_dkdv64=0),
                ["attn_bwd_dq_kernel", "attn_bwd_dkdv_kernel", "attn_bwd_group_sum_kernel"]),
    "r64": (dict(attn_bwd_waves=4, attn_bwd_split=0, attn_bwd_dq64=1, attn_bwd_dkdv64=1), ["attn_bwd_dq64_kernel", "attn_bwd_dkdv64_kernel"]),
    "r64split": (dict(attn_bwd_waves=4, attn_bwd_split=1, attn_bwd_dq64=1, attn_bwd_dkdv64=1),
                 ["attn_bwd_dq64_kernel", "attn_bwd_dkdv64_kernel", "attn_bwd_group_sum_kernel"]),
}


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_backward_forms(ops, family, causal):
    """dQ + dK / dV with 4 and 8 waves, the per-q-head split with the group sum, the 64-row passes grouped and split; out / lse from
    varlen_attn_fwd_lse at the same scale.  dQ is bit-identical in every form, the 64-row passes reproduce the 4-wave forms bit for bit.

    ([scale_1p0-False] sat at 1.029 of the slice gate while the model rounded every P on the grid of its ROW maximum; with the forward's
    lazy reference exponent in the model -- the grid the kernel really rounds on -- every family sits at <= 0.47 of the gate.)"""
    lens = BWD_SHAPE[0]
    q, k, v, do, cu, sc, ref, model, lse_ref = _bwd_case(family, _as_shape(BWD_SHAPE), causal)
    qd, kd, vd, dod, cud = _dev(q), _dev(k), _dev(v), _dev(do), torch.from_numpy(cu).cuda()
    out, lse = ops.varlen_attn_fwd_lse(qd, kd, vd, cud, max(lens), causal=causal, softmax_scale=sc)
    parity.check_lse(_case(), _np(lse), lse_ref)
    res = {}
    for form, (knobs, names) in BWD_FORMS.items():
        res[form] = _profiled(lambda: ops.varlen_attn_bwd(dod, qd, kd, vd, out, lse, cud, max(lens), causal=causal, softmax_scale=sc), knobs, names)
        _check_grads(f"[{form}]", res[form], ref, model, cu)
    for form in res:
        assert torch.equal(res[form][0], res["w4"][0]), form
    for a, b in (("r64", "w4"), ("r64split", "w4split")):
        assert torch.equal(res[a][1], res[b][1]) and torch.equal(res[a][2], res[b][2]), (a, b)


@pytest.mark.parametrize("family", PARTS_FAMILIES)
def test_backward_group_in_parts(ops, family):
    """dK / dV with a group's q heads cut in two parts (fp32 partials, attn_bwd_group_sum_kernel adds and scales them)."""
    lens = PARTS_SHAPE[0]
    q, k, v, do, cu, sc, ref, model, lse_ref = _bwd_case(family, _as_shape(PARTS_SHAPE), True)
    qd, kd, vd, dod, cud = _dev(q), _dev(k), _dev(v), _dev(do), torch.from_numpy(cu).cuda()
    out, lse = ops.varlen_attn_fwd_lse(qd, kd, vd, cud, max(lens), softmax_scale=sc)
    parity.check_lse(_case(), _np(lse), lse_ref)
    run = lambda: ops.varlen_attn_bwd(dod, qd, kd, vd, out, lse, cud, max(lens), softmax_scale=sc)  # noqa: E731
    parts = _profiled(run, dict(attn_bwd_split=2, attn_bwd_dkdv64=1, attn_bwd_dq64=1),
                      ["attn_bwd_dq64_kernel", "attn_bwd_dkdv64_kernel", "attn_bwd_group_sum_kernel"])
    whole = _profiled(run, dict(attn_bwd_split=0, attn_bwd_dkdv64=1, attn_bwd_dq64=1), ["attn_bwd_dq64_kernel", "attn_bwd_dkdv64_kernel"])
    _check_grads("[parts]", parts, ref, model, cu)
    assert torch.equal(parts[0], whole[0])
    for i in (1, 2):
        assert float((parts[i].float() - whole[i].float()).abs().max()) <= 2 ** -7 * float(whole[i].float().abs().max())


# ---- wrappers at softmax_scale = 0.25 ------------------------------------------------------------------------------------------------
def test_autograd_wrapper_keeps_the_scale(ops):
    """attention.varlen_attention under autograd: forward and .backward() against the oracle at scale 0.25, and the bits of
    ops.varlen_attn_fwd_lse / ops.varlen_attn_bwd called by hand with that scale (the scale is not dropped between forward and ctx)."""
    from visionselector_amd.attention import varlen_attention
    lens, hq, hkv = [150, 64, 9], 4, 2
    q, k, v, do = amr.make_inputs("default", sum(lens), hq, hkv, seed=31)
    cu = _cu(lens)
    cud = torch.from_numpy(cu).cuda()
    qd, kd, vd = (_dev(x).requires_grad_(True) for x in (q, k, v))
    out = varlen_attention(qd, kd, vd, cud, max(lens), causal=True, softmax_scale=0.25)
    out.backward(_dev(do))
    check_fwd(out, oattn.varlen_attention(q, k, v, cu, softmax_scale=0.25))
    _check_grads("", (qd.grad, kd.grad, vd.grad), oattn.varlen_attention_backward(q, k, v, cu, do, softmax_scale=0.25),
                 amr.varlen_attention_backward_model(q, k, v, cu, do, True, 0.25), cu)
    o2, lse = ops.varlen_attn_fwd_lse(_dev(q), _dev(k), _dev(v), cud, max(lens), softmax_scale=0.25)
    g2 = ops.varlen_attn_bwd(_dev(do), _dev(q), _dev(k), _dev(v), o2, lse, cud, max(lens), softmax_scale=0.25)
    assert torch.equal(out, o2)
    for a, b in zip((qd.grad, kd.grad, vd.grad), g2):
        assert torch.equal(a, b)
    o3, _ = ops.varlen_attn_fwd_lse(_dev(q), _dev(k), _dev(v), cud, max(lens))
    assert not torch.equal(o2, o3)


def test_flash_attn_compat_functions_keep_the_scale(ops):
    from visionselector_amd.flash_attn_compat import flash_attn_func, flash_attn_varlen_func
    lens, hq, hkv = [150, 64, 9], 4, 2
    q, k, v, do = amr.make_inputs("default", sum(lens), hq, hkv, seed=33)
    cu = _cu(lens)
    cud = torch.from_numpy(cu).cuda()
    ref = oattn.varlen_attention(q, k, v, cu, softmax_scale=0.25)
    rg = oattn.varlen_attention_backward(q, k, v, cu, do, softmax_scale=0.25)
    mg = amr.varlen_attention_backward_model(q, k, v, cu, do, True, 0.25)
    with torch.no_grad():
        check_fwd(flash_attn_varlen_func(_dev(q), _dev(k), _dev(v), cud, cud, max(lens), max(lens), softmax_scale=0.25, causal=True), ref, "[nograd]")
    qd, kd, vd = (_dev(x).requires_grad_(True) for x in (q, k, v))
    out = flash_attn_varlen_func(qd, kd, vd, cud, cud, max(lens), max(lens), softmax_scale=0.25, causal=True)
    out.backward(_dev(do))
    check_fwd(out, ref, "[grad]")
    _check_grads("[varlen]", (qd.grad, kd.grad, vd.grad), rg, mg, cu)
    # dense batched form: 2 x 100 tokens
    b, L = 2, 100
    q, k, v, do = amr.make_inputs("default", b * L, hq, hkv, seed=35)
    cu = _cu([L] * b)
    ref = oattn.varlen_attention(q, k, v, cu, softmax_scale=0.25)
    with torch.no_grad():
        ob = flash_attn_func(_dev(q).view(b, L, hq, 128), _dev(k).view(b, L, hkv, 128), _dev(v).view(b, L, hkv, 128), softmax_scale=0.25, causal=True)
    assert ob.shape == (b, L, hq, 128)
    check_fwd(ob.reshape(b * L, hq, 128), ref, "[dense]")
    qd, kd, vd = (_dev(x).view(b, L, -1, 128).requires_grad_(True) for x in (q, k, v))
    og = flash_attn_func(qd, kd, vd, softmax_scale=0.25, causal=True)
    og.backward(_dev(do).view(b, L, hq, 128))
    assert torch.equal(og, ob)
    _check_grads("[dense]", tuple(t.grad.reshape(b * L, -1, 128) for t in (qd, kd, vd)),
                 oattn.varlen_attention_backward(q, k, v, cu, do, softmax_scale=0.25), amr.varlen_attention_backward_model(q, k, v, cu, do, True, 0.25), cu)


def test_hf_attention_interface_keeps_the_scaling(ops):
    """vsel_attention_forward(..., scaling=0.25): prefill on head-major tensors, prefill under autograd (packed path) and the
    _decode_attention path (Lq < Lk on tensors the strided entry cannot take)."""
    from visionselector_amd import attention as A
    b, hq, hkv, L = 2, 4, 2, 130
    q, k, v, do = amr.make_inputs("default", b * L, hq, hkv, seed=37)
    cu = _cu([L] * b)
    ref = oattn.varlen_attention(q, k, v, cu, softmax_scale=0.25)
    hm = lambda x: _dev(x).view(b, L, -1, 128).transpose(1, 2).contiguous()  # noqa: E731
    out, _ = A.vsel_attention_forward(None, hm(q), hm(k), hm(v), None, scaling=0.25)
    assert out.shape == (b, L, hq, 128)
    check_fwd(out.reshape(b * L, hq, 128), ref, "[prefill]")
    qd, kd, vd = (hm(x).requires_grad_(True) for x in (q, k, v))
    og, _ = A.vsel_attention_forward(None, qd, kd, vd, None, scaling=0.25)
    og.backward(_dev(do).view(b, L, hq, 128))
    check_fwd(og.reshape(b * L, hq, 128), ref, "[train]")
    unhm = lambda t: t.transpose(1, 2).reshape(b * L, -1, 128)  # noqa: E731
    _check_grads("[train]", (unhm(qd.grad), unhm(kd.grad), unhm(vd.grad)), oattn.varlen_attention_backward(q, k, v, cu, do, softmax_scale=0.25),
                 amr.varlen_attention_backward_model(q, k, v, cu, do, True, 0.25), cu)
    # decode against a longer cache
    lq, lk = 3, 90
    q2, k2, v2, _ = amr.make_inputs("default", b * lq, hq, hkv, seed=39, total_k=b * lk)
    kp, vp, bt = _one_page_per_sequence(k2, v2, [lk] * b)
    ref2 = oattn.paged_attention(q2, kp, vp, _cu([lq] * b), np.array([lk] * b), bt, causal=True, softmax_scale=0.25)
    hm2 = lambda x, n: _dev(x).view(b, n, -1, 128).transpose(1, 2).contiguous()  # noqa: E731
    o2 = A._decode_attention(hm2(q2, lq), hm2(k2, lk), hm2(v2, lk), 0.25, True)
    check_fwd(o2.reshape(b * lq, hq, 128), ref2, "[decode]")
    o3, _ = A.vsel_attention_forward(None, hm2(q2, lq), hm2(k2, lk), hm2(v2, lk), None, scaling=0.25)
    check_fwd(o3.reshape(b * lq, hq, 128), ref2, "[decode-head-major]")


# ---- unusable scales are refused before any launch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0.0, -0.1, float("nan"), float("inf")])
def test_unusable_softmax_scales_raise(ops, bad):
    from visionselector_amd import _native as N
    t, hq, hkv = 16, 4, 2
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")  # noqa: E731
    q, k, v = z(t, hq, 128), z(t, hkv, 128), z(t, hkv, 128)
    cu = torch.tensor([0, t], dtype=torch.int32, device="cuda")
    lse = torch.zeros(t, hq, dtype=torch.float32, device="cuda")
    one = torch.tensor([t], dtype=torch.int32, device="cuda")
    bt = torch.zeros(1, 1, dtype=torch.int32, device="cuda")
    cache = z(1, 32, hkv, 128)
    calls = {
        "varlen_attn": lambda: ops.varlen_attn(q, k, v, cu, t, softmax_scale=bad),
        "varlen_attn_fwd_lse": lambda: ops.varlen_attn_fwd_lse(q, k, v, cu, t, softmax_scale=bad),
        "varlen_attn_bwd": lambda: ops.varlen_attn_bwd(q, q, k, v, q, lse, cu, t, softmax_scale=bad),
        "paged_attn": lambda: ops.paged_attn(q, k.view(1, t, hkv, 128), v.view(1, t, hkv, 128), cu, one, bt, t, softmax_scale=bad),
        "kvcache_attn": lambda: ops.kvcache_attn(z(1, 1, hq, 128), cache, cache.clone(), cache_seqlens=8, softmax_scale=bad),
        "attn_head_major": lambda: ops.attn_head_major(z(1, hq, t, 128), z(1, hkv, t, 128), z(1, hkv, t, 128), softmax_scale=bad),
        "varlen_attn_kv": lambda: ops.varlen_attn_kv(q, k, v, cu, cu, t, softmax_scale=bad),
    }
    for name, call in calls.items():
        N.profile_start()
        with pytest.raises(N.VselError, match="scale"):
            call()
        assert not [n for n in N.profile_stop() if not n.startswith("<")], name          # nothing was launched
    lib = N.lib()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.empty_like(q)
    rc = lib.vsel_varlen_attn_fwd_ws(None, q.data_ptr(), k.data_ptr(), v.data_ptr(), cu.data_ptr(), 1, t, t, hq, hkv, 128, bad, 1, out.data_ptr(), None,
                                     ws.data_ptr(), ws.numel())
    assert rc == 1 and b"scale" in lib.vsel_last_error(), rc     # VSEL_ERR_INVALID
