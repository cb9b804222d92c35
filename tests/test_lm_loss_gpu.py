"""vsel_token_logprob_fwd / _bwd and causal_lm_loss on the GPU against the fp64 oracle (tests/lm_loss_ref.py), DESIGN.md §16.

Forward gate, per input family: the kernel's row error against the oracle <= max(2 x the largest row error of torch's own
F.cross_entropy(x.float(), t, reduction="none") on the same device tensors, 1 fp32 ulp of max(|x_t|, |lse|)) -- two correctly rounded
fp32 results may differ by an ulp, the factor 2 covers another summation order over V terms.  lse the same way against
torch.logsumexp(x.float()).  Backward gate: every element within one ulp of the output dtype of the oracle rounded once to it
(lm_loss_ref.grad_gate): the kernel's value is within about 1e-5 relative of the true one, so rounding can move it by one step at most.
The backward is a function of (logits, targets, lse, c): it is fed the oracle's lse rounded to fp32 and checked against the oracle
evaluated at that stored lse (0.5 fp32 ulp of an lse of 12 is already 4 fp32 ulps of every exp(x - lse)); end to end, through the
kernel's own lse, it is checked in bf16 (test_autograd_*, test_causal_lm_loss_*), where that difference is far inside a step."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lm_loss_ref as ref

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f32": torch.float32}


def strided_rows(values: torch.Tensor, stride: int, offset: int = 1) -> torch.Tensor:
    """[rows, V] values -> the same values as rows `stride` elements apart in a buffer, the first row `offset` elements in."""
    rows, v = values.shape
    buf = torch.zeros(offset + max(rows, 1) * stride + 8, dtype=values.dtype, device=values.device)
    view = buf.as_strided((rows, v), (stride, 1), offset)
    view.copy_(values)
    return view


def randn(rows, v, dtype, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(rows, v, device="cuda", generator=g) * scale).to(DT[dtype])


def targets_for(rows, v, seed, ignore=()):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, v, (rows,), generator=g)
    if rows:
        t[0] = 0
        t[-1] = v - 1                                               # first and last column
    for i in ignore:
        t[i] = -100
    return t.cuda()


def forward_gate(name, x, t, lp, lse, ignore_index=-100):
    """asserts the forward gate on the rows with a finite oracle value, exact agreement (inf / NaN / zeros) on the others"""
    from visionselector_amd import ops  # noqa: F401
    o_lse, o_lp = ref.lse_logprob(x, t.cpu().numpy(), ignore_index)
    xs = ref.as_f64(x)
    tn = t.cpu().numpy()
    valid = tn != ignore_index
    fin = valid & np.isfinite(o_lp) & np.isfinite(o_lse)
    k_lp, k_lse = ref.as_f64(lp), ref.as_f64(lse)
    assert not k_lp[~valid].any() and not k_lse[~valid].any(), name
    rest = valid & ~fin
    assert np.array_equal(k_lp[rest], o_lp[rest], equal_nan=True) and np.array_equal(np.isnan(k_lse[rest]), np.isnan(o_lse[rest])), name
    if not fin.any():
        return
    idx = torch.from_numpy(np.nonzero(fin)[0]).cuda()
    xf = x.index_select(0, idx).float()
    t_lp = ref.as_f64(-F.cross_entropy(xf, t.index_select(0, idx), reduction="none"))
    t_lse = ref.as_f64(torch.logsumexp(xf, -1))
    x_t = xs[np.nonzero(fin)[0], tn[fin]]
    e_k, e_t = np.abs(k_lp[fin] - o_lp[fin]), np.abs(t_lp - o_lp[fin])
    l_k, l_t = np.abs(k_lse[fin] - o_lse[fin]), np.abs(t_lse - o_lse[fin])
    print(f"lm_loss fwd {name}: logprob err kernel {e_k.max():.3e} torch {e_t.max():.3e} | lse err kernel {l_k.max():.3e} "
          f"torch {l_t.max():.3e} | rows {int(fin.sum())}")
    assert (e_k <= np.maximum(2 * e_t.max(), ref.ulp(np.maximum(np.abs(x_t), np.abs(o_lse[fin])), "f32"))).all(), name
    assert (l_k <= np.maximum(2 * l_t.max(), ref.ulp(o_lse[fin], "f32"))).all(), name


def backward_gate(name, x, t, dtype, c_rows=None, c_scale=None, ignore_index=-100):
    """the backward kernel on (x, t, fp32(oracle lse), c) against the oracle at that stored lse"""
    from visionselector_amd import ops
    tn = t.cpu().numpy()
    o_lse, _ = ref.lse_logprob(x, tn, ignore_index)
    lse32 = torch.from_numpy(o_lse.astype(np.float32)).cuda()
    g = ops.token_logprob_bwd(x, t, lse32, grad_rows=c_rows, grad_scale=c_scale, ignore_index=ignore_index)
    assert g.shape == x.shape and g.dtype == x.dtype and g.is_contiguous()
    c = np.ones(x.shape[0])
    if c_rows is not None:
        c = c * ref.as_f64(c_rows)
    if c_scale is not None:
        c = c * float(c_scale[0])
    want = ref.grad(x, tn, c, ignore_index, lse=ref.as_f64(lse32))
    ok, worst = ref.grad_gate(g, want, dtype)
    print(f"lm_loss bwd {name}: worst element {worst:.3f} ulp({dtype})")
    assert ok, (name, worst)
    zero = (tn == ignore_index) | (tn < 0) | (tn >= x.shape[1])
    assert not ref.as_f64(g)[zero].any(), name
    return g


# 4096 is the largest vocabulary of the kernel's one-chunk-per-thread form (fp64 terms), 4099 the first of the streaming form
CASES = [(v, r) for v in (1, 7, 8, 9, 1000, 4099) for r in (1, 3, 300)] + [(4096, 3), (152064, 3)]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("vocab,rows", CASES)
def test_forward_backward_shapes_and_strides(vocab, rows, dtype):
    """every vocabulary / row count, rows at stride V, V + 1 and V + 8 from a base pointer one element in (odd strides, a misaligned
    first row): the results do not depend on the layout, and pass both gates"""
    from visionselector_amd import ops
    vals = randn(rows, vocab, dtype, seed=vocab + rows)
    t = targets_for(rows, vocab, seed=rows, ignore=(1,) if rows > 2 else ())
    c_rows = torch.linspace(-1.5, 2.0, rows, device="cuda")
    c_scale = torch.tensor([0.37], device="cuda")
    first = None
    for stride in (vocab, vocab + 1, vocab + 8):
        x = strided_rows(vals, stride)
        lp, lse = ops.token_logprob_fwd(x, t)
        g = ops.token_logprob_bwd(x, t, lse, grad_rows=c_rows, grad_scale=c_scale)
        if first is None:
            first = (lp, lse, g)
            forward_gate(f"N(0,1) {dtype} V={vocab} rows={rows}", x, t, lp, lse)
            backward_gate(f"N(0,1) {dtype} V={vocab} rows={rows}", x, t, dtype, c_rows, c_scale)
        else:
            assert torch.equal(lp, first[0]) and torch.equal(lse, first[1]) and torch.equal(g, first[2]), stride
    xc = vals.contiguous()                                            # and from an aligned, contiguous tensor
    lp, lse = ops.token_logprob_fwd(xc, t)
    assert torch.equal(lp, first[0]) and torch.equal(lse, first[1])
    assert torch.equal(ops.token_logprob_bwd(xc, t, lse, grad_rows=c_rows, grad_scale=c_scale), first[2])


def test_offsets_beyond_2_31_elements():
    """rows 2^30 + 8 elements apart in an uninitialised bf16 buffer: the third row starts past 2^31 elements"""
    from visionselector_amd import ops
    stride, rows, v = 2 ** 30 + 8, 3, 1000
    buf = torch.empty(2 * stride + v + 16, dtype=torch.bfloat16, device="cuda")
    x = buf.as_strided((rows, v), (stride, 1), 1)
    vals = randn(rows, v, "bf16", seed=11)
    x.copy_(vals)
    t = targets_for(rows, v, seed=3)
    lp, lse = ops.token_logprob_fwd(x, t)
    lp0, lse0 = ops.token_logprob_fwd(vals, t)
    assert torch.equal(lp, lp0) and torch.equal(lse, lse0)
    forward_gate("2^31 offsets", x, t, lp, lse)
    assert torch.equal(ops.token_logprob_bwd(x, t, lse), ops.token_logprob_bwd(vals, t, lse0))
    del buf, x


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_targets(dtype):
    from visionselector_amd import ops
    rows, v = 9, 1000
    x = strided_rows(randn(rows, v, dtype, seed=5), v + 1)
    base = targets_for(rows, v, seed=9)
    base[base == 5] = 6                                              # 5 is the other ignore_index below
    lp_all, lse_all = ops.token_logprob_fwd(x, base)                 # none ignored
    forward_gate(f"targets none ignored {dtype}", x, base, lp_all, lse_all)
    backward_gate(f"targets none ignored {dtype}", x, base, dtype)
    # all ignored: zeros everywhere, also for a non-default ignore_index
    for ign in (-100, 5):
        t = torch.full((rows,), ign, dtype=torch.int64, device="cuda")
        lp, lse, total, n = ops.token_logprob_fwd(x, t, ignore_index=ign, reduce=True)
        assert not lp.any() and not lse.any() and float(total) == 0.0 and int(n) == 0
        assert not ops.token_logprob_bwd(x, t, lse, ignore_index=ign).any()
    # mixed, with a non-default ignore_index: -100 is then an out-of-range target like any other
    t = base.clone()
    t[2] = 5
    t[4] = 5
    lp, lse, total, n = ops.token_logprob_fwd(x, t, ignore_index=5, reduce=True)
    assert int(n) == rows - 2 and float(lp[2]) == 0.0 and float(lse[4]) == 0.0
    keep = [i for i in range(rows) if i not in (2, 4)]
    assert torch.equal(lp[keep], lp_all[keep]) and torch.equal(lse[keep], lse_all[keep])
    forward_gate(f"targets ignore_index=5 {dtype}", x, t, lp, lse, ignore_index=5)
    backward_gate(f"targets ignore_index=5 {dtype}", x, t, dtype, ignore_index=5)
    # out of range (vocab, -5; -100 under another ignore_index): NaN for that row alone, a zero gradient row, the others unchanged
    for bad, ign in ((v, -100), (-5, -100), (-100, 5)):
        t = base.clone()
        t[3] = bad
        lp, lse, total, n = ops.token_logprob_fwd(x, t, ignore_index=ign, reduce=True)
        g = ops.token_logprob_bwd(x, t, lse, ignore_index=ign)
        torch.cuda.synchronize()                                     # no device error
        assert bool(torch.isnan(lp[3])) and bool(torch.isnan(lse[3])) and bool(torch.isnan(total)) and int(n) == rows
        assert not g[3].any()
        others = [i for i in range(rows) if i != 3]
        x_wo, t_wo = strided_rows(x[others], v + 1), t[others]
        lp_wo, lse_wo = ops.token_logprob_fwd(x_wo, t_wo, ignore_index=ign)
        assert torch.equal(lp[others], lp_wo) and torch.equal(lse[others], lse_wo)
        assert torch.equal(g[others], ops.token_logprob_bwd(x_wo, t_wo, lse_wo, ignore_index=ign))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("vocab", [1000, 4099])
def test_value_families(vocab, dtype):
    from visionselector_amd import ops
    rows = 12
    t = targets_for(rows, vocab, seed=21, ignore=(5,))
    fams = {"N(0,1)x30": randn(rows, vocab, dtype, seed=31, scale=30.0)}
    spike = randn(rows, vocab, dtype, seed=32)
    spike[torch.arange(rows), torch.arange(rows) * 7 % vocab] = 3e4   # one +3e4 per row (29952 once stored as bf16)
    fams["spike 3e4"] = spike
    block = randn(rows, vocab, dtype, seed=33)
    block[:, 100:900] = float("-inf")                                 # whole 16-byte vectors and whole threads see only -inf
    block[3, :vocab - 1] = float("-inf")                              # one finite entry, the last
    fams["-inf block"] = block
    on_inf = block.clone()
    t_inf = t.clone()
    t_inf[2] = 500                                                    # a target on -inf: logprob -inf, lse finite
    for name, vals in fams.items():
        x = strided_rows(vals, vocab + 1)
        lp, lse = ops.token_logprob_fwd(x, t)
        forward_gate(f"{name} {dtype} V={vocab}", x, t, lp, lse)
        backward_gate(f"{name} {dtype} V={vocab}", x, t, dtype, c_scale=torch.tensor([1.0 / 7], device="cuda"))
    x = strided_rows(on_inf, vocab + 1)
    lp, lse = ops.token_logprob_fwd(x, t_inf)
    assert float(lp[2]) == float("-inf") and bool(torch.isfinite(lse[2]))
    forward_gate(f"target on -inf {dtype} V={vocab}", x, t_inf, lp, lse)
    backward_gate(f"target on -inf {dtype} V={vocab}", x, t_inf, dtype)
    # a row of all -inf, a row with a NaN, a row with a +inf: NaN for each, the neighbours bit for bit as without them
    clean = randn(rows, vocab, dtype, seed=34)
    lp0, lse0 = ops.token_logprob_fwd(clean, t)
    g0 = ops.token_logprob_bwd(clean, t, lse0)
    dirty = clean.clone()
    dirty[1, :] = float("-inf")
    dirty[4, vocab // 2] = float("nan")
    dirty[8, vocab - 1] = float("inf")
    x = strided_rows(dirty, vocab + 8)
    lp, lse = ops.token_logprob_fwd(x, t)
    g = ops.token_logprob_bwd(x, t, lse)
    torch.cuda.synchronize()
    bad = [1, 4, 8]
    good = [i for i in range(rows) if i not in bad]
    assert bool(torch.isnan(lp[bad]).all()) and bool(torch.isnan(lse[bad]).all())
    assert torch.equal(lp[good], lp0[good]) and torch.equal(lse[good], lse0[good]) and torch.equal(g[good], g0[good])
    forward_gate(f"NaN / inf rows {dtype} V={vocab}", x, t, lp, lse)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_row_invariance_determinism_and_sum(dtype):
    from visionselector_amd import ops
    rows, v = 300, 4099
    vals = randn(rows, v, dtype, seed=41)
    t = targets_for(rows, v, seed=42, ignore=(7, 8))
    c = torch.tensor([-1.0 / 290], device="cuda")
    lp, lse, total, n = ops.token_logprob_fwd(vals, t, reduce=True)
    g = ops.token_logprob_bwd(vals, t, lse, grad_scale=c)
    lp2, lse2, total2, n2 = ops.token_logprob_fwd(vals, t, reduce=True)            # two runs: bit-identical
    assert torch.equal(lp, lp2) and torch.equal(lse, lse2) and torch.equal(total, total2) and int(n) == int(n2) == rows - 2
    assert torch.equal(g, ops.token_logprob_bwd(vals, t, lse, grad_scale=c))
    mid = 150
    alone_x, alone_t = vals[mid:mid + 1].clone(), t[mid:mid + 1].clone()           # the row alone
    lp_a, lse_a = ops.token_logprob_fwd(alone_x, alone_t)
    assert torch.equal(lp_a, lp[mid:mid + 1]) and torch.equal(lse_a, lse[mid:mid + 1])
    assert torch.equal(ops.token_logprob_bwd(alone_x, alone_t, lse_a, grad_scale=c)[0], g[mid])
    t_n = t.clone()                                                                  # its neighbours ignored
    t_n[mid - 3:mid] = -100
    t_n[mid + 1:mid + 4] = -100
    lp_n, lse_n = ops.token_logprob_fwd(vals, t_n)
    assert torch.equal(lp_n[mid], lp[mid]) and torch.equal(lse_n[mid], lse[mid])
    assert torch.equal(ops.token_logprob_bwd(vals, t_n, lse_n, grad_scale=c)[mid], g[mid])
    # sum_out: the fixed order of include/vsel.h over the kernel's own fp32 log-probabilities; more rows than one 1024 stride too
    assert float(total) == float(ref.fixed_order_sum(lp.cpu().numpy()))
    big = randn(2500, 9, dtype, seed=43)
    tb = targets_for(2500, 9, seed=44, ignore=(0, 17, 2499))
    lpb, _, totb, nb = ops.token_logprob_fwd(big, tb, reduce=True)
    assert float(totb) == float(ref.fixed_order_sum(lpb.cpu().numpy())) and int(nb) == 2497
    # no rows: nothing but sum = 0, n_valid = 0
    e = ops.token_logprob_fwd(torch.empty(0, 9, dtype=DT[dtype], device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda"),
                              reduce=True)
    assert e[0].numel() == 0 and float(e[2]) == 0.0 and int(e[3]) == 0


def test_autograd_function_end_to_end_bf16():
    """ops.token_logprobs: the gradient through the kernel's own lse against the true oracle, one bf16 ulp; lse is not differentiable"""
    from visionselector_amd import ops
    rows, v = 7, 1000
    x = randn(rows, v, "bf16", seed=51).requires_grad_(True)
    t = targets_for(rows, v, seed=52, ignore=(3,))
    w = torch.linspace(-2.0, 1.0, rows, device="cuda")
    lp, lse = ops.token_logprobs(x, t)
    (lp * w).sum().backward()
    ok, worst = ref.grad_gate(x.grad, ref.grad(x, t.cpu().numpy(), w), "bf16")
    print(f"lm_loss autograd bf16: worst element {worst:.3f} ulp(bf16)")
    assert ok and x.grad.dtype == torch.bfloat16 and not x.grad[3].any()
    lp, lse = ops.token_logprobs(x, t)
    with pytest.raises(RuntimeError, match="lse"):
        (lp.sum() + lse.sum()).backward()


def test_no_hidden_copy_of_the_logits():
    from visionselector_amd.loss import causal_lm_loss
    rows, v = 64, 8192
    logits = randn(rows, v, "bf16", seed=61).view(1, rows, v).requires_grad_(True)
    labels = torch.randint(0, v, (1, rows), device="cuda")
    causal_lm_loss(logits.detach(), labels, v)                        # library load, allocator warm-up
    torch.cuda.synchronize()
    nbytes = rows * v * 2
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = causal_lm_loss(logits, labels, v)
    torch.cuda.synchronize()
    fwd_delta = torch.cuda.max_memory_allocated() - base
    loss.backward()
    torch.cuda.synchronize()
    both_delta = torch.cuda.max_memory_allocated() - base
    print(f"lm_loss peak memory: forward +{fwd_delta} B, forward + backward +{both_delta} B, logits {nbytes} B")
    assert fwd_delta < nbytes and both_delta < 2 * nbytes
    assert logits.grad.dtype == torch.bfloat16 and logits.grad.shape == logits.shape


@pytest.mark.parametrize("num_items", [None, 5, "tensor"])
def test_causal_lm_loss_matches_ForCausalLMLoss(num_items):
    from transformers.loss.loss_utils import ForCausalLMLoss
    from visionselector_amd.loss import causal_lm_loss
    b, l, v = 2, 9, 1000
    vals = randn(b * l, v, "bf16", seed=71).view(b, l, v)
    labels = torch.randint(0, v, (b, l), generator=torch.Generator().manual_seed(72)).cuda()
    labels[0, :4] = -100
    labels[1, 6] = -100
    n = torch.tensor(5, device="cuda") if num_items == "tensor" else num_items
    xa, xb = vals.clone().requires_grad_(True), vals.clone().requires_grad_(True)
    la = causal_lm_loss(xa, labels, v, num_items_in_batch=n)
    lb = ForCausalLMLoss(xb, labels, v, num_items_in_batch=n)
    la.backward()
    lb.backward()
    assert la.dtype == lb.dtype == torch.float32 and la.shape == lb.shape
    t = ref.hf_shift(labels.cpu().numpy())
    _, lp = ref.lse_logprob(vals.view(-1, v), t)
    denom = float((t != -100).sum()) if num_items is None else 5.0
    want = -lp.sum() / denom
    e_k, e_t = abs(float(la.detach()) - want), abs(float(lb.detach()) - want)
    print(f"lm_loss causal_lm_loss num_items={num_items}: loss err kernel {e_k:.3e} torch {e_t:.3e}")
    assert e_k <= max(2 * e_t, float(ref.ulp(want, "f32")))
    # logits.grad: within the backward gate of the oracle, and of what HF's chain leaves in the bf16 leaf (both are roundings of values
    # within 1e-5 relative of the same number, so they are equal or adjacent)
    ok, worst = ref.grad_gate(xa.grad.view(-1, v), ref.grad(vals.view(-1, v), t, -1.0 / denom), "bf16")
    assert ok, worst
    hf = ref.as_f64(xb.grad.view(-1, v))
    diff = np.abs(ref.as_f64(xa.grad.view(-1, v)) - hf) / ref.ulp(hf, "bf16")
    diff[(np.abs(hf) < ref.TINY) & (np.abs(ref.as_f64(xa.grad.view(-1, v))) < ref.TINY)] = 0.0
    print(f"lm_loss causal_lm_loss num_items={num_items}: grad vs oracle {worst:.3f} ulp(bf16), vs HF {diff.max():.3f} ulp(bf16)")
    assert diff.max() <= 1.0
    # shift_labels given: the same result without the internal shift
    xc = vals.clone().requires_grad_(True)
    lc = causal_lm_loss(xc, None, v, num_items_in_batch=n, shift_labels=torch.from_numpy(t).view(b, l).cuda())
    lc.backward()
    assert torch.equal(lc, la) and torch.equal(xc.grad, xa.grad)


def test_causal_lm_loss_all_ignored():
    from visionselector_amd.loss import causal_lm_loss
    x = randn(18, 1000, "bf16", seed=81).view(2, 9, 1000).requires_grad_(True)
    labels = torch.full((2, 9), -100, dtype=torch.int64, device="cuda")
    loss = causal_lm_loss(x, labels, 1000)
    loss.backward()
    assert bool(torch.isnan(loss)) and not x.grad.any()
