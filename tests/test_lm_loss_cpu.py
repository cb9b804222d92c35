"""CPU-side checks of the fused LM cross-entropy: the fp64 oracle against torch in float64, the label shift against
transformers' ForCausalLMLoss, the C entries' argument validation (which returns before any HIP call), the refusal of CPU tensors and
the loss_function override."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lm_loss_ref as ref


@pytest.fixture(scope="module")
def lib():
    from visionselector_amd import _native as N
    from visionselector_amd import build
    build.build_native(verbose=False)
    return N.lib()


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_oracle_matches_torch_float64(reduction):
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(12, 37, generator=g) * 3).bfloat16()
    x[3, 5:20] = float("-inf")
    t = torch.randint(0, 37, (12,), generator=g)
    t[[1, 7]] = -100
    t[3] = 2                                                          # (a target on -inf: test_oracle_special_rows)
    xd = x.double().requires_grad_(True)
    want = F.cross_entropy(xd, t, ignore_index=-100, reduction=reduction)
    lse, lp = ref.lse_logprob(x, t.numpy())
    valid = t.numpy() != -100
    got = {"none": -lp, "sum": -lp.sum(), "mean": -lp.sum() / valid.sum()}[reduction]
    assert np.abs(got - want.detach().numpy()).max() <= 1e-12
    assert np.abs(lse[valid] - torch.logsumexp(x.double(), -1).numpy()[valid]).max() <= 1e-12
    w = torch.randn(12, generator=g).double()
    if reduction == "none":
        (want * w).sum().backward()
        c = -w.numpy()
    else:
        want.backward()
        c = np.full(12, -1.0 if reduction == "sum" else -1.0 / valid.sum())
    assert np.abs(ref.grad(x, t.numpy(), c) - xd.grad.numpy()).max() <= 1e-12


def test_oracle_special_rows():
    x = np.zeros((6, 4))
    x[1, 2] = np.nan
    x[2, 0] = np.inf
    x[3, :] = -np.inf
    x[4, 1] = -np.inf
    lse, lp = ref.lse_logprob(x, [0, 0, 1, 2, 1, 4])
    assert lse[0] == pytest.approx(np.log(4)) and lp[0] == pytest.approx(-np.log(4))
    assert np.isnan(lse[1:4]).all() and np.isnan(lp[1:4]).all()
    assert lse[4] == pytest.approx(np.log(3)) and lp[4] == -np.inf
    assert np.isnan(lse[5]) and np.isnan(lp[5])                      # target == vocab
    g = ref.grad(x, [0, -100, -100, -100, 1, 4], 2.0)
    assert not g[1:4].any() and not g[5].any() and g[4, 1] == 2.0 and g[0, 0] == pytest.approx(1.5)
    assert ref.fixed_order_sum(np.arange(3000, dtype=np.float32)) == np.float32(3000 * 2999 / 2)


@pytest.mark.parametrize("use_shift", [False, True])
@pytest.mark.parametrize("num_items", [None, 3, "tensor"])
def test_shift_helper_and_loss_formula_match_ForCausalLMLoss(use_shift, num_items):
    """B = 2, L = 5: the pure shift helper and -sum / denominator over the oracle's log-probabilities give ForCausalLMLoss's value."""
    from transformers.loss.loss_utils import ForCausalLMLoss
    from visionselector_amd.loss import shift_labels_for_causal_lm
    g = torch.Generator().manual_seed(1)
    v = 11
    logits = torch.randn(2, 5, v, generator=g)
    labels = torch.randint(0, v, (2, 5), generator=g)
    labels[0, :2] = -100
    labels[1, 3] = -100
    shifted = shift_labels_for_causal_lm(labels)
    assert shifted.dtype == torch.int64 and shifted.is_contiguous()
    assert np.array_equal(shifted.numpy(), ref.hf_shift(labels.numpy()))
    assert np.array_equal(shifted.view(2, 5)[:, -1].numpy(), [-100, -100])
    n = torch.tensor(3) if num_items == "tensor" else num_items
    kw = dict(shift_labels=shifted.view(2, 5)) if use_shift else {}
    want = ForCausalLMLoss(logits, None if use_shift else labels, v, num_items_in_batch=n, **kw)
    _, lp = ref.lse_logprob(logits.view(-1, v), shifted.numpy())
    denom = float((shifted != -100).sum()) if num_items is None else 3.0
    assert abs(-lp.sum() / denom - float(want)) <= 1e-5
    # a non-default ignore_index is what pads the shifted labels
    assert shift_labels_for_causal_lm(labels, ignore_index=-7).view(2, 5)[:, -1].tolist() == [-7, -7]


def test_argument_validation_without_gpu(lib):
    p = 16                                                            # any non-NULL value: every check returns before a HIP call
    fwd, bwd = lib.vsel_token_logprob_fwd, lib.vsel_token_logprob_bwd

    def f(logits=p, rows=4, vocab=8, stride=8, targets=p, logprob=p, lse=p):
        return fwd(None, logits, 0, rows, vocab, stride, targets, -100, logprob, lse, None, None)

    def b(logits=p, rows=4, vocab=8, stride=8, targets=p, lse=p, grad=p):
        return bwd(None, logits, 0, rows, vocab, stride, targets, -100, lse, None, None, grad)

    for call, kw, word in ((f, dict(logits=None), b"logits"), (f, dict(targets=None), b"targets"), (f, dict(logprob=None), b"logprob"),
                           (f, dict(lse=None), b"lse"), (b, dict(logits=None), b"logits"), (b, dict(targets=None), b"targets"),
                           (b, dict(lse=None), b"lse"), (b, dict(grad=None), b"grad_logits"),
                           (f, dict(vocab=0, stride=0), b"vocab=0"), (b, dict(vocab=0, stride=0), b"vocab=0"),
                           (f, dict(stride=7), b"row_stride=7"), (b, dict(stride=7), b"row_stride=7"),
                           (f, dict(rows=-1), b"rows=-1"), (b, dict(rows=-1), b"rows=-1")):
        assert call(**kw) == 1, kw
        assert word in lib.vsel_last_error(), (kw, lib.vsel_last_error())
    for call in (f, b):
        assert call(vocab=2 ** 31, stride=2 ** 31) == 4
        assert b"vocab" in lib.vsel_last_error()
    assert fwd(None, p, 7, 4, 8, 8, p, -100, p, p, None, None) == 1 and b"dtype" in lib.vsel_last_error()


def test_ops_refuse_cpu_tensors(lib):
    from visionselector_amd import loss, ops
    x, t = torch.zeros(3, 8), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.token_logprobs(x, t)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.token_logprob_fwd(x, t)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.token_logprob_bwd(x, t, torch.zeros(3))
    with pytest.raises(RuntimeError, match="GPU only"):
        loss.causal_lm_loss(torch.zeros(1, 3, 8), t.view(1, 3), 8)


def test_loss_function_override_set_and_removed():
    from test_hf_gpu import tiny_config
    from transformers.loss.loss_utils import ForCausalLMLoss
    from transformers.models.qwen2_5_vl import modeling_qwen2_5_vl as hf
    from visionselector_amd.hf_qwen25vl import install_selector
    from visionselector_amd.loss import causal_lm_loss, use_fused_lm_loss
    model = hf.Qwen2_5_VLForConditionalGeneration(tiny_config())
    assert model.loss_function is ForCausalLMLoss
    install_selector(model, budget=0.25)
    assert model.loss_function is ForCausalLMLoss                    # the default leaves transformers' loss in place
    assert use_fused_lm_loss(model) is model and model.loss_function is causal_lm_loss
    use_fused_lm_loss(model, enable=False)
    assert model.loss_function is ForCausalLMLoss and "_loss_function" not in model.__dict__
    use_fused_lm_loss(model, enable=False)                            # removing twice is fine
    install_selector(model, budget=0.25, fused_lm_loss=True)
    assert model.loss_function is causal_lm_loss
