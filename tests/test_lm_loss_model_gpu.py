"""The fused LM cross-entropy inside the training forward: install_selector(..., fused_lm_loss=True) against the default
on the tiny Qwen2.5-VL selector model of tests/test_hf_gpu.py -- identical weights and inputs, one image, labels on the last few
tokens only."""
import copy

import numpy as np
import pytest
import torch

import lm_loss_ref as ref
from test_hf_gpu import IMG, make_inputs, randomize_scorer, tiny_config

pytestmark = pytest.mark.gpu

# Relative L2 distance of each scorer gradient between the two paths, measured on the MI355X (profiles/lm_loss_pytest_gpu.txt): the
# paths differ only in dlogits (fp32 here: HF's chain against one rounding from fp64) and in the loss's last bit.  The gate is 4 x the
# largest measured value, and never above the 2^-6 of the attention backward tests (tests/parity.py).
MEASURED_REL_L2 = 2.7e-7
GRAD_GATE = min(4 * MEASURED_REL_L2, 2.0 ** -6)


def build(fused, state=None, **kw):
    from transformers.models.qwen2_5_vl import modeling_qwen2_5_vl as hf
    from visionselector_amd.hf_qwen25vl import install_selector
    torch.manual_seed(0)
    model = hf.Qwen2_5_VLForConditionalGeneration(tiny_config()).cuda().float().train()
    install_selector(model, budget=0.25, regularization_weight=0.7, **({"fused_lm_loss": fused} if fused is not None else {}), **kw)
    randomize_scorer(model.model.visual.importance_scorer, seed=2)
    if state is not None:
        model.load_state_dict(state)
    for n, p in model.named_parameters():
        p.requires_grad = "importance_scorer" in n
    return model


def batch(seed=5):
    inp, _ = make_inputs(seed=seed)
    labels = torch.full_like(inp["input_ids"], -100)
    labels[:, -4:] = inp["input_ids"][:, -4:]                        # the answer: the last few tokens
    assert not (labels == IMG).any()
    return dict(inp, labels=labels)


@pytest.fixture(scope="module")
def pair():
    default = build(False)
    fused = build(True, state=copy.deepcopy(default.state_dict()))
    return default, fused


def run(model, b):
    for p in model.parameters():
        p.grad = None
    out = model(**b)
    out.loss.backward()
    return out, {n: p.grad.detach().clone() for n, p in model.model.visual.importance_scorer.named_parameters()}


def test_loss_and_scorer_gradients_agree(pair):
    from transformers.loss.loss_utils import ForCausalLMLoss
    from visionselector_amd.loss import causal_lm_loss
    default, fused = pair
    assert default.loss_function is ForCausalLMLoss and fused.loss_function is causal_lm_loss
    b = batch()
    out_d, g_d = run(default, b)
    out_f, g_f = run(fused, b)
    assert torch.equal(out_d.logits, out_f.logits) and torch.equal(out_d.constraint_loss, out_f.constraint_loss)
    # the loss, constraint term included: the forward gate on the LM part (oracle on the logits as stored), the same BCE on both sides
    v = out_d.logits.shape[-1]
    t = ref.hf_shift(b["labels"].cpu().numpy())
    _, lp = ref.lse_logprob(out_d.logits.view(-1, v), t)
    extra = 0.7 * float(out_d.constraint_loss.double())
    want = -lp.sum() / (t != -100).sum() + extra
    e_k, e_t = abs(float(out_f.loss.double()) - want), abs(float(out_d.loss.double()) - want)
    print(f"lm_loss model: loss {float(out_f.loss):.7f} err fused {e_k:.3e} default {e_t:.3e}")
    assert e_k <= max(2 * e_t, float(ref.ulp(want, "f32")))
    assert sorted(g_f) == ["k_proj.bias", "k_proj.weight", "q_proj.bias", "q_proj.weight"]
    # q_proj.bias shifts every score by the same amount, which the soft top-k and the constraint mask do not see: its gradient is zero
    # in exact arithmetic and rounding noise on both paths (norm 3e-10 against 2e-3 measured), so a gradient below 1e-3 of the largest
    # of the four norms is measured against that largest norm, every other one against its own
    top = max(float(g.double().norm()) for g in g_d.values())
    assert top > 0
    for n in g_f:
        own = float(g_d[n].double().norm())
        rel = float((g_f[n].double() - g_d[n].double()).norm()) / (own if own >= 1e-3 * top else top)
        print(f"lm_loss model: scorer gradient {n}: norm {own:.3e}, relative L2 distance fused vs default {rel:.3e} (gate {GRAD_GATE:.3e})")
        assert rel <= GRAD_GATE, (n, rel)


def test_kernel_names_on_the_fused_path_only(pair):
    from visionselector_amd import _native as N
    default, fused = pair
    b = batch()
    seen = {}
    for name, model in (("default", default), ("fused", fused)):
        N.profile_start()
        run(model, b)
        torch.cuda.synchronize()
        seen[name] = N.profile_stop()
    new = {"token_logprob_fwd_kernel", "token_logprob_bwd_kernel"}
    assert new <= set(seen["fused"]) and not (new & set(seen["default"])), seen
    assert seen["fused"]["token_logprob_fwd_kernel"][1] == 1 and seen["fused"]["token_logprob_bwd_kernel"][1] == 1


def test_trainer_step_fused_and_default():
    from transformers.loss.loss_utils import ForCausalLMLoss
    from visionselector_amd.loss import causal_lm_loss
    from visionselector_amd.trainer import LisTrainer
    batches = [batch(5), batch(6)]
    state = copy.deepcopy(build(None).state_dict())
    results = {}
    for name, kw in (("plain", {}), ("off", dict(fused_lm_loss=False)), ("on", dict(fused_lm_loss=True))):
        model = build(None, state=state)
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        tr = LisTrainer(model, max_steps=4, lr=1e-2, warmup_ratio=0.0, log=lambda s: None, **kw)
        assert model.loss_function is (causal_lm_loss if name == "on" else ForCausalLMLoss)
        loss = tr.train_step(batches)
        results[name] = (loss, {n: p.detach().clone() for n, p in model.named_parameters()})
        if name == "on":
            assert np.isfinite(loss)
            for n, p in model.named_parameters():
                assert (not torch.equal(before[n], p.detach())) == ("importance_scorer" in n), n
    # fused_lm_loss=False is the construction without the argument, bit for bit
    assert results["off"][0] == results["plain"][0]
    for n, p in results["plain"][1].items():
        assert torch.equal(results["off"][1][n], p), n
    # the fused step's loss: each micro-batch loss is the same number rounded to fp32 along another route (an ulp or two apart)
    assert abs(results["on"][0] - results["plain"][0]) <= 4 * float(ref.ulp(results["plain"][0], "f32"))
