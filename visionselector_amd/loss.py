"""Fused LM cross-entropy for the training forwards.

`causal_lm_loss` has the signature and the result of transformers' `ForCausalLMLoss` (what `self.loss_function` resolves to for
the causal LMs): labels padded by one ignore_index and shifted, mean over the valid tokens (or sum / num_items_in_batch).  The
logits stay as they are -- no fp32 copy, no log-softmax tensor: vsel_token_logprob_fwd reads every valid row once, the backward
reads it once more and writes the gradient in the logits' dtype; rows whose label is ignore_index are never read.  The reference
computes the same loss in torch (qwen-vl-finetune/compression_method/selector_model.py:293-305,
llava-ov-15/compression_method/selector_model.py:353).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops


def shift_labels_for_causal_lm(labels: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    """ForCausalLMLoss's shift: token n is predicted from position n - 1, the last position predicts nothing.
    labels int [..., L] -> int64 [prod(...) * L], contiguous."""
    labels = torch.nn.functional.pad(labels, (0, 1), value=ignore_index)
    return labels[..., 1:].contiguous().view(-1).to(torch.int64)


class _FusedLmLoss(torch.autograd.Function):
    """loss = -sum(logprob over the valid rows) / denom, denom = the number of valid rows (a device value) or num_items_in_batch."""

    @staticmethod
    def forward(ctx, logits2d, targets, ignore_index, denom):
        _, lse, total, n_valid = ops.token_logprob_fwd(logits2d, targets, ignore_index, reduce=True)
        if denom is None:
            denom = n_valid.to(torch.float32)                       # 0 valid rows: -0 / 0 = NaN, as F.cross_entropy's mean
        ctx.save_for_backward(logits2d, targets, lse, -1.0 / denom)
        ctx.ignore_index = ignore_index
        return (-total / denom).reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        logits2d, targets, lse, neg_inv = ctx.saved_tensors
        scale = (grad_loss.to(torch.float32).reshape(1) * neg_inv).contiguous()
        return ops.token_logprob_bwd(logits2d, targets, lse, grad_scale=scale, ignore_index=ctx.ignore_index), None, None, None


def causal_lm_loss(logits: torch.Tensor, labels: Optional[torch.Tensor], vocab_size: int,
                   num_items_in_batch=None, ignore_index: int = -100, shift_labels: Optional[torch.Tensor] = None,
                   **kwargs) -> torch.Tensor:
    """Drop-in for transformers.loss.loss_utils.ForCausalLMLoss on GPU logits [..., L, V] (bf16 / fp32): the same scalar (fp32),
    the gradient in the logits' dtype.  The logits are viewed as [rows, V] (no copy, no upcast), the labels are shifted in torch on
    the int64 labels, and nothing is read on the host: the valid-row count and 1 / num_items_in_batch stay on the device."""
    if shift_labels is None:
        targets = shift_labels_for_causal_lm(labels, ignore_index)
    else:
        targets = shift_labels.contiguous().view(-1).to(torch.int64)
    logits2d = logits.view(-1, vocab_size)
    targets = targets.to(logits2d.device)
    denom = None
    if num_items_in_batch is not None:
        if torch.is_tensor(num_items_in_batch):
            denom = num_items_in_batch.to(device=logits2d.device, dtype=torch.float32).reshape(1)
        else:
            denom = torch.full((1,), float(num_items_in_batch), dtype=torch.float32, device=logits2d.device)
    return _FusedLmLoss.apply(logits2d, targets, int(ignore_index), denom)


def use_fused_lm_loss(model, enable: bool = True):
    """Make `model.loss_function` (what the training forwards of hf_qwen25vl / hf_llavaov15 and transformers' own
    Qwen2_5_VLForConditionalGeneration.forward call) the fused loss, or with enable=False remove the override again so that the
    property falls back to transformers' loss for the model's loss_type.  -> model."""
    if enable:
        model.loss_function = causal_lm_loss
    elif "_loss_function" in model.__dict__:
        del model._loss_function
    return model
