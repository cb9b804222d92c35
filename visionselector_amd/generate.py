"""Batched generation (greedy or sampled) of compressed prompts on a paged KV cache (Qwen2.5-VL selector models).

packed_prefill stops at the first token.  packed_generate continues from the same packed inputs (packed._packed_inputs: tower,
M-RoPE positions, ragged LIS, splice) and decodes every prompt of the batch together:
  prefill  the LLM over the packed compressed prompts with the var-len attention over cu_seqlens' (the calls packed_prefill
           makes), plus ONE append launch per layer that writes the prompts' keys / values into their pages;
  decode   one new token per active prompt, packed as [1, B_active, D]: per layer one vsel_kvcache_attn_fwd (append launch +
           attention over the prompt's pages).
The attention interface `vsel_paged` (register_paged_attention) reads the layer's pools through `module.layer_idx` and the
paged state from the `vsel_paged` keyword argument of the LLM forward -- the route packed_prefill uses for cu_seq_lens_q.
Page allocation is host bookkeeping: lengths are known from the kept-token counts and the step count, so nothing reads device
memory except the next tokens -- the greedy argmax, or with do_sample ops.sample_tokens (one synchronisation per step, as in HF
generate).  A prompt that emits eos or reaches max_new_tokens leaves the batch and its pages return to the free list.
"""
from __future__ import annotations

from typing import Sequence

import torch

from . import ops
from .attention import vsel_attention_forward
from .packed import _packed_inputs

ATTN_NAME_PAGED = "vsel_paged"


class PagedKVPool:
    """Per-layer K / V pools [n_pages, page_size, Hkv, d] bf16 and a host-side free list of page numbers."""

    def __init__(self, n_layers: int, n_pages: int, page_size: int, hkv: int, head_dim: int, device, dtype=torch.bfloat16):
        if dtype != torch.bfloat16:
            raise TypeError("the paged KV cache is bfloat16")
        if n_pages < 1 or page_size < 1:
            raise ValueError("need at least one page of at least one position")
        self.n_pages, self.page_size, self.hkv, self.head_dim = n_pages, page_size, hkv, head_dim
        self.k = [torch.zeros(n_pages, page_size, hkv, head_dim, dtype=dtype, device=device) for _ in range(n_layers)]
        self.v = [torch.zeros(n_pages, page_size, hkv, head_dim, dtype=dtype, device=device) for _ in range(n_layers)]
        self._free = list(range(n_pages - 1, -1, -1))       # pop() hands out the lowest page first

    @property
    def n_free(self) -> int:
        return len(self._free)

    def alloc(self, n: int) -> list:
        if n > len(self._free):
            raise RuntimeError(f"KV page pool exhausted: {n} pages wanted, {len(self._free)} of {self.n_pages} free")
        return [self._free.pop() for _ in range(n)]

    def release(self, pages: Sequence[int]) -> None:
        self._free.extend(pages)


class PagedState:
    """What the vsel_paged attention reads during one LLM forward: the pool, the mode, and its device index tensors.
    prefill: tok_table int32 [T, max_pages] (token t -> its prompt's block-table row), tok_pos int32 [T] (its position);
    decode:  block_table int32 [B_active, max_pages] (-1-padded), cache_seqlens int32 [B_active] (keys before this step)."""

    def __init__(self, pool: PagedKVPool):
        self.pool = pool
        self.mode = None
        self.tok_table = self.tok_pos = self.block_table = self.cache_seqlens = None


def vsel_paged_attention_forward(module, query, key, value, attention_mask, dropout: float = 0.0, scaling=None, is_causal=None,
                                 **kwargs):
    """transformers AttentionInterface function for packed_generate.  query [1, Hq, T, d], key / value [1, Hkv, T, d] (packed).
    Prefill: vsel_attention_forward over cu_seq_lens_q, then the prompt keys / values appended into the pages (append-only
    vsel_kvcache_attn_fwd, one token per row).  Decode: T = active prompts, one token each -> vsel_kvcache_attn_fwd."""
    st = kwargs.get("vsel_paged")
    if not isinstance(st, PagedState):
        raise RuntimeError("the vsel_paged attention runs inside packed_generate (it needs the vsel_paged= forward argument)")
    if dropout:
        raise NotImplementedError("attention dropout is not supported")
    kc, vc = st.pool.k[module.layer_idx], st.pool.v[module.layer_idx]
    k_rows, v_rows = key.permute(2, 0, 1, 3), value.permute(2, 0, 1, 3)          # [T, 1, Hkv, d] views, no copies
    if st.mode == "prefill":
        out, _ = vsel_attention_forward(module, query, key, value, attention_mask, scaling=scaling, is_causal=is_causal, **kwargs)
        ops.kvcache_attn(None, kc, vc, k=k_rows, v=v_rows, cache_seqlens=st.tok_pos, block_table=st.tok_table)
        return out, None
    if st.mode != "decode":
        raise RuntimeError(f"unknown paged mode {st.mode!r}")
    q = query.permute(2, 0, 1, 3)                                                  # [B_active, 1, Hq, d]
    out = ops.kvcache_attn(q, kc, vc, k=k_rows, v=v_rows, cache_seqlens=st.cache_seqlens, block_table=st.block_table,
                           softmax_scale=scaling, causal=True)
    return out.view(1, q.shape[0], q.shape[2], q.shape[3]), None


def register_paged_attention() -> str:
    """Register `vsel_paged` (and its mask flavour, the un-padded flash one) with transformers, next to the names
    attention.replace_qwen2_vl_attention_class registers."""
    from transformers import AttentionInterface
    AttentionInterface.register(ATTN_NAME_PAGED, vsel_paged_attention_forward)
    try:
        from transformers.masking_utils import AttentionMaskInterface, flash_attention_mask
        AttentionMaskInterface.register(ATTN_NAME_PAGED, flash_attention_mask)
    except ImportError:
        pass
    return ATTN_NAME_PAGED


def _h2d(values, dtype, device) -> torch.Tensor:
    return torch.tensor(values, dtype=dtype).pin_memory().to(device, non_blocking=True)


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


@torch.no_grad()
def packed_generate(model, input_ids: Sequence[torch.Tensor], pixel_values: torch.Tensor, image_grid_thw: torch.Tensor,
                    images_per_prompt: Sequence[int], max_new_tokens: int, budgets: float | None = None, eos_token_id=None,
                    page_size: int = 64, pool: PagedKVPool | None = None, return_logits: bool = False, do_sample: bool = False,
                    temperature: float = 1.0, top_p: float = 1.0, top_k: int = 0, seed: int = 0):
    """Greedy or sampled generation for a batch of image prompts (arguments as packed_prefill).
    -> dict(tokens: B lists of new token ids (each ends at eos or after max_new_tokens), kept [B], first_logits [B, vocab]
            (bit-identical to packed_prefill's logits), pool, and with return_logits: logits, B lists of [vocab] per step).
    Decode positions continue each prompt's M-RoPE positions from its last prompt token (+1 per step), which is what the batch-1
    Qwen2_5_VLForConditionalGeneration_Selector.generate() uses ("decode positions").
    pool: a PagedKVPool to draw pages from (default: one sized for this call); every page drawn is back on its free list on return.
    do_sample=False: the next token is the argmax of the logits.  do_sample=True: ops.sample_tokens with temperature, top_k (0: off),
    top_p and seed, as HF's do_sample with those warpers; the draw of prompt b at its s-th new token uses row id b and
    step s, so it does not depend on the other prompts or on when they leave the batch.  A prompt whose logits hold a NaN / +inf
    (or no finite value) raises RuntimeError."""
    if max_new_tokens < 1:
        raise ValueError("max_new_tokens must be >= 1")
    if not isinstance(do_sample, bool):
        raise TypeError(f"do_sample must be a bool, got {do_sample!r}")
    if do_sample:
        ops.check_sampling_args(temperature, top_p, top_k, seed)
    eos = set() if eos_token_id is None else ({int(eos_token_id)} if isinstance(eos_token_id, int) else {int(e) for e in eos_token_id})
    lm = model.model.language_model
    register_paged_attention()
    p = _packed_inputs(model, input_ids, pixel_values, image_grid_thw, images_per_prompt, budgets)
    emb, pos, cu, lengths = p["inputs_embeds"], p["position_ids"], p["cu_seqlens"], p["lengths"]
    dev, n = emb.device, len(lengths)
    attn0 = lm.layers[0].self_attn
    hkv, hd = lm.config.num_key_value_heads, attn0.head_dim
    # the last new token is never fed back: a prompt holds at most L + max_new_tokens - 1 keys
    most = [_cdiv(L + max_new_tokens - 1, page_size) for L in lengths]
    if pool is None:
        pool = PagedKVPool(len(lm.layers), sum(most), page_size, hkv, hd, dev)
    elif pool.page_size != page_size or pool.hkv != hkv or pool.head_dim != hd or len(pool.k) != len(lm.layers):
        raise ValueError("the pool's geometry does not match the model / page_size")
    width = max(most)
    pages = [[] for _ in range(n)]
    state = PagedState(pool)
    old_impl = lm.config._attn_implementation
    try:
        for b, L in enumerate(lengths):
            pages[b] = pool.alloc(_cdiv(L, page_size))
        bt = _h2d([pg + [-1] * (width - len(pg)) for pg in pages], torch.int32, dev)
        # prefill: the packed prompts through the LLM; each layer also appends its keys / values, token t into row
        # prompt(t) of the block table at its position
        state.mode = "prefill"
        state.tok_table = bt.index_select(0, _h2d([b for b, L in enumerate(lengths) for _ in range(L)], torch.int64, dev))
        state.tok_pos = _h2d([i for L in lengths for i in range(L)], torch.int32, dev)
        lm.config._attn_implementation = ATTN_NAME_PAGED
        max_len = p["max_len"]
        hidden = lm(inputs_embeds=emb[None], position_ids=pos[:, None, :], use_cache=False, cu_seq_lens_q=cu, cu_seq_lens_k=cu,
                    max_length_q=max_len, max_length_k=max_len, vsel_paged=state).last_hidden_state[0]
        last = cu[1:].to(torch.int64) - 1
        logits = model.lm_head(hidden[last])
        first_logits = logits
        state.tok_table = state.tok_pos = None
        step_pos = pos[:, last] + 1                                   # [3, B]: the next token's M-RoPE position
        active = list(range(n))
        lens = list(lengths)
        tokens = [[] for _ in range(n)]
        step_logits = [[] for _ in range(n)]
        seqlens = _h2d(lens, torch.int32, dev)
        embed = model.get_input_embeddings()
        row_ids = torch.arange(n, dtype=torch.int64, device=dev) if do_sample else None     # the prompt index of each active row
        state.mode = "decode"
        step = 0
        while True:
            if do_sample:
                nxt = ops.sample_tokens(logits, temperature, top_p, top_k, seed, row_ids=row_ids, step=step)
            else:
                nxt = logits.argmax(-1)
            host = nxt.tolist()                                       # the one host synchronisation of a step
            keep = []
            for i, b in enumerate(active):
                if host[i] < 0:
                    raise RuntimeError(f"sampling failed for prompt {b} at step {step}: its logits hold a NaN / +inf or no finite value")
                tokens[b].append(host[i])
                if return_logits:
                    step_logits[b].append(logits[i])
                if host[i] in eos or len(tokens[b]) >= max_new_tokens:
                    pool.release(pages[b])                            # the prompt leaves the batch
                    pages[b] = []
                else:
                    keep.append(i)
            if not keep:
                break
            if len(keep) < len(active):
                idx = _h2d(keep, torch.int64, dev)
                nxt, bt, step_pos, seqlens = nxt[idx], bt[idx], step_pos[:, idx], seqlens[idx]
                if do_sample:
                    row_ids = row_ids[idx]
                active = [active[i] for i in keep]
            for i, b in enumerate(active):                            # this step appends position lens[b]
                need = _cdiv(lens[b] + 1, page_size)
                if need > len(pages[b]):
                    pages[b] += pool.alloc(1)
                    bt[i, need - 1] = pages[b][-1]
            state.block_table, state.cache_seqlens = bt, seqlens
            hidden = lm(inputs_embeds=embed(nxt)[None], position_ids=step_pos[:, None, :], use_cache=False,
                        vsel_paged=state).last_hidden_state[0]
            logits = model.lm_head(hidden)
            for b in active:
                lens[b] += 1
            seqlens = seqlens + 1
            step_pos = step_pos + 1
            step += 1
    finally:
        lm.config._attn_implementation = old_impl
        for pg in pages:
            pool.release(pg)
    out = {"tokens": tokens, "kept": p["kept"], "first_logits": first_logits, "pool": pool}
    if return_logits:
        out["logits"] = step_logits
    return out
