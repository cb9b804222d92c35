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
memory except the next tokens -- the greedy argmax, or with do_sample ops.sample_tokens, either after ops.repetition_penalty when
one is set (one synchronisation per step, as in HF generate).  A prompt that emits eos or reaches max_new_tokens leaves the batch and
its pages return to the free list.  hf_generation_kwargs turns HF generate() keyword arguments and the model's generation_config into
packed_generate's.
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
                    temperature: float = 1.0, top_p: float = 1.0, top_k: int = 0, seed: int = 0, repetition_penalty: float = 1.0):
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
    penalize = ops.check_repetition_penalty(repetition_penalty) != 1.0
    eos = set() if eos_token_id is None else ({int(eos_token_id)} if isinstance(eos_token_id, int) else {int(e) for e in eos_token_id})
    lm = model.model.language_model
    # the token sets of the penalty: every prompt id as passed (range-checked on the host before any device work)
    sets = ops.token_sets(input_ids, model.lm_head.out_features, model.lm_head.weight.device) if penalize else None
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
        # the prompt index of each active row (the sampler's row id, the penalty's token set)
        row_ids = torch.arange(n, dtype=torch.int64, device=dev) if do_sample or penalize else None
        prev = None                                                   # the last step's tokens, which join the sets at this step
        state.mode = "decode"
        step = 0
        while True:
            if penalize and do_sample:
                pen = ops.repetition_penalty(logits, repetition_penalty, sets, row_ids=row_ids, prev_tokens=prev)
                nxt = ops.sample_tokens(pen, temperature, top_p, top_k, seed, row_ids=row_ids, step=step)
            elif penalize:
                nxt = ops.repetition_penalty(logits, repetition_penalty, sets, row_ids=row_ids, prev_tokens=prev, return_tokens=True)
            elif do_sample:
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
                if row_ids is not None:
                    row_ids = row_ids[idx]
                active = [active[i] for i in keep]
            for i, b in enumerate(active):                            # this step appends position lens[b]
                need = _cdiv(lens[b] + 1, page_size)
                if need > len(pages[b]):
                    pages[b] += pool.alloc(1)
                    bt[i, need - 1] = pages[b][-1]
            prev = nxt
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


# HF generation options packed_generate cannot honour, each with the condition under which HF's _get_logits_processor (or its search
# loop) makes it active: hf_generation_kwargs refuses them by name instead of returning kwargs that would generate something else
_UNSUPPORTED = (
    ("num_beams", lambda g: g.num_beams is not None and g.num_beams > 1),
    ("num_return_sequences", lambda g: g.num_return_sequences is not None and g.num_return_sequences > 1),
    ("guidance_scale", lambda g: g.guidance_scale is not None and g.guidance_scale != 1),
    ("sequence_bias", lambda g: g.sequence_bias is not None),
    ("encoder_repetition_penalty", lambda g: g.encoder_repetition_penalty is not None and g.encoder_repetition_penalty != 1.0),
    ("no_repeat_ngram_size", lambda g: g.no_repeat_ngram_size is not None and g.no_repeat_ngram_size > 0),
    ("encoder_no_repeat_ngram_size", lambda g: g.encoder_no_repeat_ngram_size is not None and g.encoder_no_repeat_ngram_size > 0),
    ("bad_words_ids", lambda g: g.bad_words_ids is not None),
    ("min_length", lambda g: g.min_length is not None and g.min_length > 0),
    ("min_new_tokens", lambda g: g.min_new_tokens is not None and g.min_new_tokens > 0),
    ("forced_bos_token_id", lambda g: g.forced_bos_token_id is not None),
    ("forced_eos_token_id", lambda g: g.forced_eos_token_id is not None),
    ("remove_invalid_values", lambda g: g.remove_invalid_values is True),
    ("exponential_decay_length_penalty", lambda g: g.exponential_decay_length_penalty is not None),
    ("suppress_tokens", lambda g: g.suppress_tokens is not None),
    ("begin_suppress_tokens", lambda g: g.begin_suppress_tokens is not None),
    ("watermarking_config", lambda g: getattr(g, "watermarking_config", None) is not None),
    ("renormalize_logits", lambda g: g.renormalize_logits is True),
    ("stop_strings", lambda g: getattr(g, "stop_strings", None) is not None),
    ("max_time", lambda g: getattr(g, "max_time", None) is not None),
    # the warpers HF applies only when sampling
    ("top_h", lambda g: g.do_sample and getattr(g, "top_h", None) is not None),
    ("min_p", lambda g: g.do_sample and g.min_p is not None),
    ("typical_p", lambda g: g.do_sample and g.typical_p is not None and g.typical_p < 1.0),
    ("epsilon_cutoff", lambda g: g.do_sample and g.epsilon_cutoff is not None and 0.0 < g.epsilon_cutoff < 1.0),
    ("eta_cutoff", lambda g: g.do_sample and g.eta_cutoff is not None and 0.0 < g.eta_cutoff < 1.0),
)


def hf_generation_kwargs(model, **generate_kwargs) -> dict:
    """The packed_generate keyword arguments that reproduce HF `model.generate(**generate_kwargs)`: transformers' own merge
    (GenerationMixin._prepare_generation_config: the caller's kwargs over model.generation_config over HF's global defaults, e.g.
    top_k 50) -> dict(do_sample, temperature, top_p, top_k, repetition_penalty, eos_token_id, max_new_tokens), with HF's "off" values
    as packed_generate spells them (top_p 1.0, top_k 0, repetition_penalty 1.0).  NotImplementedError, naming the option, for any
    active setting packed_generate does not implement (beam search, min-p, n-gram blocking, ..., max_length without max_new_tokens): the
    caller then runs HF generate() itself rather than getting other answers.  TypeError for keywords that are no generation option.
    `seed` is not HF's: pass it to packed_generate directly."""
    g, rest = model._prepare_generation_config(None, **generate_kwargs)
    rest = {k: v for k, v in rest.items() if k not in ("output_attentions", "output_hidden_states")}     # (outputs, not tokens)
    if rest:
        raise TypeError(f"not generation options: {sorted(rest)}")
    for name, active in _UNSUPPORTED:
        if active(g):
            raise NotImplementedError(f"packed_generate does not implement the generation option {name}={getattr(g, name)!r}; "
                                      "use the model's generate()")
    if g.max_new_tokens is None:
        raise NotImplementedError(f"packed_generate needs max_new_tokens (the merged config gives max_length={g.max_length!r} "
                                  "without it); use the model's generate() or pass max_new_tokens")
    return dict(do_sample=bool(g.do_sample), temperature=1.0 if g.temperature is None else float(g.temperature),
                top_p=1.0 if g.top_p is None else float(g.top_p), top_k=0 if g.top_k is None else int(g.top_k),
                repetition_penalty=1.0 if g.repetition_penalty is None else float(g.repetition_penalty),
                eos_token_id=g.eos_token_id, max_new_tokens=int(g.max_new_tokens))
