"""Batched generation (greedy or sampled) of compressed prompts on a paged KV cache (Qwen2.5-VL selector models).

packed_prefill stops at the first token.  packed_generate continues from the same packed inputs (packed._packed_inputs: tower,
M-RoPE positions, ragged LIS, splice) and decodes every prompt of the batch together:
  prefill  (_prefill) the LLM over the packed compressed prompts with the var-len attention over cu_seqlens' (the calls packed_prefill
           makes), plus ONE append launch per layer that writes the prompts' keys / values into their pages;
  decode   (_eager_decode) one new token per active prompt, packed as [1, B_active, D]: per layer one vsel_kvcache_attn_fwd
           (append launch + attention over the prompt's pages).
The attention interface `vsel_paged` (register_paged_attention) reads the layer's pools through `module.layer_idx` and the
paged state from the `vsel_paged` keyword argument of the LLM forward -- the route packed_prefill uses for cu_seq_lens_q.
Page allocation is host bookkeeping: lengths are known from the kept-token counts and the step count, so nothing reads device
memory except the next tokens -- the greedy argmax, or with do_sample ops.sample_tokens, either after ops.repetition_penalty when
one is set (_selector, the one selector of both decode loops; one synchronisation per step, as in HF generate).  A prompt that emits
eos or reaches max_new_tokens leaves the batch and its pages return to the free list.  hf_generation_kwargs turns HF generate() keyword
arguments and the model's generation_config into packed_generate's.
packed_generate(graph=True) keeps the decode loop on the device (_graph_decode): the LLM step is replayed from a captured
graph, the token bookkeeping is one ops.decode_advance launch per step, and the host reads a four-word status `lookahead` steps behind
instead of the tokens.  DecodeGraphs keeps the captured graphs between calls.
"""
from __future__ import annotations

import time
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


DEFAULT_LOOKAHEAD = 2        # steps the host runs ahead of the status it reads (tools/bench_generate.py --graph sweep)
_INVALID_LOGITS = "its logits hold a NaN / +inf or no finite value"


class _StepGraph:
    """The static buffers of one batch size and, once captured, the graph of the LLM decode step + lm_head over them."""

    def __init__(self, n: int, width: int, pos_dtype, pool: PagedKVPool, dev):
        # done, n_tokens (int32 [n] each) and feed (int64 [n]) share one buffer: one fill resets a call's state
        self.zeros = torch.zeros(4 * n, dtype=torch.int32, device=dev)
        self.done, self.n_tokens, self.feed = self.zeros[:n], self.zeros[n:2 * n], self.zeros[2 * n:].view(torch.int64)
        self.pos = torch.zeros(3, n, dtype=pos_dtype, device=dev)
        self.status = torch.zeros(4, dtype=torch.int32, device=dev)
        self.state = PagedState(pool)
        self.state.mode = "decode"
        self.state.cache_seqlens = torch.zeros(n, dtype=torch.int32, device=dev)
        self.state.block_table = torch.full((n, width), -1, dtype=torch.int32, device=dev)
        self.graph = self.logits = None


class DecodeGraphs:
    """The captured decode-step graphs of one model on one pool, kept between packed_generate(graph=...) calls: one graph per batch size,
    every block table `max_pages_per_prompt` wide (unused entries -1), all captured and replayed on one stream of its own.  `captures`
    counts the graphs captured so far and `capture_ms` the time spent on them (warm-up forward + capture), so a caller can see reuse."""

    def __init__(self, model, pool: PagedKVPool, max_pages_per_prompt: int):
        self.model, self.pool, self.max_pages_per_prompt = model, pool, ops._int_in("max_pages_per_prompt", max_pages_per_prompt, 1)
        self.captures, self.capture_ms = 0, 0.0
        self.stream = None
        self._steps, self._rings = {}, {}

    def _step(self, n: int, pos_dtype, dev) -> _StepGraph:
        key = (n, pos_dtype)
        if key not in self._steps:
            self._steps[key] = _StepGraph(n, self.max_pages_per_prompt, pos_dtype, self.pool, dev)
        return self._steps[key]

    def _ring(self, slots: int):
        if slots not in self._rings:
            self._rings[slots] = (torch.zeros(slots, 4, dtype=torch.int32).pin_memory(), [torch.cuda.Event() for _ in range(slots)])
        return self._rings[slots]


def _capture(graphs: DecodeGraphs, sg: _StepGraph, model, lm) -> None:
    """Warm up and capture the decode step over sg's static buffers on the current stream (graphs.stream).  Capture executes nothing and
    the warm-up is a real forward that writes K / V at cache_seqlens, so the caller runs this where the first decode step belongs and
    then replays the graph: an exact repeat of the warm-up on unchanged state, which leaves the logits in the static output."""
    embed = model.get_input_embeddings()

    def step():
        hidden = lm(inputs_embeds=embed(sg.feed)[None], position_ids=sg.pos[:, None, :], use_cache=False,
                    vsel_paged=sg.state).last_hidden_state[0]
        return model.lm_head(hidden)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=graphs.stream):          # one stream, no side streams: the graph has no parallel branches
        sg.logits = step()
    torch.cuda.synchronize()
    sg.graph = g
    graphs.captures += 1
    graphs.capture_ms += (time.perf_counter() - t0) * 1e3


def _selector(do_sample: bool, temperature, top_p, top_k, seed, repetition_penalty, sets, rows=None, logprobs: bool = False):
    """The token selector of both decode loops: select(logits [n, V], step, prev_tokens, row_ids) -> (int64 [n] tokens (-1: invalid row),
    float32 [n] log-probabilities or None).
    sets: the penalty's token sets, or None without a penalty; row_ids: the prompt index of each row (the sampler's row id, the penalty's
    token set), None when neither is on; prev_tokens: the last step's tokens, which join the sets at this step (None at step 0).
    rows None: one set of parameters for the call -- argmax, ops.sample_tokens or ops.repetition_penalty, the launches made before
    per-prompt parameters existed.  rows: dict(temperature, top_p, top_k, min_p) of device arrays with one value per PROMPT (temperature
    0: a greedy prompt) -> ops.sample_tokens_rows over the arrays' entries at row_ids, and with `logprobs` the tokens' log-probabilities."""
    def select(logits, step, prev_tokens, row_ids):
        if sets is not None and do_sample:
            pen = ops.repetition_penalty(logits, repetition_penalty, sets, row_ids=row_ids, prev_tokens=prev_tokens)
            return ops.sample_tokens(pen, temperature, top_p, top_k, seed, row_ids=row_ids, step=step), None
        if sets is not None:
            return ops.repetition_penalty(logits, repetition_penalty, sets, row_ids=row_ids, prev_tokens=prev_tokens, return_tokens=True), None
        if do_sample:
            return ops.sample_tokens(logits, temperature, top_p, top_k, seed, row_ids=row_ids, step=step), None
        return logits.argmax(-1), None

    if rows is None:
        return select
    n = rows["temperature"].shape[0]
    active = {"ids": None, "rows": rows}

    def select_rows(logits, step, prev_tokens, row_ids):
        if row_ids is not active["ids"]:                 # the eager loop hands over a new row_ids when prompts have left the batch
            active["ids"] = row_ids
            active["rows"] = rows if row_ids.shape[0] == n else {k: v.index_select(0, row_ids) for k, v in rows.items()}
        if sets is not None:
            logits = ops.repetition_penalty(logits, repetition_penalty, sets, row_ids=row_ids, prev_tokens=prev_tokens)
        out = ops.sample_tokens_rows(logits, seed=seed, row_ids=row_ids, step=step, return_logprobs=logprobs, **active["rows"])
        return out if logprobs else (out, None)
    return select_rows


def _per_prompt(name: str, value, n: int):
    """A packed_generate parameter given as one value or as a list / tuple with one value per prompt -> (n values, was a sequence)"""
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError(f"{name} holds {len(value)} values for {n} prompts")
        return list(value), True
    return [value] * n, False


def _prefill(model, lm, state: PagedState, p, bt):
    """The packed prompts through the LLM; each layer also appends its keys / values, token t into row prompt(t) of the block table bt
    at its position.  -> (logits [B, V] of each prompt's last token, step_pos [3, B]: the next token's M-RoPE position)"""
    emb, pos, cu, lengths, max_len = p["inputs_embeds"], p["position_ids"], p["cu_seqlens"], p["lengths"], p["max_len"]
    dev = emb.device
    state.mode = "prefill"
    state.tok_table = bt.index_select(0, _h2d([b for b, L in enumerate(lengths) for _ in range(L)], torch.int64, dev))
    state.tok_pos = _h2d([i for L in lengths for i in range(L)], torch.int32, dev)
    hidden = lm(inputs_embeds=emb[None], position_ids=pos[:, None, :], use_cache=False, cu_seq_lens_q=cu, cu_seq_lens_k=cu,
                max_length_q=max_len, max_length_k=max_len, vsel_paged=state).last_hidden_state[0]
    last = cu[1:].to(torch.int64) - 1
    logits = model.lm_head(hidden[last])
    state.tok_table = state.tok_pos = None
    return logits, pos[:, last] + 1


def _eager_decode(model, lm, state: PagedState, pages, lengths, logits, step_pos, seqlens, bt, max_new_tokens: int, eos, select, row_ids,
                  return_logits: bool):
    """The host-driven decode loop: every step is an eager forward over the active rows and the host reads the step's tokens.  logits,
    step_pos, seqlens, bt, select, row_ids as in _graph_decode; pages: each prompt's pages, which hold its `lengths` prompt keys.  A row
    that crosses a page boundary draws one page; a prompt that emits eos or reaches max_new_tokens leaves the batch and its pages go
    back to the pool at once (pages[b] is emptied).  -> (tokens, per-step logits or None, per-step log-probabilities or None)"""
    pool, dev, n = state.pool, logits.device, len(lengths)
    active = list(range(n))
    lens = list(lengths)
    tokens = [[] for _ in range(n)]
    step_logits = [[] for _ in range(n)]
    logprobs = [[] for _ in range(n)]
    embed = model.get_input_embeddings()
    prev = None
    state.mode = "decode"
    step = 0
    while True:
        nxt, lp = select(logits, step, prev, row_ids)
        host = nxt.tolist()                                       # the one host synchronisation of a step
        lp_host = None if lp is None else lp.tolist()
        keep = []
        for i, b in enumerate(active):
            if host[i] < 0:
                raise RuntimeError(f"sampling failed for prompt {b} at step {step}: {_INVALID_LOGITS}")
            tokens[b].append(host[i])
            if lp_host is not None:
                logprobs[b].append(lp_host[i])
            if return_logits:
                step_logits[b].append(logits[i])
            if host[i] in eos or len(tokens[b]) >= max_new_tokens:
                pool.release(pages[b])                            # the prompt leaves the batch
                pages[b] = []
            else:
                keep.append(i)
        if not keep:
            return tokens, step_logits if return_logits else None, logprobs if lp_host is not None else None
        if len(keep) < len(active):
            idx = _h2d(keep, torch.int64, dev)
            nxt, bt, step_pos, seqlens = nxt[idx], bt[idx], step_pos[:, idx], seqlens[idx]
            if row_ids is not None:
                row_ids = row_ids[idx]
            active = [active[i] for i in keep]
        for i, b in enumerate(active):                            # this step appends position lens[b]
            need = _cdiv(lens[b] + 1, pool.page_size)
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


def _graph_decode(model, lm, graphs: DecodeGraphs, logits, step_pos, seqlens, bt, max_new_tokens: int, lookahead: int, eos, select,
                  row_ids, return_logits: bool):
    """The device-resident decode loop.  logits [n, V]: the prefill's; step_pos [3, n], seqlens int32 [n], bt int32 [n, width]: the
    state of the first decode step; select, row_ids: _selector's, rows = prompts throughout.  Per step the host enqueues the
    selector, ops.decode_advance, a copy of its status into a pinned ring slot with an event, and the graph replay; before step s it
    reads the status of step s - lookahead.  Rows never leave the batch: decode_advance freezes a finished row, and later replays rewrite
    one cache slot of that row's own pages with the same values.  The selector's log-probabilities, when it returns them, go into column
    `step` of a [n, max_new_tokens] device buffer that is read once after the loop.
    -> (tokens, per-step logits or None, per-step log-probabilities or None)"""
    dev, n = logits.device, logits.shape[0]
    cur = torch.cuda.current_stream(dev)
    if graphs.stream is None:
        graphs.stream = torch.cuda.Stream(dev)
    s = graphs.stream
    s.wait_stream(cur)
    slots = lookahead + 1
    ring, events = graphs._ring(slots)
    kept_logits = []
    lp_buf = None

    def status_of(step: int) -> int:
        events[step % slots].synchronize()
        active, row, at, _ = ring[step % slots].tolist()
        if row >= 0:
            raise RuntimeError(f"sampling failed for prompt {row} at step {at}: {_INVALID_LOGITS}")
        return active

    try:
        with torch.cuda.stream(s):
            sg = graphs._step(n, step_pos.dtype, dev)
            sg.zeros.zero_()
            sg.pos.copy_(step_pos)
            sg.state.cache_seqlens.copy_(seqlens)
            sg.state.block_table.fill_(-1)
            sg.state.block_table[:, :bt.shape[1]].copy_(bt)
            eos_d = _h2d(sorted(eos), torch.int64, dev) if eos else None
            tokens_out = torch.zeros(n, max_new_tokens, dtype=torch.int64, device=dev)
            enqueued = checked = 0
            for step in range(max_new_tokens):
                if step >= lookahead:
                    checked = step - lookahead + 1
                    if status_of(step - lookahead) == 0:
                        break
                # every row starts at step 0 together, so the loop index is the step of every active row
                nxt, lp = select(logits, step, sg.feed if step else None, row_ids)
                if lp is not None:
                    if lp_buf is None:
                        lp_buf = torch.zeros(n, max_new_tokens, dtype=torch.float32, device=dev)
                    lp_buf[:, step].copy_(lp)
                if return_logits:
                    kept_logits.append(logits if step == 0 else logits.clone())
                ops.decode_advance(nxt, eos_d, max_new_tokens, sg.done, sg.n_tokens, sg.state.cache_seqlens, sg.pos, sg.feed, tokens_out,
                                   sg.status)
                ring[step % slots].copy_(sg.status, non_blocking=True)
                events[step % slots].record(s)
                enqueued = step + 1
                if step + 1 < max_new_tokens:      # (after the last step every row has stopped: nothing is replayed)
                    if sg.graph is None:
                        _capture(graphs, sg, model, lm)
                    sg.graph.replay()
                    logits = sg.logits
            for step in range(checked, enqueued):   # the steps not looked at yet: an invalid row among them still raises
                status_of(step)
            counts = sg.n_tokens.tolist()
            rows = tokens_out.tolist()
            lp_rows = None if lp_buf is None else lp_buf.tolist()
    finally:
        s.synchronize()                             # also on an exception: nothing in flight writes pages that go back to the free list
        cur.wait_stream(s)
    tokens = [rows[b][:counts[b]] for b in range(n)]
    step_logits = [[kept_logits[i][b] for i in range(counts[b])] for b in range(n)] if return_logits else None
    logprobs = None if lp_rows is None else [lp_rows[b][:counts[b]] for b in range(n)]
    return tokens, step_logits, logprobs


@torch.no_grad()
def packed_generate(model, input_ids: Sequence[torch.Tensor], pixel_values: torch.Tensor, image_grid_thw: torch.Tensor,
                    images_per_prompt: Sequence[int], max_new_tokens: int, budgets: float | None = None, eos_token_id=None,
                    page_size: int = 64, pool: PagedKVPool | None = None, return_logits: bool = False, do_sample: bool = False,
                    temperature: float = 1.0, top_p: float = 1.0, top_k: int = 0, seed: int = 0, repetition_penalty: float = 1.0,
                    graph=False, lookahead: int = DEFAULT_LOOKAHEAD, min_p: float = 0.0, return_logprobs: bool = False):
    """Greedy or sampled generation for a batch of image prompts (arguments as packed_prefill).
    -> dict(tokens: B lists of new token ids (each ends at eos or after max_new_tokens), kept [B], first_logits [B, vocab]
            (bit-identical to packed_prefill's logits), pool, and with return_logits: logits, B lists of [vocab] per step).
    Decode positions continue each prompt's M-RoPE positions from its last prompt token (+1 per step), which is what the batch-1
    Qwen2_5_VLForConditionalGeneration_Selector.generate() uses ("decode positions").
    pool: a PagedKVPool to draw pages from (default: one sized for this call); every page drawn is back on its free list on return.
    do_sample=False: the next token is the argmax of the logits.  do_sample=True: ops.sample_tokens with temperature, top_k (0: off),
    top_p and seed, as HF's do_sample with those warpers; the draw of prompt b at its s-th new token uses row id b and
    step s, so it does not depend on the other prompts or on when they leave the batch.  A prompt whose logits hold a NaN / +inf
    (or no finite value) raises RuntimeError.
    Per-prompt parameters: do_sample, temperature, top_p, top_k and min_p each take one value or a list / tuple with one value per prompt,
    so a call can mix greedy and sampled prompts and different temperatures.  min_p (0: off) is HF's MinPLogitsWarper, applied after top-k
    and top-p.  return_logprobs=True adds `logprobs`: B lists of floats aligned with `tokens`, the log-probability of each token under
    the distribution it was drawn from (a greedy prompt: the log-softmax of its logits); with a repetition penalty that is the
    distribution of the PENALISED logits.  A list, min_p != 0 or return_logprobs selects through ops.sample_tokens_rows (DESIGN.md §13,
    "per-row parameters"), a prompt with do_sample False as a temperature-0 row; every other call makes the launches it made before these
    arguments existed.
    graph=False: every decode step is an eager forward and the host reads the step's tokens.  graph=True, or a DecodeGraphs (which keeps
    the captured graph between calls and fixes the pool): the same tokens and logits from the device-resident loop of DESIGN.md §15 --
    every prompt holds all its pages from the start, finished prompts stay in the batch as frozen rows, and the host reads a status
    word `lookahead` (>= 1) steps behind the step it enqueues."""
    if max_new_tokens < 1:
        raise ValueError("max_new_tokens must be >= 1")
    if not isinstance(graph, (bool, DecodeGraphs)):
        raise TypeError(f"graph must be a bool or a DecodeGraphs, got {graph!r}")
    ops._int_in("lookahead", lookahead, 1)
    if isinstance(graph, DecodeGraphs):
        if graph.model is not model or (pool is not None and pool is not graph.pool):
            raise ValueError("this DecodeGraphs was built for another model / pool")
        pool = graph.pool
    n_prompts = len(input_ids)
    (ds, seq), (ts, seq_t), (ps, seq_p), (ks, seq_k), (mps, seq_m) = (_per_prompt(name, v, n_prompts) for name, v in (
        ("do_sample", do_sample), ("temperature", temperature), ("top_p", top_p), ("top_k", top_k), ("min_p", min_p)))
    for d in ds:
        if not isinstance(d, bool):
            raise TypeError(f"do_sample must be a bool or one bool per prompt, got {do_sample!r}")
    if not isinstance(return_logprobs, bool):
        raise TypeError(f"return_logprobs must be a bool, got {return_logprobs!r}")
    for b in range(n_prompts):                   # (a greedy prompt's sampling parameters are not looked at, as before)
        if ds[b]:
            ops.check_sampling_args(ts[b], ps[b], ks[b], seed)
            ops.check_row_sampling_args(min_p=mps[b])
    per_row = seq or seq_t or seq_p or seq_k or seq_m or return_logprobs or any(d and m != 0 for d, m in zip(ds, mps))
    if per_row:
        for b in range(n_prompts):
            if ds[b]:
                ops.check_row_sampling_args(ts[b], ps[b], ks[b], mps[b])
        ops._int_in("seed", seed, 0, 2 ** 64)
    penalize = ops.check_repetition_penalty(repetition_penalty) != 1.0
    eos = set() if eos_token_id is None else ({int(eos_token_id)} if isinstance(eos_token_id, int) else {int(e) for e in eos_token_id})
    lm = model.model.language_model
    # the token sets of the penalty: every prompt id as passed (range-checked on the host before any device work)
    sets = ops.token_sets(input_ids, model.lm_head.out_features, model.lm_head.weight.device) if penalize else None
    rows = None
    if per_row:
        # one device array per parameter, built once per call; a greedy prompt is a temperature-0 row with every filter off
        dev0 = model.lm_head.weight.device
        rows = dict(temperature=_h2d([float(t) if d else 0.0 for d, t in zip(ds, ts)], torch.float32, dev0),
                    top_p=_h2d([float(x) if d else 1.0 for d, x in zip(ds, ps)], torch.float32, dev0),
                    top_k=_h2d([k if d else 0 for d, k in zip(ds, ks)], torch.int32, dev0),
                    min_p=_h2d([float(x) if d else 0.0 for d, x in zip(ds, mps)], torch.float32, dev0))
    select = _selector(do_sample, temperature, top_p, top_k, seed, repetition_penalty, sets, rows, return_logprobs)
    register_paged_attention()
    p = _packed_inputs(model, input_ids, pixel_values, image_grid_thw, images_per_prompt, budgets)
    lengths = p["lengths"]
    dev, n = p["inputs_embeds"].device, len(lengths)
    hkv, hd = lm.config.num_key_value_heads, lm.layers[0].self_attn.head_dim
    # the last new token is never fed back: a prompt holds at most L + max_new_tokens - 1 keys
    most = [_cdiv(L + max_new_tokens - 1, page_size) for L in lengths]
    if pool is None:
        pool = PagedKVPool(len(lm.layers), sum(most), page_size, hkv, hd, dev)
    elif pool.page_size != page_size or pool.hkv != hkv or pool.head_dim != hd or len(pool.k) != len(lm.layers):
        raise ValueError("the pool's geometry does not match the model / page_size")
    width = max(most)
    graphs = graph if isinstance(graph, DecodeGraphs) else (DecodeGraphs(model, pool, width) if graph else None)
    if graphs is not None and width > graphs.max_pages_per_prompt:
        raise ValueError(f"a prompt needs {width} pages, this DecodeGraphs holds {graphs.max_pages_per_prompt} per prompt")
    pages = [[] for _ in range(n)]
    state = PagedState(pool)
    old_impl = lm.config._attn_implementation
    try:
        if graphs is not None:
            # all pages up front: the block table is constant for the call.  most[b] pages hold the L + max_new_tokens - 1 keys of a
            # prompt that runs to the limit; a row frozen on eos at token s <= max_new_tokens - 2 keeps cache_seqlens = L + s inside them
            drawn = pool.alloc(sum(most))
            for b, m in enumerate(most):
                pages[b], drawn = drawn[:m], drawn[m:]
                assert len(pages[b]) * page_size >= lengths[b] + max_new_tokens - 1
        else:
            for b, L in enumerate(lengths):
                pages[b] = pool.alloc(_cdiv(L, page_size))
        bt = _h2d([pg + [-1] * (width - len(pg)) for pg in pages], torch.int32, dev)
        lm.config._attn_implementation = ATTN_NAME_PAGED
        first_logits, step_pos = _prefill(model, lm, state, p, bt)
        seqlens = _h2d(lengths, torch.int32, dev)
        row_ids = torch.arange(n, dtype=torch.int64, device=dev) if per_row or do_sample or penalize else None
        if graphs is not None:
            tokens, step_logits, logprobs = _graph_decode(model, lm, graphs, first_logits, step_pos, seqlens, bt, max_new_tokens, lookahead, eos, select,
                                                row_ids, return_logits)
        else:
            tokens, step_logits, logprobs = _eager_decode(model, lm, state, pages, lengths, first_logits, step_pos, seqlens, bt, max_new_tokens, eos,
                                                select, row_ids, return_logits)
    finally:
        lm.config._attn_implementation = old_impl
        for pg in pages:
            pool.release(pg)
    out = {"tokens": tokens, "kept": p["kept"], "first_logits": first_logits, "pool": pool}
    if return_logits:
        out["logits"] = step_logits
    if return_logprobs:
        out["logprobs"] = logprobs
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
