"""numpy oracle of vsel_decode_advance (csrc/decode_step.hip): the bookkeeping of one decode step, row by row.

State is a dict of numpy arrays, updated in place as the kernel updates its device tensors:
    done int32 [B] (0 active, 1 eos, 2 length, 3 invalid logits), n_tokens int32 [B], cache_seqlens int32 [B], pos [3, B],
    feed int64 [B], tokens_out int64 [B, max_new_tokens], status int32 [4].
Rules: a row with done != 0 on entry changes nothing.  An active row: n_tokens > 0 on entry -> cache_seqlens += 1 and pos += 1 (its
previous token went through the LLM step since the last advance).  Then t = next[b]: t < 0 -> done = 3 (nothing else written);
else tokens_out[b, n_tokens] = t, n_tokens += 1, and done = 1 if t is in eos, else done = 2 if n_tokens == max_new_tokens, else
feed[b] = t.  An active row whose n_tokens is outside [0, max_new_tokens) stops with done = 2 and nothing else.
status = {rows with done == 0 after the launch, lowest row that turned invalid in this launch or -1, that row's n_tokens or -1, 0}."""
import numpy as np


def new_state(cache_seqlens, pos, max_new_tokens, pos_dtype=np.int64):
    b = len(cache_seqlens)
    return dict(done=np.zeros(b, np.int32), n_tokens=np.zeros(b, np.int32), cache_seqlens=np.asarray(cache_seqlens, np.int32).copy(),
                pos=np.asarray(pos, pos_dtype).reshape(3, b).copy(), feed=np.zeros(b, np.int64),
                tokens_out=np.full((b, max_new_tokens), -7, np.int64), status=np.full(4, -9, np.int32))


def decode_advance(state, next_tokens, eos, max_new_tokens):
    """One launch.  next_tokens int64 [B]; eos: a sequence of ids (may be empty).  Updates `state` in place and returns it."""
    eos = {int(e) for e in eos}
    bad_row, bad_step = -1, -1
    for b in range(len(next_tokens)):
        if state["done"][b] != 0:
            continue
        n = int(state["n_tokens"][b])
        if n < 0 or n >= max_new_tokens:
            state["done"][b] = 2
            continue
        if n > 0:
            state["cache_seqlens"][b] += 1
            state["pos"][:, b] += 1
        t = int(next_tokens[b])
        if t < 0:
            state["done"][b] = 3
            if bad_row < 0:
                bad_row, bad_step = b, n
            continue
        state["tokens_out"][b, n] = t
        n += 1
        state["n_tokens"][b] = n
        if t in eos:
            state["done"][b] = 1
        elif n == max_new_tokens:
            state["done"][b] = 2
        else:
            state["feed"][b] = t
    state["status"][:] = (int((state["done"] == 0).sum()), bad_row, bad_step, 0)
    return state
