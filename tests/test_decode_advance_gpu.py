"""vsel_decode_advance (ops.decode_advance) on the GPU against the numpy oracle tests/decode_advance_ref.py: exact, after
every launch of multi-step random runs, eager and replayed from a captured graph."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_advance_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("done", "n_tokens", "cache_seqlens", "pos", "feed", "tokens_out", "status")


def _device_state(st):
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in st.items()}


def _advance(dev, nxt, eos_d, max_new):
    from visionselector_amd import ops
    ops.decode_advance(nxt, eos_d, max_new, dev["done"], dev["n_tokens"], dev["cache_seqlens"], dev["pos"], dev["feed"], dev["tokens_out"],
                       dev["status"])


def _same(dev, st, where):
    for k in KEYS:
        got = dev[k].cpu().numpy()
        assert got.dtype == st[k].dtype and np.array_equal(got, st[k]), (where, k, got, st[k])


def _run(b, n_eos, max_new, seed, pos_dtype=np.int64, vocab=12):
    rng = np.random.default_rng(seed)
    st = R.new_state(rng.integers(1, 4000, b), rng.integers(0, 4000, (3, b)), max_new, pos_dtype)
    eos = rng.choice(vocab, n_eos, replace=False).tolist()
    st["start_seqlens"] = st["cache_seqlens"].copy()
    dev = _device_state(st)
    eos_d = torch.tensor(eos, dtype=torch.int64).cuda() if n_eos else None
    for step in range(max_new + 2):                                   # two launches past the point where every row has stopped
        nxt = rng.integers(0, vocab, b)
        nxt[rng.random(b) < 0.04] = -1                                # the sampler's "invalid logits"
        R.decode_advance(st, nxt, eos, max_new)
        _advance(dev, torch.from_numpy(nxt).cuda(), eos_d, max_new)
        _same(dev, st, (b, n_eos, step))
    assert st["status"][0] == 0 and (st["done"] != 0).all()
    return st


@pytest.mark.parametrize("b", [1, 3, 33, 300])
@pytest.mark.parametrize("n_eos", [0, 1, 5])
def test_decode_advance_matches_the_oracle_after_every_launch(b, n_eos):
    st = _run(b, n_eos, max_new=9, seed=100 * b + n_eos)
    if b == 300:                                                      # the run saw every way a row can stop
        assert set(st["done"].tolist()) == ({2, 3} if n_eos == 0 else {1, 2, 3})


def test_decode_advance_int32_positions():
    _run(33, 2, max_new=6, seed=7, pos_dtype=np.int32)


def test_decode_advance_max_new_tokens_1():
    st = _run(5, 1, max_new=1, seed=3)
    assert np.array_equal(st["cache_seqlens"], st["start_seqlens"])         # a first token never advances the cache


def test_decode_advance_is_graph_capturable():
    """Captured on one stream and replayed after `next` was rewritten on the device: state and status as the oracle's, launch by launch."""
    b, max_new, eos = 33, 7, [2, 5]
    rng = np.random.default_rng(11)
    st = R.new_state(rng.integers(1, 4000, b), rng.integers(0, 4000, (3, b)), max_new)
    dev = _device_state(st)
    eos_d = torch.tensor(eos, dtype=torch.int64).cuda()
    nxt_s = torch.zeros(b, dtype=torch.int64).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    first = rng.integers(0, 12, b)
    with torch.cuda.stream(s):
        nxt_s.copy_(torch.from_numpy(first).cuda())
        _advance(dev, nxt_s, eos_d, max_new)                          # warm-up: a real launch
    torch.cuda.synchronize()
    R.decode_advance(st, first, eos, max_new)
    _same(dev, st, "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        _advance(dev, nxt_s, eos_d, max_new)
    _same(dev, st, "capture executes nothing")
    for step in range(max_new + 1):
        nxt = rng.integers(0, 12, b)
        nxt[rng.random(b) < 0.05] = -1
        with torch.cuda.stream(s):
            nxt_s.copy_(torch.from_numpy(nxt).cuda())
            graph.replay()
        torch.cuda.synchronize()
        R.decode_advance(st, nxt, eos, max_new)
        _same(dev, st, ("replay", step))
    assert st["status"][0] == 0
