"""packed_generate(graph=...) -- the LLM decode step replayed from a captured graph, the token bookkeeping done by vsel_decode_advance,
the host reading a status word `lookahead` steps behind -- against the eager loop (graph=False), which runs the same
kernels on the same inputs at the same shapes, and against the batch-1 Qwen2_5_VLForConditionalGeneration_Selector.generate().  The tiny
selector model of tests/generate_model.py."""
import pytest
import torch

import generate_model
from generate_model import IMG, _compare, _pool, _sub

pytestmark = pytest.mark.gpu

MODES = {
    "greedy": dict(),
    "sampled": dict(do_sample=True, temperature=0.7, top_p=0.9, top_k=50, seed=11),
    "penalty": dict(repetition_penalty=1.05),
    "penalty_sampled": dict(repetition_penalty=1.05, do_sample=True, temperature=0.7, top_p=0.9, top_k=50, seed=11),
}


@pytest.fixture(scope="module")
def setup():
    return generate_model.build()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_graph_equals_eager_bit_for_bit(setup, mode):
    """No eos, B = 3, 8 new tokens: the same shapes run the same kernels on the same inputs -> tokens and per-step logits are equal."""
    from visionselector_amd.generate import packed_generate
    from visionselector_amd.packed import packed_prefill
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    eager = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, return_logits=True, **MODES[mode])
    graph = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, return_logits=True, graph=True, **MODES[mode])
    print(mode, "eager", eager["tokens"], "graph", graph["tokens"])
    assert graph["tokens"] == eager["tokens"] and all(len(t) == 8 for t in graph["tokens"])
    assert torch.equal(graph["first_logits"], packed_prefill(model, ids, pix, grids, ipp)["logits"])
    assert graph["kept"] == eager["kept"]
    for b in range(3):
        assert len(graph["logits"][b]) == 8
        for s in range(8):
            assert torch.equal(graph["logits"][b][s], eager["logits"][b][s]), (b, s)
    assert float(torch.stack(graph["logits"][0]).float().abs().max()) > 0


@pytest.mark.parametrize("mode", ["greedy", "penalty_sampled"])
def test_graph_eos_truncates_one_row_and_leaves_the_others_alone(setup, mode):
    """Rows are independent at constant B: the run with an eos only prompt 1 emits equals the run without it, cut after that token."""
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    pool = _pool(model, 64)
    base = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, page_size=16, pool=pool, graph=True, **MODES[mode])
    assert pool.n_free == 64
    # stop prompt 1 at the earliest step whose token no other prompt emits
    stop = next(((s, t) for s, t in enumerate(base["tokens"][1]) if s > 0 and t not in base["tokens"][1][:s] and all(t not in base["tokens"][b] for b in (0, 2))), None)
    assert stop is not None, base["tokens"]
    s, eos = stop
    gen = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, page_size=16, pool=pool, eos_token_id=[eos, 10 ** 6], graph=True,
                          return_logits=True, **MODES[mode])
    assert gen["tokens"][1] == base["tokens"][1][:s + 1] and len(gen["logits"][1]) == s + 1
    for b in (0, 2):
        assert gen["tokens"][b] == base["tokens"][b] and len(gen["tokens"][b]) == 8 and len(gen["logits"][b]) == 8
    assert pool.n_free == 64


def test_graph_lookahead_does_not_change_the_tokens(setup):
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    base = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, **MODES["sampled"])
    eos = base["tokens"][2][3]                                            # some rows stop early, so look-ahead steps are wasted
    want = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, eos_token_id=eos, graph=True, **MODES["sampled"])["tokens"]
    assert len(want[2]) <= 4
    for la in (1, 3, 8):
        got = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, eos_token_id=eos, graph=True, lookahead=la, **MODES["sampled"])
        assert got["tokens"] == want, la


def _lengths(setup, which, kept):
    return [int(setup[1][b].numel() - (setup[1][b] == IMG).sum()) + k for b, k in zip(which, kept)]


def test_graph_pool_pages_budget_and_exhaustion(setup):
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    kept = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=1)["kept"]
    lengths = _lengths(setup, [0, 1, 2], kept)
    # prompt 0's keys, L + max_new_tokens - 1, end exactly on a page boundary
    max_new = (-(lengths[0] - 1)) % 16
    max_new += 16 if max_new < 2 else 0
    assert (lengths[0] + max_new - 1) % 16 == 0
    need = sum(-(-(L + max_new - 1) // 16) for L in lengths)
    eager = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=max_new, page_size=16)
    pool = _pool(model, need)                                             # exactly the budget
    gen = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=max_new, page_size=16, pool=pool, graph=True)
    assert gen["tokens"] == eager["tokens"] and all(len(t) == max_new for t in gen["tokens"])
    assert pool.n_free == need
    short = _pool(model, need - 1)
    with pytest.raises(RuntimeError, match="pool exhausted"):
        packed_generate(model, ids, pix, grids, ipp, max_new_tokens=max_new, page_size=16, pool=short, graph=True)
    assert short.n_free == need - 1


def test_decode_graphs_are_reused_between_calls(setup):
    from visionselector_amd.generate import DecodeGraphs, packed_generate
    model = setup[0]
    pool = _pool(model, 64)
    graphs = DecodeGraphs(model, pool, max_pages_per_prompt=24)
    assert graphs.captures == 0
    a_in, b_in = _sub(setup, [0, 1]), _sub(setup, [2, 1])
    a = packed_generate(model, *a_in, max_new_tokens=8, page_size=16, graph=graphs, **MODES["penalty"])
    assert graphs.captures == 1 and graphs.capture_ms > 0 and pool.n_free == 64
    b = packed_generate(model, *b_in, max_new_tokens=8, page_size=16, graph=graphs, return_logits=True, **MODES["penalty"])
    assert graphs.captures == 1 and pool.n_free == 64                   # the same batch size: no second capture
    fresh = packed_generate(model, *b_in, max_new_tokens=8, page_size=16, graph=True, return_logits=True, **MODES["penalty"])
    assert b["tokens"] == fresh["tokens"] and b["tokens"] != a["tokens"]
    for r in range(2):
        for s in range(8):
            assert torch.equal(b["logits"][r][s], fresh["logits"][r][s]), (r, s)
    packed_generate(model, *_sub(setup, [0]), max_new_tokens=4, page_size=16, graph=graphs)
    assert graphs.captures == 2                                           # another batch size: its own graph
    with pytest.raises(ValueError, match="another model / pool"):
        packed_generate(model, *a_in, max_new_tokens=4, page_size=16, pool=_pool(model, 64), graph=graphs)
    with pytest.raises(ValueError, match="pages"):
        packed_generate(model, *a_in, max_new_tokens=400, page_size=16, graph=graphs)
    assert pool.n_free == 64


def test_graph_batch1_matches_hf_generate(setup):
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    compared = 0
    for b in range(3):
        one, p1, g1, i1 = _sub(setup, [b])
        gen = packed_generate(model, one, p1, g1, i1, max_new_tokens=8, return_logits=True, graph=True)
        inp = dict(input_ids=one[0][None].cuda(), attention_mask=torch.ones_like(one[0])[None].cuda(), pixel_values=p1,
                   image_grid_thw=g1, mm_token_type_ids=(one[0] == IMG).int()[None].cuda())
        model.model.rope_deltas = None
        o = model.generate(**inp, max_new_tokens=8, do_sample=False, output_logits=True, return_dict_in_generate=True)
        ref = o.sequences[0, one[0].numel():].tolist()
        assert len(gen["tokens"][0]) == 8
        compared += _compare(gen["tokens"][0], ref, [lg[0] for lg in o.logits], gen["logits"][0])
    assert compared >= 3          # the comparison is not vacuous


def test_graph_invalid_logits_raise_and_return_the_pages(setup):
    """A NaN in one lm_head row makes every prompt's logits invalid for the sampler: the status word carries the lowest row and its step."""
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    pool = _pool(model, 64)
    w = model.lm_head.weight
    saved = w[5].clone()
    try:
        with torch.no_grad():
            w[5] = float("nan")
        with pytest.raises(RuntimeError, match="sampling failed for prompt 0 at step 0"):
            packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, page_size=16, pool=pool, graph=True, **MODES["sampled"])
    finally:
        with torch.no_grad():
            w[5] = saved
    assert pool.n_free == 64
    ok = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=4, page_size=16, pool=pool, graph=True, **MODES["sampled"])
    assert all(len(t) == 4 for t in ok["tokens"]) and pool.n_free == 64
