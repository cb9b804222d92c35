"""packed_generate with per-prompt sampling parameters, min_p and return_logprobs on the tiny selector model of tests/generate_model.py:
the scalar path is untouched; in a batch that mixes a greedy prompt, two sampled ones and a min-p one every token (and its
log-probability, bit for bit) is ops.sample_tokens_rows of its own step's logits with that prompt's parameters, row id = prompt, step =
tokens generated before it -- in the eager and in the graph loop, also after a prompt has left the batch at eos."""
import pytest
import torch

import generate_model
from generate_model import _sub

pytestmark = pytest.mark.gpu

SEED = 4321
# prompt 0 greedy (its sampling values are never looked at), 1: T 0.7 / top_p 0.9, 2: T 1.2 / top_k 5, 3: T 1 / min_p 0.2
MIXED = dict(do_sample=[False, True, True, True], temperature=[1.0, 0.7, 1.2, 1.0], top_p=[1.0, 0.9, 1.0, 1.0], top_k=[0, 0, 5, 0],
             min_p=[0.0, 0.0, 0.0, 0.2])
SOLO = [dict(temperature=0.0), dict(temperature=0.7, top_p=0.9), dict(temperature=1.2, top_k=5), dict(temperature=1.0, min_p=0.2)]


@pytest.fixture(scope="module")
def setup():
    return generate_model.build()


@pytest.fixture(scope="module")
def runs(setup):
    """the mixed batch of 4 prompts (prompt 0 twice), eager and graph, with an eos that prompt 1 emits early: computed once"""
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2, 0])
    first = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, page_size=16, seed=SEED, **MIXED)
    eos = first["tokens"][1][2]
    out = {"first": first, "eos": eos}
    for graph in (False, True):
        out[graph] = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, page_size=16, seed=SEED, eos_token_id=eos,
                                     return_logits=True, return_logprobs=True, graph=graph, **MIXED)
    return out


def test_scalar_path_is_unchanged_by_the_new_keywords(setup):
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    for kw in (dict(), dict(do_sample=True, temperature=0.8, top_p=0.9, top_k=20, seed=1234)):
        base = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=6, **kw)
        same = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=6, min_p=0.0, return_logprobs=False, **kw)
        assert same["tokens"] == base["tokens"] and "logprobs" not in same
        assert torch.equal(same["first_logits"], base["first_logits"])
    # ... and a call whose lists all hold one value is the scalar call's tokens through the per-row entry
    lists = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=6, do_sample=[True] * 3, temperature=[0.8] * 3, top_p=[0.9] * 3,
                            top_k=[20] * 3, seed=1234)
    assert lists["tokens"] == base["tokens"]


@pytest.mark.parametrize("graph", [False, True])
def test_each_token_and_logprob_is_sample_tokens_rows_of_its_step(runs, graph):
    from visionselector_amd import ops
    gen = runs[graph]
    assert len(gen["tokens"][1]) <= 3 < 8 and gen["tokens"][1][-1] == runs["eos"]           # prompt 1 left; the others went on
    checked = 0
    for b in range(4):
        assert len(gen["tokens"][b]) == len(gen["logits"][b]) == len(gen["logprobs"][b])
        for s, t in enumerate(gen["tokens"][b]):
            lg = gen["logits"][b][s][None]
            rid = torch.tensor([b], device="cuda")
            tok, lp = ops.sample_tokens_rows(lg, seed=SEED, row_ids=rid, step=s, return_logprobs=True, **SOLO[b])
            assert t == tok.item(), (b, s)
            assert gen["logprobs"][b][s] == lp.item(), (b, s)              # the same fp32 value, bit for bit
            if b == 0:
                assert t == int(lg.argmax())
                ref = float(ops.token_logprobs(lg, tok)[0])
                assert abs(lp.item() - ref) <= 1e-6 + 2.0 ** -22 * abs(ref), (s, lp.item(), ref)
            elif b in (1, 2):                                                # no min-p: the scalar entry draws the same token
                kw = SOLO[b]
                assert t == ops.sample_tokens(lg, kw["temperature"], kw.get("top_p", 1.0), kw.get("top_k", 0), SEED, row_ids=rid,
                                              step=s).item(), (b, s)
            checked += 1
    assert checked > 8


def test_graph_and_eager_loops_agree(runs):
    assert runs[True]["tokens"] == runs[False]["tokens"]
    assert runs[True]["logprobs"] == runs[False]["logprobs"]
    # without eos the same prompts give the same first tokens: a prompt's stream does not depend on who leaves the batch
    for b in range(4):
        n = len(runs[False]["tokens"][b])
        assert runs["first"]["tokens"][b][:n] == runs[False]["tokens"][b]


def test_logprobs_with_a_repetition_penalty_are_of_the_penalised_logits(setup):
    from visionselector_amd import ops
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1])
    gen = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=4, do_sample=[False, True], temperature=0.9, seed=SEED,
                          repetition_penalty=1.3, return_logits=True, return_logprobs=True)
    sets = ops.token_sets(ids, model.lm_head.out_features, "cuda")
    for b in range(2):
        for s, t in enumerate(gen["tokens"][b]):
            rid = torch.tensor([b], device="cuda")
            prev = torch.tensor([gen["tokens"][b][s - 1]], device="cuda") if s else None
            pen = ops.repetition_penalty(gen["logits"][b][s][None], 1.3, sets, row_ids=rid, prev_tokens=prev)
            tok, lp = ops.sample_tokens_rows(pen, 0.9 if b else 0.0, seed=SEED, row_ids=rid, step=s, return_logprobs=True)
            assert (t, gen["logprobs"][b][s]) == (tok.item(), lp.item()), (b, s)
