"""packed_generate with do_sample on the tiny selector model of tests/generate_model.py: greedy stays
the default code path, sampled runs are repeatable, each token is ops.sample_tokens of its own step's logits at row id = prompt and
step = tokens generated before it (also after prompts have left the batch), top_k = 1 is greedy, pages return to the pool."""
import pytest
import torch

import generate_model
from generate_model import _sub

pytestmark = pytest.mark.gpu

SAMPLE = dict(temperature=0.8, top_p=0.9, top_k=20, seed=1234)


@pytest.fixture(scope="module")
def setup():
    return generate_model.build()


def test_do_sample_false_is_the_default_path(setup):
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    base = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=6)
    same = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=6, do_sample=False, **SAMPLE)
    assert same["tokens"] == base["tokens"]
    assert torch.equal(same["first_logits"], base["first_logits"])


def test_sampling_is_repeatable_and_seeded(setup):
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    a = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=12, do_sample=True, temperature=1.5, seed=7)
    b = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=12, do_sample=True, temperature=1.5, seed=7)
    c = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=12, do_sample=True, temperature=1.5, seed=8)
    assert a["tokens"] == b["tokens"]
    assert a["tokens"] != c["tokens"]


def test_each_token_is_sample_tokens_of_its_step(setup):
    """row id = the prompt's index, step = tokens generated so far -- also once a prompt has left the batch at eos"""
    from visionselector_amd import ops
    from visionselector_amd.generate import PagedKVPool, packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    lm = model.model.language_model
    pool = PagedKVPool(len(lm.layers), 64, 16, lm.config.num_key_value_heads, 128, "cuda")
    first = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, page_size=16, pool=pool, do_sample=True, **SAMPLE)
    eos = first["tokens"][1][2]                       # prompt 1 leaves at step <= 2; the others go on without it
    gen = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, page_size=16, pool=pool, eos_token_id=eos,
                          return_logits=True, do_sample=True, **SAMPLE)
    assert len(gen["tokens"][1]) <= 3 < 8
    assert pool.n_free == 64
    checked = 0
    for b in range(3):
        assert len(gen["tokens"][b]) == len(gen["logits"][b])
        for s, t in enumerate(gen["tokens"][b]):
            want = ops.sample_tokens(gen["logits"][b][s][None], SAMPLE["temperature"], SAMPLE["top_p"], SAMPLE["top_k"], SAMPLE["seed"],
                                     row_ids=torch.tensor([b], device="cuda"), step=s)
            assert t == want.item(), (b, s)
            checked += 1
    assert checked > 8


def test_top_k_1_is_greedy(setup):
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    gen = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, return_logits=True, do_sample=True, top_k=1, temperature=0.7,
                          seed=3)
    compared = 0
    for b in range(3):
        for s, t in enumerate(gen["tokens"][b]):
            lg = gen["logits"][b][s].float()
            top2 = lg.topk(2).values
            if top2[0] > top2[1]:
                assert t == int(lg.argmax()), (b, s)
                compared += 1
    assert compared >= 12


def test_invalid_parameters_refused_before_device_work(setup):
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0])
    for kw in (dict(temperature=0.0), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(seed=-1)):
        with pytest.raises(ValueError):
            packed_generate(model, ids, pix, grids, ipp, max_new_tokens=2, do_sample=True, **kw)
