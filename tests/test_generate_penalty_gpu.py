"""packed_generate with repetition_penalty on the tiny selector model of tests/generate_model.py: greedy tokens
against the batch-1 HF generate() with the same penalty (the tie rule of test_generate_gpu.py on HF's processed scores), the token sets
built from the prompts as passed (image ids the selector dropped included), sampled tokens as ops.sample_tokens of HF's processed
logits, 1.0 as the path without the penalty, hf_generation_kwargs driving packed_generate from the model's generation_config, and every
page back on the pool."""
import pytest
import torch

import generate_model
from generate_model import IMG, VEND, VSTART, _compare, _sub

pytestmark = pytest.mark.gpu

SAMPLE = dict(temperature=0.8, top_p=0.9, top_k=20, seed=1234)


@pytest.fixture(scope="module")
def setup():
    return generate_model.build()


def _hf_batch1(model, setup, b, **kw):
    one, p1, g1, _ = _sub(setup, [b])
    inp = dict(input_ids=one[0][None].cuda(), attention_mask=torch.ones_like(one[0])[None].cuda(), pixel_values=p1,
               image_grid_thw=g1, mm_token_type_ids=(one[0] == IMG).int()[None].cuda())
    model.model.rope_deltas = None
    o = model.generate(**inp, max_new_tokens=8, output_scores=True, output_logits=True, return_dict_in_generate=True, **kw)
    return o.sequences[0, one[0].numel():].tolist(), [s[0] for s in o.scores]


def _processed(ids, logits, theta):
    """HF's processor on one row of logits, given the ids before it"""
    from transformers import RepetitionPenaltyLogitsProcessor
    return RepetitionPenaltyLogitsProcessor(penalty=float(theta))(torch.as_tensor(ids, device="cuda")[None], logits.float()[None])[0]


def test_greedy_matches_batch1_generate_with_penalty(setup):
    from visionselector_amd.generate import PagedKVPool, packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    lm = model.model.language_model
    pool = PagedKVPool(len(lm.layers), 64, 16, lm.config.num_key_value_heads, 128, "cuda")
    gen = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, page_size=16, pool=pool, repetition_penalty=1.3,
                          return_logits=True)
    assert pool.n_free == 64
    plain = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8)
    assert gen["tokens"] != plain["tokens"]                       # the penalty changes what is generated: the comparison is not vacuous
    compared = 0
    for b in range(3):
        ref, scores = _hf_batch1(model, setup, b, do_sample=False, repetition_penalty=1.3)
        assert len(gen["tokens"][b]) == 8
        compared += _compare(gen["tokens"][b], ref, scores)
        # the processed logits of our own steps, from our raw logits and tokens, pick our tokens
        for s, t in enumerate(gen["tokens"][b]):
            y = _processed(ids[b].tolist() + gen["tokens"][b][:s], gen["logits"][b][s], 1.3)
            assert t == int(y.argmax()), (b, s)
    assert compared >= 3


def test_sets_hold_the_prompts_as_passed(setup, monkeypatch):
    """The sets come from the uncompressed ids: every image-pad id (also of the visual tokens the selector dropped) and the
    vision start / end ids are in, as in HF generate(), which keeps the full input_ids while the selector compresses inside forward."""
    from visionselector_amd import ops
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    seen = []
    real = ops.token_sets

    def spy(ids_list, vocab, device):
        sets = real(ids_list, vocab, device)
        seen.append(([torch.as_tensor(x).tolist() for x in ids_list], sets.clone()))
        return sets

    monkeypatch.setattr(ops, "token_sets", spy)
    gen = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=2, repetition_penalty=1.3)
    assert len(seen) == 1
    passed, sets = seen[0]
    assert passed == [x.tolist() for x in ids]
    words = sets.cpu().view(torch.uint8).numpy()
    for b in range(3):
        n_img = int((ids[b] == IMG).sum())
        assert gen["kept"][b] < n_img                              # the selector dropped image tokens of this prompt
        bits = {k for k in range(words.shape[1] * 8) if (words[b, k >> 3] >> (k & 7)) & 1}
        assert bits == set(ids[b].tolist()) and {IMG, VSTART, VEND} <= bits


def test_sampled_tokens_are_sample_tokens_of_processed_logits(setup):
    from visionselector_amd import ops
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    first = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, do_sample=True, repetition_penalty=1.2, **SAMPLE)
    eos = first["tokens"][1][2]                                     # prompt 1 leaves at step <= 2; the rows are compacted under the others
    gen = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, eos_token_id=eos, return_logits=True, do_sample=True,
                          repetition_penalty=1.2, **SAMPLE)
    assert len(gen["tokens"][1]) <= 3
    checked = 0
    for b in range(3):
        for s, t in enumerate(gen["tokens"][b]):
            y = _processed(ids[b].tolist() + gen["tokens"][b][:s], gen["logits"][b][s], 1.2)
            want = ops.sample_tokens(y[None], SAMPLE["temperature"], SAMPLE["top_p"], SAMPLE["top_k"], SAMPLE["seed"],
                                     row_ids=torch.tensor([b], device="cuda"), step=s)
            assert t == want.item(), (b, s)
            checked += 1
    assert checked > 8


@pytest.mark.parametrize("kw", [dict(), dict(do_sample=True, **SAMPLE)])
def test_penalty_one_is_the_path_without_it(setup, kw):
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    base = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=6, return_logits=True, **kw)
    same = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=6, return_logits=True, repetition_penalty=1.0, **kw)
    assert same["tokens"] == base["tokens"]
    assert torch.equal(same["first_logits"], base["first_logits"])
    for b in range(3):
        assert all(torch.equal(x, y) for x, y in zip(same["logits"][b], base["logits"][b]))


def test_hf_generation_kwargs_drives_packed_generate(setup):
    from visionselector_amd.generate import PagedKVPool, hf_generation_kwargs, packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    old = model.generation_config.repetition_penalty
    model.generation_config.repetition_penalty = 1.3
    try:
        kw = hf_generation_kwargs(model, do_sample=False, max_new_tokens=8)
        assert kw["repetition_penalty"] == 1.3 and kw["do_sample"] is False and kw["max_new_tokens"] == 8
        lm = model.model.language_model
        pool = PagedKVPool(len(lm.layers), 64, 16, lm.config.num_key_value_heads, 128, "cuda")
        gen = packed_generate(model, ids, pix, grids, ipp, page_size=16, pool=pool, **kw)
        assert pool.n_free == 64
        compared = 0
        for b in range(3):
            ref, scores = _hf_batch1(model, setup, b, do_sample=False)          # the penalty comes from generation_config
            compared += _compare(gen["tokens"][b], ref, scores)
        assert compared >= 3
    finally:
        model.generation_config.repetition_penalty = old


def test_invalid_penalty_refused_before_device_work(setup):
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0])
    for p in (0.0, -1.2, float("nan"), float("inf"), True):
        with pytest.raises(ValueError):
            packed_generate(model, ids, pix, grids, ipp, max_new_tokens=2, repetition_penalty=p)
    with pytest.raises(ValueError, match="ids must be in"):
        packed_generate(model, [torch.cat((ids[0], torch.tensor([10 ** 6])))], pix, grids, ipp, max_new_tokens=2, repetition_penalty=1.2)
