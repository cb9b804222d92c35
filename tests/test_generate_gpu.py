"""packed_generate (batched greedy generation of compressed prompts on a paged KV cache) against packed_prefill and the batch-1
Qwen2_5_VLForConditionalGeneration_Selector.generate(), on the tiny selector model of
tests/test_hf_gpu.py::test_packed_prefill_matches_per_prompt_forward (head_dim 128), built by tests/generate_model.py."""
import pytest
import torch

import generate_model
from generate_model import IMG, _compare, _sub

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    return generate_model.build()


def test_first_step_logits_are_packed_prefill_bit_for_bit(setup):
    from visionselector_amd.generate import packed_generate
    from visionselector_amd.packed import packed_prefill
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    pre = packed_prefill(model, ids, pix, grids, ipp)
    gen = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=2)
    assert gen["kept"] == pre["kept"]
    assert torch.equal(gen["first_logits"], pre["logits"])
    assert [t[0] for t in gen["tokens"]] == pre["logits"].argmax(-1).tolist()


def test_tokens_and_logits_match_batch1_generate(setup):
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    gen = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, return_logits=True)
    compared = 0
    for b in range(3):
        one, p1, g1, _ = _sub(setup, [b])
        inp = dict(input_ids=one[0][None].cuda(), attention_mask=torch.ones_like(one[0])[None].cuda(), pixel_values=p1,
                   image_grid_thw=g1, mm_token_type_ids=(one[0] == IMG).int()[None].cuda())
        model.model.rope_deltas = None
        o = model.generate(**inp, max_new_tokens=8, do_sample=False, output_logits=True, return_dict_in_generate=True)
        ref = o.sequences[0, one[0].numel():].tolist()
        assert len(gen["tokens"][b]) == 8
        compared += _compare(gen["tokens"][b], ref, [lg[0] for lg in o.logits], gen["logits"][b])
    assert compared >= 3          # the comparison is not vacuous


def test_eos_leaves_the_batch_and_returns_pages(setup):
    from visionselector_amd.generate import PagedKVPool, packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    lm = model.model.language_model
    pool = PagedKVPool(len(lm.layers), 64, 16, lm.config.num_key_value_heads, 128, "cuda")
    base = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, page_size=16, pool=pool, return_logits=True)
    assert pool.n_free == 64
    # stop prompt 1 at the earliest step whose token no other prompt emits
    stop = next(((s, t) for s, t in enumerate(base["tokens"][1]) if s > 0 and t not in base["tokens"][1][:s] and all(t not in base["tokens"][b] for b in (0, 2))), None)
    assert stop is not None, base["tokens"]
    s, eos = stop
    gen = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, page_size=16, pool=pool, eos_token_id=[eos, 10 ** 6])
    assert gen["tokens"][1] == base["tokens"][1][:s + 1] and len(gen["tokens"][1]) == s + 1
    for b in (0, 2):      # (the batch shrank under them: other GEMM shapes, so the tie rule of the batch-1 comparison)
        assert len(gen["tokens"][b]) == 8
        _compare(gen["tokens"][b], base["tokens"][b], base["logits"][b])
    assert pool.n_free == 64


def test_prompt_alone_and_in_the_batch_agree(setup):
    from visionselector_amd.generate import packed_generate
    model = setup[0]
    ids, pix, grids, ipp = _sub(setup, [0, 1, 2])
    batch = packed_generate(model, ids, pix, grids, ipp, max_new_tokens=8, return_logits=True)
    for b in (0, 2):
        one, p1, g1, i1 = _sub(setup, [b])
        alone = packed_generate(model, one, p1, g1, i1, max_new_tokens=8, return_logits=True)
        _compare(batch["tokens"][b], alone["tokens"][0], alone["logits"][0], batch["logits"][b])
