"""packed_generate (batched greedy generation of compressed prompts on a paged KV cache) against packed_prefill and the batch-1
Qwen2_5_VLForConditionalGeneration_Selector.generate(), on the tiny selector model of
tests/test_hf_gpu.py::test_packed_prefill_matches_per_prompt_forward (head_dim 128), rebuilt here."""
import pytest
import torch

pytestmark = pytest.mark.gpu

IMG, VID, VSTART, VEND = 10, 11, 12, 13
TOL = 3e-2           # of the logits' max: the packed pass and the per-prompt pass run different GEMM shapes in bf16


@pytest.fixture(scope="module")
def setup():
    assert torch.cuda.is_available()
    from transformers import Qwen2_5_VLConfig
    from visionselector_amd.attention import ATTN_NAME_PACKED, replace_qwen2_vl_attention_class
    from visionselector_amd.hf_qwen25vl import Qwen2_5_VLForConditionalGeneration_Selector
    replace_qwen2_vl_attention_class()
    cfg = Qwen2_5_VLConfig(
        text_config=dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                         num_key_value_heads=1, vocab_size=64, max_position_embeddings=4096,
                         rope_parameters=dict(rope_type="default", mrope_section=[16, 24, 24], rope_theta=10000.0)),
        vision_config=dict(depth=2, hidden_size=64, num_heads=4, intermediate_size=128, out_hidden_size=256, patch_size=14,
                           spatial_merge_size=2, temporal_patch_size=2, window_size=112, fullatt_block_indexes=[1],
                           in_channels=3),
        image_token_id=IMG, video_token_id=VID, vision_start_token_id=VSTART, vision_end_token_id=VEND)
    torch.manual_seed(0)
    model = Qwen2_5_VLForConditionalGeneration_Selector(cfg).cuda().bfloat16().eval()
    model.model.language_model.config._attn_implementation = ATTN_NAME_PACKED
    model.model.visual.config._attn_implementation = "sdpa"                  # head_dim 16 tower
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in model.visual.importance_scorer.parameters():
            p.copy_((0.05 * torch.randn(p.shape, generator=g)).to(p.device))
    model.visual.budgets = 0.25
    g = torch.Generator().manual_seed(3)
    grids = [[(1, 16, 16)], [(1, 32, 16), (1, 8, 8)], [(1, 24, 24)]]          # prompt 1 holds two images
    prompts, pix, flat_grids = [], [], []
    for gl in grids:
        parts = [torch.randint(20, 60, (int(torch.randint(3, 9, (1,), generator=g)),), generator=g)]
        for (t, hh, ww) in gl:
            parts += [torch.tensor([VSTART]), torch.full((t * hh * ww // 4,), IMG), torch.tensor([VEND])]
            pix.append(torch.randn(t * hh * ww, 3 * 2 * 14 * 14, generator=g))
            flat_grids.append([t, hh, ww])
        parts.append(torch.randint(20, 60, (int(torch.randint(4, 12, (1,), generator=g)),), generator=g))
        prompts.append(torch.cat(parts))
    return model, prompts, grids, torch.cat(pix).bfloat16().cuda(), torch.tensor(flat_grids).cuda()


def _sub(setup, which):
    """prompts `which` of the batch with their images: (ids list, pixel_values, grids, images_per_prompt)"""
    _, prompts, grids, pix, grid_all = setup
    p0 = [0]
    for gl in grids:
        p0.append(p0[-1] + sum(t * h * w for t, h, w in gl))
    g0 = [0]
    for gl in grids:
        g0.append(g0[-1] + len(gl))
    return ([prompts[b] for b in which], torch.cat([pix[p0[b]:p0[b + 1]] for b in which]),
            torch.cat([grid_all[g0[b]:g0[b + 1]] for b in which]), [len(grids[b]) for b in which])


def _compare(tokens, ref_tokens, ref_logits, got_logits=None):
    """Equal tokens up to the first step where the reference's top-2 gap is within TOL (a tie; comparison stops there);
    logits within TOL of the max up to that step.  -> steps compared"""
    for s, r in enumerate(ref_tokens):
        lg = ref_logits[s].float()
        scale = max(1.0, float(lg.abs().max()))
        if got_logits is not None:
            assert float((got_logits[s].float() - lg).abs().max()) <= TOL * scale, s
        top2 = lg.topk(2).values
        if float(top2[0] - top2[1]) <= TOL * scale:
            return s
        assert s < len(tokens) and tokens[s] == r, (s, tokens, ref_tokens)
    return len(ref_tokens)


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
