"""The tiny selector model of the packed_generate tests (tests/test_generate*_gpu.py), its three image prompts, and the helpers those tests
share: the model of tests/test_hf_gpu.py::test_packed_prefill_matches_per_prompt_forward (head_dim 128)."""
import torch

IMG, VID, VSTART, VEND = 10, 11, 12, 13
TOL = 3e-2           # of the logits' max: the packed pass and the per-prompt pass run different GEMM shapes in bf16


def build():
    """-> (model, prompts, grids, pixel_values, image_grid_thw): what the tests' `setup` module fixture returns"""
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


def _pool(model, n_pages, page_size=16):
    from visionselector_amd.generate import PagedKVPool
    lm = model.model.language_model
    return PagedKVPool(len(lm.layers), n_pages, page_size, lm.config.num_key_value_heads, 128, "cuda")


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
