"""What tools/bench_generate.py, bench_sample.py and bench_penalty.py share: the Qwen2.5-VL-7B-geometry selector model with random bf16
weights (built as tools/bench_e2e.py builds it) and its prompts of 2304 visual + 64 text tokens, the JSON line stamped with the box and
the commit (VSEL_COMMIT, since the tree may travel without its .git), and the device-event timer."""
import json
import os
import socket

import torch


def _stamp(rec):
    rec.update(box=f"{socket.gethostname()} / {torch.cuda.get_device_name(0)}", commit=os.environ.get("VSEL_COMMIT", "unknown"))
    print(json.dumps(rec), flush=True)


def _time_us(fn, iters=50, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


IMG, VID, VSTART, VEND = 151655, 151656, 151652, 151653


def model_and_prompts(n_prompts):
    """-> (model, prompts, pixel rows per prompt, the one image grid, visual tokens, text tokens)"""
    from transformers import Qwen2_5_VLConfig
    from visionselector_amd.attention import ATTN_NAME, ATTN_NAME_PACKED, replace_qwen2_vl_attention_class
    from visionselector_amd.hf_qwen25vl import Qwen2_5_VLForConditionalGeneration_Selector
    replace_qwen2_vl_attention_class()
    cfg = Qwen2_5_VLConfig(
        text_config=dict(hidden_size=3584, intermediate_size=18944, num_hidden_layers=28, num_attention_heads=28,
                         num_key_value_heads=4, vocab_size=152064, max_position_embeddings=32768,
                         rope_parameters=dict(rope_type="default", mrope_section=[16, 24, 24], rope_theta=1000000.0)),
        vision_config=dict(depth=32, hidden_size=1280, num_heads=16, intermediate_size=3420, out_hidden_size=3584, patch_size=14,
                           spatial_merge_size=2, temporal_patch_size=2, window_size=112, fullatt_block_indexes=[7, 15, 23, 31],
                           in_channels=3),
        image_token_id=IMG, video_token_id=VID, vision_start_token_id=VSTART, vision_end_token_id=VEND)
    torch.manual_seed(0)
    torch.set_default_dtype(torch.bfloat16)
    with torch.device("cuda"):
        model = Qwen2_5_VLForConditionalGeneration_Selector(cfg).eval()
    torch.set_default_dtype(torch.float32)
    model.model.language_model.config._attn_implementation = ATTN_NAME
    model.model.visual.config._attn_implementation = ATTN_NAME_PACKED
    with torch.no_grad():
        for p in model.visual.importance_scorer.parameters():
            p.copy_(0.02 * torch.randn_like(p))
    model.visual.budgets = 0.2
    grid, n_vis, n_text = (1, 96, 96), 96 * 96 // 4, 64
    g = torch.Generator().manual_seed(1)
    prompts, pix = [], []
    for _ in range(n_prompts):
        pre = torch.randint(1000, 5000, (n_text // 2,), generator=g)
        post = torch.randint(1000, 5000, (n_text - n_text // 2 - 2,), generator=g)
        prompts.append(torch.cat((pre, torch.tensor([VSTART]), torch.full((n_vis,), IMG), torch.tensor([VEND]), post)))
        pix.append(torch.randn(96 * 96, 3 * 2 * 14 * 14, generator=g).bfloat16())
    grid_t = torch.tensor([list(grid)]).cuda()
    return model, prompts, pix, grid_t, n_vis, n_text
