"""CPU checks of flash_attn_with_kvcache (flash-attn 2.7.4's decode entry point on vsel_kvcache_attn_fwd): its signature, the
drop-in import path, the options it refuses before any device work, and the C-ABI declaration."""
import inspect
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# flash_attn/flash_attn_interface.py of flash-attn 2.7.4: parameter names and defaults, in order
FA274_KVCACHE = [("q", inspect.Parameter.empty), ("k_cache", inspect.Parameter.empty), ("v_cache", inspect.Parameter.empty),
                 ("k", None), ("v", None), ("rotary_cos", None), ("rotary_sin", None), ("cache_seqlens", None),
                 ("cache_batch_idx", None), ("cache_leftpad", None), ("block_table", None), ("softmax_scale", None),
                 ("causal", False), ("window_size", (-1, -1)), ("softcap", 0.0), ("rotary_interleaved", True),
                 ("alibi_slopes", None), ("num_splits", 0), ("return_softmax_lse", False)]


def test_signature_matches_flash_attn_274():
    from visionselector_amd.flash_attn_compat import flash_attn_with_kvcache
    params = list(inspect.signature(flash_attn_with_kvcache).parameters.values())
    assert [(p.name, p.default) for p in params] == FA274_KVCACHE
    assert all(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params)


def test_dropin_import_path_resolves():
    from visionselector_amd.flash_attn_compat import flash_attn_with_kvcache as ours
    sys.path.insert(0, os.path.join(ROOT, "visionselector_amd", "dropin"))
    try:
        for m in [k for k in sys.modules if k == "flash_attn" or k.startswith("flash_attn.")]:
            del sys.modules[m]
        from flash_attn import flash_attn_with_kvcache
        from flash_attn.flash_attn_interface import flash_attn_with_kvcache as f2
    finally:
        sys.path.pop(0)
        for m in [k for k in sys.modules if k == "flash_attn" or k.startswith("flash_attn.")]:
            del sys.modules[m]
    assert flash_attn_with_kvcache is ours and f2 is ours


def _cpu_case(dtype=torch.bfloat16, d=128, hq=4, hkv=2, paged=False):
    q = torch.zeros(2, 1, hq, d, dtype=dtype)
    cache = torch.zeros(8, 16, hkv, d, dtype=dtype) if paged else torch.zeros(2, 64, hkv, d, dtype=dtype)
    kw = dict(block_table=torch.zeros(2, 4, dtype=torch.int32)) if paged else {}
    return q, cache, cache.clone(), kw


@pytest.mark.parametrize("opt,exc", [(dict(window_size=(8, 0)), NotImplementedError), (dict(window_size=(-1, 0)), NotImplementedError),
                                     (dict(softcap=30.0), NotImplementedError),
                                     (dict(alibi_slopes=torch.zeros(4)), NotImplementedError)])
def test_refused_options(opt, exc):
    from visionselector_amd.flash_attn_compat import flash_attn_with_kvcache
    q, kc, vc, _ = _cpu_case()
    with pytest.raises(exc):
        flash_attn_with_kvcache(q, kc, vc, cache_seqlens=3, **opt)


@pytest.mark.parametrize("extra", ["cache_leftpad", "cache_batch_idx"])
def test_paged_cache_refuses_leftpad_and_batch_idx(extra):
    from visionselector_amd.flash_attn_compat import flash_attn_with_kvcache
    q, kc, vc, kw = _cpu_case(paged=True)
    with pytest.raises(NotImplementedError, match="paged"):
        flash_attn_with_kvcache(q, kc, vc, cache_seqlens=3, **kw, **{extra: torch.zeros(2, dtype=torch.int32)})


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_non_bf16_is_a_type_error(dtype):
    from visionselector_amd.flash_attn_compat import flash_attn_with_kvcache
    q, kc, vc, _ = _cpu_case(dtype=dtype)
    with pytest.raises(TypeError):
        flash_attn_with_kvcache(q, kc, vc, cache_seqlens=3)
    q, kc, vc, _ = _cpu_case()
    k = torch.zeros(2, 1, 2, 128, dtype=dtype)
    with pytest.raises(TypeError):
        flash_attn_with_kvcache(q, kc, vc, k=k, v=k, cache_seqlens=3)


@pytest.mark.parametrize("d", [32, 96, 256])
def test_unsupported_head_dim(d):
    from visionselector_amd.flash_attn_compat import flash_attn_with_kvcache
    q, kc, vc, _ = _cpu_case(d=d)
    with pytest.raises(NotImplementedError, match="head_dim"):
        flash_attn_with_kvcache(q, kc, vc, cache_seqlens=3)


def test_cpu_tensors_do_not_fall_back():
    """Valid options on CPU tensors reach the op, which refuses to run anywhere but the GPU."""
    from visionselector_amd.flash_attn_compat import flash_attn_with_kvcache
    q, kc, vc, _ = _cpu_case()
    with pytest.raises(RuntimeError, match="GPU only"):
        flash_attn_with_kvcache(q, kc, vc, cache_seqlens=3, num_splits=4)


def test_capi_declares_the_entry_point():
    from visionselector_amd import _native
    text = open(os.path.join(ROOT, "include", "vsel.h")).read()
    for name in ("vsel_kvcache_attn_fwd", "vsel_kvcache_attn_workspace_bytes"):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _native.SIGNATURES
