"""CPU checks of the repetition penalty (vsel_token_sets_build, vsel_repetition_penalty, ops.token_sets / ops.repetition_penalty,
packed_generate's repetition_penalty keyword) and of generate.hf_generation_kwargs, which resolves HF generate() keyword arguments
with transformers' own merge: the argument checks run before any device work."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from visionselector_amd import _native as N
    from visionselector_amd import build
    build.build_native(verbose=False)
    return N.lib()


@pytest.mark.parametrize("name", ["vsel_token_sets_build", "vsel_repetition_penalty"])
def test_capi_declares_and_exports_penalty_symbols(lib, name):
    from visionselector_amd import _native
    text = open(os.path.join(ROOT, "include", "vsel.h")).read()
    assert re.search(rf"\b{name}\s*\(", text)
    assert name in _native.SIGNATURES
    assert hasattr(lib, name)


# (logits, dtype, batch, vocab, row_stride, penalty, sets, n_sets, tokens, out): a fake non-NULL device address where one is needed;
# every call below must fail in the host checks, before any HIP call
_OK = dict(logits=16, dtype=0, batch=2, vocab=100, row_stride=100, penalty=1.2, sets=16, n_sets=2, tokens=16, out=16)


@pytest.mark.parametrize("bad", [dict(penalty=0.0), dict(penalty=-1.05), dict(penalty=float("inf")), dict(penalty=float("nan")),
                                 dict(vocab=0), dict(batch=-1), dict(row_stride=99), dict(n_sets=-1), dict(logits=None),
                                 dict(sets=None), dict(tokens=None, out=None), dict(dtype=7)])
def test_repetition_penalty_argument_validation_without_gpu(lib, bad):
    a = dict(_OK, **bad)
    st = lib.vsel_repetition_penalty(None, a["logits"], a["dtype"], a["batch"], a["vocab"], a["row_stride"], a["penalty"], a["sets"],
                                     a["n_sets"], None, None, a["tokens"], a["out"])
    assert st == 1, lib.vsel_last_error()


def test_repetition_penalty_vocab_2_31_unsupported(lib):
    v = 2 ** 31
    assert lib.vsel_repetition_penalty(None, 16, 0, 2, v, v, 1.2, 16, 2, None, None, 16, None) == 4


def test_repetition_penalty_empty_batch_is_a_no_op(lib):
    assert lib.vsel_repetition_penalty(None, 16, 1, 0, 100, 100, 1.2, 16, 0, None, None, 16, None) == 0


@pytest.mark.parametrize("args,want", [((None, 16, 2, 100, 16), 1), ((16, None, 2, 100, 16), 1), ((16, 16, 2, 100, None), 1),
                                       ((16, 16, -1, 100, 16), 1), ((16, 16, 2, 0, 16), 1), ((16, 16, 2, 2 ** 31, 16), 4),
                                       ((16, 16, 0, 100, 16), 0)])
def test_token_sets_build_argument_validation_without_gpu(lib, args, want):
    assert lib.vsel_token_sets_build(None, *args) == want, lib.vsel_last_error()


def test_ops_refuse_cpu_tensors_and_bad_ids(lib):
    from visionselector_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.token_sets([torch.tensor([1, 2])], 10, "cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.repetition_penalty(torch.zeros(2, 10), 1.2, torch.zeros(2, 1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.repetition_penalty(torch.zeros(2, 10, dtype=torch.bfloat16), 1.2, torch.zeros(2, 1, dtype=torch.int32), return_tokens=True)
    # ids outside [0, vocab) are refused on the host, before the device is touched (here: there is none)
    for bad in ([0, 10], [-1], [3, 2 ** 40]):
        with pytest.raises(ValueError, match="ids must be in"):
            ops.token_sets([torch.tensor([1, 2]), torch.tensor(bad)], 10, "cuda")


@pytest.mark.parametrize("p", [0.0, -1.2, float("nan"), float("inf"), True, "1.2", None, 1e-50])
def test_check_repetition_penalty_refuses(p):
    from visionselector_amd import ops
    with pytest.raises(ValueError):
        ops.check_repetition_penalty(p)


def test_packed_generate_signature_has_repetition_penalty():
    from visionselector_amd.generate import packed_generate
    prm = inspect.signature(packed_generate).parameters["repetition_penalty"]
    assert prm.default == 1.0 and prm.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD


# ---- hf_generation_kwargs -------------------------------------------------------------------------------------------------------

@pytest.fixture()
def model():
    from transformers import Qwen2Config, Qwen2ForCausalLM
    torch.manual_seed(0)
    return Qwen2ForCausalLM(Qwen2Config(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2,
                                        num_key_value_heads=1, vocab_size=64))


def _hf(model, **kw):
    """what HF generate() itself resolves the same call to"""
    g, _ = model._prepare_generation_config(None, **kw)
    return g


def test_resolver_config_penalty_applies_to_greedy(model):
    from visionselector_amd.generate import hf_generation_kwargs
    model.generation_config.repetition_penalty = 1.05
    kw = hf_generation_kwargs(model, do_sample=False, max_new_tokens=8)
    assert kw["do_sample"] is False and kw["repetition_penalty"] == 1.05 and kw["max_new_tokens"] == 8
    assert set(kw) == {"do_sample", "temperature", "top_p", "top_k", "repetition_penalty", "eos_token_id", "max_new_tokens"}


def test_resolver_hf_default_top_k_is_50(model):
    from visionselector_amd.generate import hf_generation_kwargs
    kw = hf_generation_kwargs(model, do_sample=True, temperature=0.7, top_p=0.9, max_new_tokens=4)
    assert kw == dict(do_sample=True, temperature=0.7, top_p=0.9, top_k=50, repetition_penalty=1.0, eos_token_id=None, max_new_tokens=4)


def test_resolver_config_top_k(model):
    from visionselector_amd.generate import hf_generation_kwargs
    model.generation_config.top_k = 1
    assert hf_generation_kwargs(model, do_sample=True, max_new_tokens=4)["top_k"] == 1
    assert hf_generation_kwargs(model, do_sample=True, top_k=7, max_new_tokens=4)["top_k"] == 7       # the caller's wins


def test_resolver_caller_top_p_none_follows_hf(model):
    """The eval callers pass top_p=None (qwen-evaluation/predict.py's default).  transformers' merge lets every keyword the caller passes
    override the checkpoint's config, None included, and HF then applies no top-p filter: the resolver gives what HF's merge gives."""
    from visionselector_amd.generate import hf_generation_kwargs
    model.generation_config.top_p = 0.8
    assert hf_generation_kwargs(model, do_sample=True, max_new_tokens=4)["top_p"] == 0.8             # not passed: the config's value
    assert _hf(model, do_sample=True, top_p=None, max_new_tokens=4).top_p is None
    assert hf_generation_kwargs(model, do_sample=True, top_p=None, max_new_tokens=4)["top_p"] == 1.0  # HF's off


def test_resolver_eos_from_config(model):
    from visionselector_amd.generate import hf_generation_kwargs
    model.generation_config.eos_token_id = [3, 5]
    assert hf_generation_kwargs(model, max_new_tokens=4)["eos_token_id"] == [3, 5]
    assert hf_generation_kwargs(model, max_new_tokens=4, eos_token_id=9)["eos_token_id"] == 9


@pytest.mark.parametrize("kw,name", [
    (dict(num_beams=2), "num_beams"), (dict(do_sample=True, min_p=0.1), "min_p"), (dict(do_sample=True, typical_p=0.9), "typical_p"),
    (dict(no_repeat_ngram_size=3), "no_repeat_ngram_size"), (dict(bad_words_ids=[[5]]), "bad_words_ids"),
    (dict(suppress_tokens=[1]), "suppress_tokens"), (dict(begin_suppress_tokens=[1]), "begin_suppress_tokens"),
    (dict(sequence_bias={(5,): 1.0}), "sequence_bias"), (dict(min_new_tokens=2), "min_new_tokens"), (dict(min_length=3), "min_length"),
    (dict(do_sample=True, epsilon_cutoff=3e-4), "epsilon_cutoff"), (dict(do_sample=True, eta_cutoff=3e-4), "eta_cutoff"),
    (dict(guidance_scale=1.5), "guidance_scale"), (dict(forced_bos_token_id=1), "forced_bos_token_id"),
    (dict(forced_eos_token_id=2), "forced_eos_token_id"), (dict(exponential_decay_length_penalty=(2, 1.1)), "exponential_decay_length_penalty"),
    (dict(renormalize_logits=True), "renormalize_logits"), (dict(max_length=30), "max_length"),
])
def test_resolver_refuses_unsupported_options(model, kw, name):
    from visionselector_amd.generate import hf_generation_kwargs
    if name != "max_length":
        kw = dict(kw, max_new_tokens=4)
    with pytest.raises(NotImplementedError, match=name):
        hf_generation_kwargs(model, **kw)


def test_resolver_refuses_non_generation_keywords(model):
    from visionselector_amd.generate import hf_generation_kwargs
    with pytest.raises(TypeError, match="seed"):
        hf_generation_kwargs(model, max_new_tokens=4, seed=3)
