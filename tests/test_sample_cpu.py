"""CPU checks of top-k / top-p sampling (vsel_sample_tokens, ops.sample_tokens, packed_generate's sampling keywords): the oracle's
Philox against the Random123 known-answer vectors, the oracle's kept set against the installed transformers warper chain, and the
argument checks that run before any device work."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as R  # noqa: E402


@pytest.mark.parametrize("ctr,key,want", [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
])
def test_oracle_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert [int(w) for w in got] == want


def test_oracle_uniforms_are_open_interval():
    u = R.uniforms(100_003, seed=7, row_id=3, step=2 ** 33 + 5)
    assert u.min() > 0 and u.max() < 1 and abs(u.mean() - 0.5) < 0.01


def _hf_survivors(x, temperature, top_p, top_k):
    from transformers import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = torch.from_numpy(x)[None].clone()
    ids = torch.zeros(1, 1, dtype=torch.long)
    s = TemperatureLogitsWarper(temperature)(ids, s)
    if top_k > 0:
        s = TopKLogitsWarper(top_k)(ids, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(top_p)(ids, s)
    return (s[0] != -float("inf")).numpy()


@pytest.mark.parametrize("temperature", [0.3, 1.0, 1.5])
@pytest.mark.parametrize("top_k,top_p", [(0, 0.9), (50, 1.0), (50, 0.9), (20, 0.5), (0, 0.5), (1000, 0.95), (0, 1e-3)])
def test_oracle_kept_set_matches_transformers(temperature, top_k, top_p):
    """On random fp32 rows whose top-k / top-p boundaries have margin, the oracle keeps exactly what HF's chain keeps."""
    rng = np.random.default_rng(int(temperature * 10) + 7 * top_k + int(top_p * 100))
    compared = 0
    for _ in range(40):
        x = (rng.standard_normal(2000) * rng.uniform(1, 4)).astype(np.float32)
        kept, info = R.kept_set(x, temperature, top_p, top_k)
        if info["margin"] < 1e-5 * info["Z"]:
            continue
        if 0 < top_k < x.size:
            srt = np.sort(x)[::-1]
            if srt[top_k - 1] - srt[top_k] < 1e-4:
                continue
        compared += 1
        np.testing.assert_array_equal(kept, _hf_survivors(x, temperature, top_p, top_k))
    assert compared >= 20


def test_oracle_keeps_ties_and_drops_minus_inf():
    x = np.array([3.0, 1.0, 3.0, -np.inf, 2.0, 2.0, 2.0, -0.0, 0.0], dtype=np.float32)
    kept, _ = R.kept_set(x, 1.0, 1.0, 3)                  # the 3rd largest is 2.0: every 2.0 stays
    assert kept.tolist() == [True, False, True, False, True, True, True, False, False]
    kept, _ = R.kept_set(x, 1.0, 1.0, 0)
    assert kept.sum() == 8 and not kept[3]
    kept, _ = R.kept_set(x, 1.0, 1e-3, 0)                 # tau = max: both 3.0 stay
    assert kept.tolist() == [True, False, True] + [False] * 6
    assert R.kept_set(np.array([1.0, np.nan], dtype=np.float32), 1.0)[0] is None
    assert R.kept_set(np.array([-np.inf], dtype=np.float32), 1.0)[0] is None


@pytest.fixture(scope="module")
def lib():
    from visionselector_amd import _native as N
    from visionselector_amd import build
    build.build_native(verbose=False)
    return N.lib()


def test_capi_declares_and_exports_sample_tokens(lib):
    from visionselector_amd import _native
    text = open(os.path.join(ROOT, "include", "vsel.h")).read()
    assert re.search(r"\bvsel_sample_tokens\s*\(", text)
    assert "vsel_sample_tokens" in _native.SIGNATURES
    assert hasattr(lib, "vsel_sample_tokens")


# (logits, dtype, batch, vocab, row_stride, temperature, top_p, top_k, tokens): a fake non-NULL device address where one is needed;
# every call below must fail in the host checks, before any HIP call
_OK = dict(logits=16, dtype=0, batch=2, vocab=100, row_stride=100, temperature=1.0, top_p=0.9, top_k=5, tokens=16)


@pytest.mark.parametrize("bad", [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")),
                                 dict(temperature=float("nan")), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.1),
                                 dict(top_p=float("nan")), dict(top_k=-1), dict(vocab=0), dict(batch=-1), dict(row_stride=99),
                                 dict(logits=None), dict(tokens=None), dict(dtype=7)])
def test_sample_tokens_argument_validation_without_gpu(lib, bad):
    a = dict(_OK, **bad)
    st = lib.vsel_sample_tokens(None, a["logits"], a["dtype"], a["batch"], a["vocab"], a["row_stride"], a["temperature"], a["top_p"],
                                a["top_k"], 0, None, 0, a["tokens"], None)
    assert st == 1, lib.vsel_last_error()


def test_sample_tokens_empty_batch_is_a_no_op(lib):
    assert lib.vsel_sample_tokens(None, 16, 0, 0, 100, 100, 1.0, 1.0, 0, 2 ** 64 - 1, None, 2 ** 64 - 1, 16, None) == 0


def test_ops_sample_tokens_refuses_cpu_tensors(lib):
    from visionselector_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.sample_tokens(torch.zeros(2, 10), 1.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.sample_tokens(torch.zeros(2, 10, dtype=torch.bfloat16), 0.7, top_p=0.9, top_k=5, return_kept=True)


@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(temperature=-2.0), dict(temperature=float("nan")), dict(top_p=0.0),
                                dict(top_p=1.01), dict(top_k=-1), dict(top_k=2.5), dict(seed=-1), dict(seed=2 ** 64)])
def test_check_sampling_args_refuses(kw):
    from visionselector_amd import ops
    a = dict(temperature=1.0, top_p=1.0, top_k=0, seed=0)
    a.update(kw)
    with pytest.raises(ValueError):
        ops.check_sampling_args(**a)


def test_packed_generate_signature_has_sampling_keywords():
    from visionselector_amd.generate import packed_generate
    params = inspect.signature(packed_generate).parameters
    want = dict(do_sample=False, temperature=1.0, top_p=1.0, top_k=0, seed=0)
    for name, default in want.items():
        assert name in params and params[name].default == default, name
        assert params[name].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD
