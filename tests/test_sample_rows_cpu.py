"""CPU checks of per-row sampling (vsel_sample_tokens_rows, ops.sample_tokens_rows, packed_generate's per-prompt parameters): the oracle
tests/sampling_rows_ref.py against HF's min-p rule, numpy's argmax and a float64 log-softmax, and the argument checks that run before any
device work."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_rows_ref as RR  # noqa: E402


def _rows(seed, n=40, v=2000):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(v) * rng.uniform(1, 4)).astype(np.float32) for _ in range(n)]


@pytest.mark.parametrize("temperature", [0.3, 1.0, 1.5])
@pytest.mark.parametrize("min_p", [0.05, 0.2, 0.5])
def test_oracle_min_p_matches_hf_rule(temperature, min_p):
    """HF's MinPLogitsWarper removes softmax(x / T) < min_p * max; rows with an entry within 1e-4 (in log2) of the threshold are left out"""
    try:
        from transformers import MinPLogitsWarper
        warper = MinPLogitsWarper(min_p)
    except ImportError:
        warper = None
    compared = 0
    for x in _rows(int(temperature * 10) + int(min_p * 100)):
        z = x.astype(np.float64) / np.float32(temperature)
        p = np.exp(z - z.max())
        p /= p.sum()
        if np.abs(np.log2(p / p.max()) - np.log2(min_p)).min() < 1e-4:
            continue
        compared += 1
        want = ~(p < min_p * p.max())
        kept, _ = RR.final_set(x, temperature, 1.0, 0, min_p)
        np.testing.assert_array_equal(kept, want)
        if warper is not None:
            s = warper(torch.zeros(1, 1, dtype=torch.long), torch.from_numpy(x)[None] / temperature)
            np.testing.assert_array_equal(kept, (s[0] != -float("inf")).numpy())
    assert compared >= 30


def test_oracle_min_p_is_applied_after_top_k_and_top_p():
    for x in _rows(5, n=10):
        before, info = RR.kept_set(x, 0.8, 0.9, 50)
        after, info2 = RR.final_set(x, 0.8, 0.9, 50, 0.3)
        assert info == info2                                      # Z and the target do not see min-p
        assert (after <= before).all() and after[np.argmax(x)]
        np.testing.assert_array_equal(after, before & (RR.d_values(x, 0.8) >= RR.min_p_threshold(0.3)))


def test_oracle_min_p_1_keeps_the_maxima_and_0_changes_nothing():
    x = np.array([1.0, 3.0, -2.0, 3.0, 2.9999998, -np.inf, 3.0], dtype=np.float32)
    kept, _ = RR.final_set(x, 0.7, 1.0, 0, 1.0)
    assert kept.tolist() == [False, True, False, True, False, False, True]
    for xr in _rows(6, n=5):
        for t, p, k in ((1.0, 1.0, 0), (0.5, 0.9, 0), (1.3, 0.8, 40)):
            np.testing.assert_array_equal(RR.final_set(xr, t, p, k, 0.0)[0], RR.kept_set(xr, t, p, k)[0])
        d = RR.d_values(xr, 0.7)
        np.testing.assert_array_equal(RR.final_set(xr, 0.7, 1.0, 0, 1.0)[0], d == d.max())
    assert RR.min_p_threshold(0.0) == -np.inf and RR.min_p_threshold(1.0) == 0 and RR.min_p_threshold(0.5) == -1


def test_oracle_greedy_row_is_argmax():
    for x in _rows(7, n=10):
        x[::7] = -np.inf
        x[100] = x[900] = x.max()                                 # equal maxima: the lowest index
        r = RR.sample_row(x, temperature=0.0, top_p=7.0, top_k=-3, min_p=9.0)       # the other parameters are ignored
        assert r["token"] == int(np.argmax(x)) == 100 and r["kept"] == 1 and r["greedy"]
    assert RR.sample_row(np.array([-0.0, 0.0], dtype=np.float32), temperature=0.0)["token"] == 0


def test_oracle_logprob_is_log_softmax():
    """The 1e-12 bound holds where d carries no float32 rounding: rows of equal finite values (d = 0) with the oracle as it is, and random
    rows through the same function with d = (x - m) * log2(e) given in float64.  With the float32 d the device forms, a random row at
    |logprob| <= 25 is within the GPU gate 1e-6 + 2^-22 |logprob| instead (d's two roundings: up to 2^-23 |d| ln 2, about 2e-6 at d = -30
    on the rare far-tail token, 1e-7 typically), which is the figure asserted below."""
    for v, val in ((1, 3.0), (6, -2.5), (1000, 0.0)):
        x = np.full(v + 2, val, dtype=np.float32)
        x[-2:] = -np.inf
        fin = np.isfinite(x)
        assert abs(RR.logprob(x, 1.0, fin, 0) - (-np.log(v))) <= 1e-12
        assert abs(RR.sample_row(x, temperature=0.0)["logprob"] - (-np.log(v))) <= 1e-12
    for x in _rows(8, n=10):
        z = x.astype(np.float64)
        ref = z - z.max() - np.log(np.exp(z - z.max()).sum())
        kept = np.ones(x.size, dtype=bool)
        top = int(np.argmax(x))
        for tok in (0, top, x.size - 1):
            assert abs(RR.logprob(x, 1.0, kept, tok, d=(z - z.max()) * RR.LOG2E) - ref[tok]) <= 1e-12
            assert abs(RR.logprob(x, 1.0, kept, tok) - ref[tok]) <= 1e-6 + 2.0 ** -22 * abs(ref[tok])
        assert RR.sample_row(x, temperature=0.0)["logprob"] == RR.logprob(x, 1.0, kept, top)


def test_oracle_refuses_bad_rows_and_parameters():
    x = np.array([1.0, 2.0, 0.5], dtype=np.float32)
    for kw in (dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_p=0.0), dict(top_p=1.5),
               dict(top_k=-1), dict(min_p=-0.1), dict(min_p=2.0)):
        r = RR.sample_row(x, **kw)
        assert r["token"] == -1 and r["kept"] == 0 and np.isnan(r["logprob"]), kw
    for bad in ([1.0, np.nan], [np.inf, 0.0], [-np.inf, -np.inf]):
        assert RR.sample_row(np.array(bad, dtype=np.float32), temperature=0.0)["token"] == -1


@pytest.fixture(scope="module")
def lib():
    from visionselector_amd import _native as N
    from visionselector_amd import build
    build.build_native(verbose=False)
    return N.lib()


def test_capi_declares_and_exports_sample_tokens_rows(lib):
    from visionselector_amd import _native
    text = open(os.path.join(ROOT, "include", "vsel.h")).read()
    assert re.search(r"\bvsel_sample_tokens_rows\s*\(", text)
    assert "vsel_sample_tokens_rows" in _native.SIGNATURES
    assert hasattr(lib, "vsel_sample_tokens_rows")


# a fake non-NULL device address where one is needed: every call below must return from the host checks, before any HIP call
_OK = dict(logits=16, dtype=0, batch=2, vocab=100, row_stride=100, tokens=16)


def _call(lib, **kw):
    a = dict(_OK, **kw)
    return lib.vsel_sample_tokens_rows(None, a["logits"], a["dtype"], a["batch"], a["vocab"], a["row_stride"], None, None, None, None, 0,
                                       None, 0, a["tokens"], None, None)


@pytest.mark.parametrize("bad", [dict(logits=None), dict(tokens=None), dict(batch=-1), dict(vocab=0), dict(row_stride=99), dict(dtype=7)])
def test_sample_tokens_rows_argument_validation_without_gpu(lib, bad):
    assert _call(lib, **bad) == 1, lib.vsel_last_error()


def test_sample_tokens_rows_large_vocab_unsupported_and_empty_batch_no_op(lib):
    assert _call(lib, vocab=2 ** 24, row_stride=2 ** 24) == 4, lib.vsel_last_error()
    assert _call(lib, vocab=2 ** 24 - 1, row_stride=2 ** 24 - 1, batch=0) == 0
    assert _call(lib, batch=0) == 0


@pytest.mark.parametrize("kw", [dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(top_p=0.0),
                                dict(top_p=1.01), dict(top_k=-1), dict(top_k=2.5), dict(top_k=2 ** 31), dict(min_p=-0.1), dict(min_p=1.5),
                                dict(min_p=float("nan")), dict(seed=-1), dict(seed=2 ** 64), dict(step=-1)])
def test_ops_sample_tokens_rows_refuses_bad_numbers(kw):
    from visionselector_amd import ops
    with pytest.raises(ValueError, match=next(iter(kw))):
        ops.sample_tokens_rows(torch.zeros(2, 10), **kw)


@pytest.mark.parametrize("kw", [dict(temperature=torch.zeros(2, dtype=torch.float64)), dict(top_p=torch.ones(3)),
                                dict(top_k=torch.zeros(2, dtype=torch.int64)), dict(min_p=torch.zeros(2, 1)),
                                dict(row_ids=torch.zeros(2, dtype=torch.int32))])
def test_ops_sample_tokens_rows_refuses_bad_tensors(kw):
    from visionselector_amd import ops
    with pytest.raises(TypeError, match=next(iter(kw))):
        ops.sample_tokens_rows(torch.zeros(2, 10), **kw)


def test_ops_sample_tokens_rows_refuses_cpu_tensors(lib):
    from visionselector_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.sample_tokens_rows(torch.zeros(2, 10))
    with pytest.raises(RuntimeError, match="GPU only"):                       # temperature 0 (a greedy row) is a valid number here
        ops.sample_tokens_rows(torch.zeros(2, 10, dtype=torch.bfloat16), temperature=0.0, top_p=torch.ones(2), top_k=5, min_p=0.1,
                               return_kept=True, return_logprobs=True)


def test_ops_sample_tokens_rows_is_device_guarded():
    from visionselector_amd import ops
    assert hasattr(ops.sample_tokens_rows, "__wrapped__")


@pytest.mark.parametrize("kw,exc", [(dict(temperature=[1.0]), ValueError), (dict(top_p=[0.9, 0.9, 0.9]), ValueError),
                                    (dict(top_k=(1,)), ValueError), (dict(min_p=[0.1]), ValueError), (dict(do_sample=[True]), ValueError),
                                    (dict(do_sample=True, min_p=1.5), ValueError), (dict(do_sample=True, min_p=-0.1), ValueError),
                                    (dict(do_sample=[False, True], min_p=[0.0, 2.0]), ValueError),
                                    (dict(do_sample=[True, True], temperature=[1.0, 0.0]), ValueError),
                                    (dict(do_sample=[True, 1]), TypeError), (dict(return_logprobs=1), TypeError)])
def test_packed_generate_refuses_bad_per_prompt_arguments_before_device_work(kw, exc):
    from visionselector_amd.generate import packed_generate
    ids = [torch.zeros(4, dtype=torch.long), torch.zeros(5, dtype=torch.long)]
    with pytest.raises(exc):
        packed_generate(None, ids, None, None, [1, 1], max_new_tokens=2, **kw)


def test_packed_generate_signature_has_the_new_keywords():
    import inspect
    from visionselector_amd.generate import packed_generate
    params = inspect.signature(packed_generate).parameters
    assert params["min_p"].default == 0.0 and params["return_logprobs"].default is False
