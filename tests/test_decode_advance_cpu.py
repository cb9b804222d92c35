"""CPU checks of the decode-step bookkeeping (vsel_decode_advance, ops.decode_advance, packed_generate's graph / lookahead keywords):
the library exports the entry, the numpy oracle tests/decode_advance_ref.py obeys its own rules on hand-written cases, and the argument
checks run before any device work."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_advance_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from visionselector_amd import _native as N
    from visionselector_amd import build
    build.build_native(verbose=False)
    return N.lib()


def test_capi_declares_and_exports_decode_advance(lib):
    from visionselector_amd import _native
    text = open(os.path.join(ROOT, "include", "vsel.h")).read()
    assert re.search(r"\bvsel_decode_advance\s*\(", text)
    assert "vsel_decode_advance" in _native.SIGNATURES
    assert hasattr(lib, "vsel_decode_advance")


# ---- the oracle's own rules ------------------------------------------------------------------------------------------------------

def _state(b=3, max_new=4):
    return R.new_state([10 + i for i in range(b)], [[100 + i for i in range(b)]] * 3, max_new)


def test_oracle_first_token_does_not_advance_later_ones_do():
    st = _state()
    R.decode_advance(st, [5, 6, 7], [], 4)
    assert st["cache_seqlens"].tolist() == [10, 11, 12] and st["pos"][0].tolist() == [100, 101, 102]
    assert st["n_tokens"].tolist() == [1, 1, 1] and st["feed"].tolist() == [5, 6, 7] and st["tokens_out"][:, 0].tolist() == [5, 6, 7]
    R.decode_advance(st, [8, 9, 10], [], 4)
    assert st["cache_seqlens"].tolist() == [11, 12, 13] and (st["pos"] == np.array([[101, 102, 103]] * 3)).all()
    assert st["n_tokens"].tolist() == [2, 2, 2] and st["feed"].tolist() == [8, 9, 10]
    assert st["status"].tolist() == [3, -1, -1, 0]


def test_oracle_done_row_never_changes():
    st = _state()
    R.decode_advance(st, [5, 6, 7], [6], 4)                       # row 1 stops on eos
    assert st["done"].tolist() == [0, 1, 0] and st["status"][0] == 2
    frozen = {k: v[..., 1].copy() if k == "pos" else v[1].copy() for k, v in st.items() if k != "status"}
    for nxt in ([1, 2, 3], [1, -1, 3], [1, 6, 3]):
        R.decode_advance(st, nxt, [6], 4)
        for k, v in frozen.items():
            now = st[k][..., 1] if k == "pos" else st[k][1]
            assert np.array_equal(now, v), k
    assert st["feed"][1] == 0                                       # the eos token was never fed
    assert st["tokens_out"][1].tolist() == [6, -7, -7, -7]


def test_oracle_eos_beats_length_when_both_hold():
    st = _state(b=2, max_new=2)
    R.decode_advance(st, [5, 5], [9], 2)
    R.decode_advance(st, [9, 4], [9], 2)                           # both rows reach the limit; row 0's token is also eos
    assert st["done"].tolist() == [1, 2] and st["n_tokens"].tolist() == [2, 2] and st["status"].tolist() == [0, -1, -1, 0]
    assert st["feed"].tolist() == [5, 5]                            # a stopping row keeps its feed


def test_oracle_no_eos_runs_to_the_length_limit():
    st = _state(b=2, max_new=3)
    for s in range(3):
        R.decode_advance(st, [s, s + 1], [], 3)
        assert st["status"][0] == (2 if s < 2 else 0)
    assert st["done"].tolist() == [2, 2] and st["tokens_out"].tolist() == [[0, 1, 2], [1, 2, 3]]
    assert st["cache_seqlens"].tolist() == [12, 13]                  # L + max_new - 1 keys: the last token is never fed back


def test_oracle_invalid_row_writes_no_token_and_lowest_is_reported():
    st = _state(b=4, max_new=4)
    R.decode_advance(st, [5, 6, 7, 8], [], 4)
    R.decode_advance(st, [5, -1, 7, -1], [], 4)
    assert st["done"].tolist() == [0, 3, 0, 3] and st["status"].tolist() == [2, 1, 1, 0]
    assert st["n_tokens"].tolist() == [2, 1, 2, 1] and st["tokens_out"][1].tolist() == [6, -7, -7, -7]
    R.decode_advance(st, [5, -1, 7, -1], [], 4)                    # already done rows are not reported again
    assert st["status"].tolist() == [2, -1, -1, 0]


def test_oracle_status0_counts_active_rows():
    rng = np.random.default_rng(0)
    st = R.new_state(rng.integers(1, 50, 40), rng.integers(1, 50, (3, 40)), 6)
    for _ in range(6):
        R.decode_advance(st, rng.integers(-1, 8, 40), [3, 4], 6)
        assert st["status"][0] == int((st["done"] == 0).sum())
    assert st["status"][0] == 0


def test_oracle_corrupt_count_stops_the_row_without_a_write():
    st = _state(b=2, max_new=3)
    st["n_tokens"][1] = 3
    before = st["tokens_out"].copy()
    R.decode_advance(st, [5, 6], [], 3)
    assert st["done"].tolist() == [0, 2] and np.array_equal(st["tokens_out"][1], before[1]) and st["cache_seqlens"][1] == 11


# ---- host checks: before any device work -------------------------------------------------------------------------------------------

# (next, batch, eos, n_eos, max_new_tokens, done, n_tokens, cache_seqlens, pos, pos_is_int64, feed, tokens_out, status): a fake non-NULL
# device address where one is needed; every call below must fail in the host checks, before any HIP call
_OK = dict(next=16, batch=2, eos=16, n_eos=1, max_new=4, done=16, n_tokens=16, seqlens=16, pos=16, pos64=1, feed=16, out=16, status=16)


@pytest.mark.parametrize("bad", [dict(max_new=0), dict(max_new=-3), dict(batch=-1), dict(n_eos=-1), dict(eos=None), dict(next=None),
                                 dict(done=None), dict(n_tokens=None), dict(seqlens=None), dict(pos=None), dict(feed=None),
                                 dict(out=None), dict(status=None), dict(pos64=2)])
def test_decode_advance_argument_validation_without_gpu(lib, bad):
    a = dict(_OK, **bad)
    st = lib.vsel_decode_advance(None, a["next"], a["batch"], a["eos"], a["n_eos"], a["max_new"], a["done"], a["n_tokens"], a["seqlens"],
                                 a["pos"], a["pos64"], a["feed"], a["out"], a["status"])
    assert st == 1, lib.vsel_last_error()


def test_decode_advance_batch_2_31_unsupported(lib):
    assert lib.vsel_decode_advance(None, 16, 2 ** 31, None, 0, 4, 16, 16, 16, 16, 1, 16, 16, 16) == 4


def _cpu_args(b=2, max_new=4):
    return dict(next_tokens=torch.zeros(b, dtype=torch.int64), eos=torch.zeros(1, dtype=torch.int64), max_new_tokens=max_new,
                done=torch.zeros(b, dtype=torch.int32), n_tokens=torch.zeros(b, dtype=torch.int32),
                cache_seqlens=torch.zeros(b, dtype=torch.int32), pos=torch.zeros(3, b, dtype=torch.int64),
                feed=torch.zeros(b, dtype=torch.int64), tokens_out=torch.zeros(b, max_new, dtype=torch.int64),
                status=torch.zeros(4, dtype=torch.int32))


@pytest.mark.parametrize("bad,exc", [
    (dict(max_new_tokens=0), ValueError), (dict(max_new_tokens=True), ValueError), (dict(max_new_tokens=2.0), ValueError),
    (dict(next_tokens=torch.zeros(2, dtype=torch.int32)), TypeError), (dict(done=torch.zeros(2, dtype=torch.int64)), TypeError),
    (dict(n_tokens=torch.zeros(3, dtype=torch.int32)), TypeError), (dict(cache_seqlens=torch.zeros(2, dtype=torch.int64)), TypeError),
    (dict(pos=torch.zeros(2, 3, dtype=torch.int64)), TypeError), (dict(pos=torch.zeros(3, 2, dtype=torch.float32)), TypeError),
    (dict(feed=torch.zeros(2, dtype=torch.int32)), TypeError), (dict(tokens_out=torch.zeros(2, 5, dtype=torch.int64)), TypeError),
    (dict(status=torch.zeros(3, dtype=torch.int32)), TypeError), (dict(eos=torch.zeros(1, dtype=torch.int32)), TypeError),
])
def test_ops_decode_advance_refuses_wrong_dtypes_and_shapes(lib, bad, exc):
    from visionselector_amd import ops
    with pytest.raises(exc):
        ops.decode_advance(**dict(_cpu_args(), **bad))


def test_ops_decode_advance_refuses_cpu_tensors(lib):
    from visionselector_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.decode_advance(**_cpu_args())


def test_packed_generate_signature_has_graph_and_lookahead():
    from visionselector_amd.generate import DEFAULT_LOOKAHEAD, packed_generate
    prm = inspect.signature(packed_generate).parameters
    assert prm["graph"].default is False and prm["lookahead"].default == DEFAULT_LOOKAHEAD and DEFAULT_LOOKAHEAD >= 1


@pytest.mark.parametrize("kw,exc", [(dict(lookahead=0), ValueError), (dict(lookahead=-2), ValueError), (dict(lookahead=1.5), ValueError),
                                    (dict(lookahead=True), ValueError), (dict(graph="yes"), TypeError), (dict(max_new_tokens=0), ValueError)])
def test_packed_generate_graph_argument_checks_run_before_any_device_work(kw, exc):
    """model=None: any touch of the model (let alone the device) would raise AttributeError instead."""
    from visionselector_amd.generate import packed_generate
    args = dict(dict(max_new_tokens=4, graph=True), **kw)
    with pytest.raises(exc):
        packed_generate(None, [torch.zeros(3, dtype=torch.int64)], torch.zeros(4, 8), torch.ones(1, 3, dtype=torch.int64), [1], **args)


def test_decode_graphs_checks_its_arguments():
    from visionselector_amd.generate import DecodeGraphs
    with pytest.raises(ValueError):
        DecodeGraphs(None, None, 0)
