"""The bf16x3 projections with their split-K slices summed in LDS (knob lis_proj_sum = 1: gemm_nt_sum / gemm_nn_sum_bf16x3_kernel,
two launches, no slabs) against the slab form (knob 0: slab GEMM + finish kernel twice): scores, indices and kept rows bit for bit
at every tile edge of the two kernels, the scores also against the oracle.  Tokens per image stay tiny: the projections do not
depend on N.  Run on the MI355X box:  pytest -m gpu."""
import numpy as np
import pytest
import torch

from oracle import inputs as oin
from oracle import lis as olis

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from visionselector_amd import ops as _ops
    return _ops


def dev(a, dtype=torch.bfloat16):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype)


def form(f):
    """with form(1): the LDS-summed projections; form(0): the slab form.  Never the small-batch kernels (they have projections of their own)."""
    from visionselector_amd._native import debug_knob
    return debug_knob(lis_proj_sum=f, lis_small_path=0)


def both_forms(call):
    """call() under form 0 and form 1 with the profiler on -> (outputs of form 1, profile of form 0, profile of form 1); asserts bit equality
    and that each form ran the launches it is meant to."""
    from visionselector_amd import _native
    res, prof = {}, {}
    for f in (0, 1):
        with form(f):
            _native.profile_start()
            res[f] = call()
            torch.cuda.synchronize()
            prof[f] = _native.profile_stop()
    for x, y in zip(res[1], res[0]):
        assert x.shape == y.shape and torch.equal(x, y)
    for nm in ("kbar_finish_split_kernel", "w_finish_kernel"):
        assert nm in prof[0] and nm not in prof[1], (nm, prof)
    for nm in ("gemm_nt_bf16x3_kernel", "gemm_nn_bf16x3_kernel"):
        assert nm in prof[0] and nm in prof[1], (nm, prof)
    assert sum(c for _, c in prof[1].values()) == sum(c for _, c in prof[0].values()) - 2, prof
    return res[1]


def check_vs_oracle(scores, c):
    """the tolerance tests/test_lis_gpu.py uses for scores"""
    ref = olis.scorer_reference(c["h"], c["wq"], c["bq"], c["wk"], c["bk"])
    s = scores.cpu().numpy()
    err, bound = np.abs(s - ref).max(), 4e-6 * max(1.0, np.abs(ref).max())
    print(f"max |score - oracle| = {err:.3e}, bound {bound:.3e}")
    assert s.shape == ref.shape and err <= bound


# S: the m-tile edges and padded columns.  hd: NT n-tile edges (144 also: two NN slices, the last 16 wide).  d: a K shorter than one
# slice, a ragged last NT slice, the NN strip edge with its clamped loads.  (33, 3584, 1792): the 14 + 14 slices of the headline geometry.
SHAPES = [(s, 256, 128) for s in (1, 31, 32, 33, 65)] + [(33, 256, hd) for hd in (16, 48, 80, 144)] + \
         [(33, d, 64) for d in (16, 64, 272, 528)] + [(33, 3584, 1792)]


@pytest.mark.parametrize("s,d,hd", SHAPES)
def test_summed_projections_are_bit_identical(ops, s, d, hd):
    n, k = 8, 3
    c = oin.make_case(d, hd, n, 1000 + s + d + hd, batch=s)
    h, wq, bq, wk, bk = (dev(c[x]) for x in ("h", "wq", "bq", "wk", "bk"))
    out, idx, scores = both_forms(lambda: ops.lis_select(h, wq, bq, wk, bk, k))
    check_vs_oracle(scores, c)
    with form(1):
        assert torch.equal(ops.lis_scores(h, wq, bq, wk, bk), scores)        # the scores-only entry takes the same projections


def test_summed_projections_on_segment_sum_planes(ops):
    """Planes written by colsum_seg_kernel (more than one 128-row chunk and >= 896 (segment, slab) pairs), as at the headline batch."""
    s, d, hd, n = 33, 3584, 1792, 136
    g = torch.Generator(device="cuda").manual_seed(5)
    h = torch.randn(s, n, d, device="cuda", generator=g).bfloat16()
    wq, wk = [(0.02 * torch.randn(hd, d, device="cuda", generator=g)).bfloat16() for _ in range(2)]
    bq, bk = [(0.02 * torch.randn(hd, device="cuda", generator=g)).bfloat16() for _ in range(2)]
    from visionselector_amd import _native
    with form(1):
        _native.profile_start()
        ops.lis_select(h, wq, bq, wk, bk, 27)
        torch.cuda.synchronize()
        assert "colsum_seg_kernel" in _native.profile_stop()
    both_forms(lambda: ops.lis_select(h, wq, bq, wk, bk, 27))


def test_summed_projections_ragged_and_presummed(ops):
    """Ragged segments and producer-supplied column sums at 33 segments: planes from colsum_finish_split_kernel."""
    d, hd = 256, 128
    lens = [8, 1, 130, 5, 17, 64, 9, 3, 40, 12, 7] * 3
    ks = [max(1, n // 3) for n in lens]
    c = oin.make_case(d, hd, sum(lens), 41)
    h, wq, bq, wk, bk = (dev(c[x]) for x in ("h", "wq", "bq", "wk", "bk"))
    out, idx, scores = both_forms(lambda: ops.lis_select_varlen(h, lens, ks, wq, bq, wk, bk))
    ro = 0
    for n in lens:
        seg = {**c, "h": c["h"][ro:ro + n][None]}
        check_vs_oracle(scores[ro:ro + n][None], seg)
        ro += n
    c2 = oin.make_case(d, hd, 8, 42, batch=33)
    h2 = dev(c2["h"])
    sums = h2.float().sum(1).contiguous()
    out, idx, scores = both_forms(lambda: ops.lis_select_presummed(h2, sums, wq, bq, wk, bk, 3))
    check_vs_oracle(scores, {**c, "h": c2["h"]})


def test_summed_projections_repeat_and_capture(ops):
    """Twenty back-to-back calls give the same bits, and the call captures into a graph and replays to them."""
    c = oin.make_case(528, 144, 8, 43, batch=33)
    h, wq, bq, wk, bk = (dev(c[x]) for x in ("h", "wq", "bq", "wk", "bk"))
    with form(1):
        outs = [ops.lis_select(h, wq, bq, wk, bk, 3) for _ in range(20)]
        torch.cuda.synchronize()
        for o in outs[1:]:
            for x, y in zip(o, outs[0]):
                assert torch.equal(x, y)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            ops.lis_select(h, wq, bq, wk, bk, 3)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = ops.lis_select(h, wq, bq, wk, bk, 3)
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
    for a, b in zip(outs[0], out):
        assert torch.equal(a, b)
