"""Every entry that runs the LIS scores stage gives the same scores, bit for bit, on the same tokens: lis_scores, lis_select,
lis_select_varlen, lis_select_permuted, lis_select_splice and (one segment) lis_train_fwd -- on both sides of the bf16x3-MFMA
condition of make_plan (csrc/lis_stages.h: D % 16 == 0 and Hd % 16 == 0), for every (token, weight) dtype pair check_scorer
accepts, for a batch the small-batch form takes (1) and one it never takes (9 > kSmallMaxSeg), with the small-batch form on
(default) and off (knob lis_small_path = 0).  Run on the MI355X box:  pytest -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, K = 300, 37                  # three 128-row chunks of sweep 1, the last one ragged
VISUAL_ID = 7
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from visionselector_amd import ops as _ops
    return _ops


def _inputs(b, d, hd, tdt, wdt):
    """Tokens in multiples of 1/8 within [-4, 4]: exact in bf16, and a column's fp32 sum over 300 rows is exact in ANY order, so
    the permuted entry (which sums the rows in physical order) must reproduce lis_select on h[l2p] bit for bit.  The weights are
    ordinary random numbers: the projections and the row dot products round like on any input."""
    g = torch.Generator().manual_seed(1000 * b + d)
    h = (torch.randint(-32, 33, (b, N, d), generator=g).float() / 8).to(tdt).cuda()
    wq, wk = (((torch.randn(hd, d, generator=g) * 0.05).to(wdt)).cuda() for _ in range(2))
    bq, bk = (((torch.randn(hd, generator=g) * 0.05).to(wdt)).cuda() for _ in range(2))
    # per-segment permutation, global row numbers (as Qwen2.5-VL's window_index / reverse_indices)
    p2l = torch.cat([torch.randperm(N, generator=g) + i * N for i in range(b)]).cuda()
    l2p = torch.argsort(p2l)
    return h, (wq, bq, wk, bk), l2p, p2l


def _prompts(b, d, tdt):
    """b prompts back to back: 2 text positions, N visual placeholders, 3 text positions."""
    ids_one = torch.tensor([1, 2] + [VISUAL_ID] * N + [3, 4, 5], dtype=torch.int64)
    seq = ids_one.numel()
    ids = ids_one.repeat(b).cuda()
    emb = torch.zeros(b * seq, d, dtype=tdt, device="cuda")
    return ids, emb, [seq] * b


@pytest.mark.parametrize("small_path", ["default", "off"])
@pytest.mark.parametrize("b", [1, 9])
@pytest.mark.parametrize("wname", list(DTYPES))
@pytest.mark.parametrize("tname", list(DTYPES))
@pytest.mark.parametrize("d,hd", [(128, 64), (72, 40)])
def test_every_entry_gives_the_same_scores(ops, d, hd, tname, wname, b, small_path):
    from visionselector_amd._native import debug_get, debug_knob
    tdt, wdt = DTYPES[tname], DTYPES[wname]
    h, w, l2p, p2l = _inputs(b, d, hd, tdt, wdt)
    flat = h.view(b * N, d)
    h_phys = torch.empty_like(flat)
    h_phys[l2p] = flat                                   # so that h_phys[l2p] == h
    assert torch.equal(h_phys[l2p], flat)
    ids, emb, seq_lens = _prompts(b, d, tdt)
    with debug_knob("lis_small_path", 0 if small_path == "off" else debug_get("lis_small_path")):
        got = {
            "lis_scores": ops.lis_scores(h, *w),
            "lis_select": ops.lis_select(h, *w, K)[2],
            "lis_select_varlen": ops.lis_select_varlen(flat, [N] * b, [K] * b, *w)[2],
            "lis_select_permuted": ops.lis_select_permuted(h_phys.view(b, N, d), l2p, p2l, *w, K)[2],
            "lis_select_splice": ops.lis_select_splice(flat, *w, ids, emb, VISUAL_ID, seq_lens, [N] * b, [K] * b)["scores"],
        }
        if b == 1:
            got["lis_train_fwd"] = ops.lis_train_fwd(h[0], *w, K)[3]
    got = {name: s.reshape(b, N) for name, s in got.items()}
    assert bool(torch.isfinite(got["lis_scores"]).all()) and float(got["lis_scores"].std()) > 0
    names = list(got)
    for i, x in enumerate(names):
        for y in names[i + 1:]:
            assert torch.equal(got[x], got[y]), (x, y, float((got[x] - got[y]).abs().max()))
