"""vsel_sample_tokens (ops.sample_tokens) on the GPU against the numpy oracle tests/sampling_ref.py: the kept set and
the token over a matrix of dtypes / vocabularies / batches / temperatures / filters, ties, determinism, row independence, the
sampled distribution, invalid rows, strided rows and top_k = 1."""
import itertools

import numpy as np
import pytest
import torch

import sampling_ref as R

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
VOCABS = [1, 63, 1000, 100_003, 151_936, 152_064]
TOL = 1e-4


def _logits(b, v, dtype, gen, scale=None):
    """rows of random logits with a spread like an LM head's: N(0, s) with s per row in [1, 4], a few boosted entries"""
    s = torch.empty(b, 1).uniform_(1.0, 4.0, generator=gen) if scale is None else torch.full((b, 1), scale)
    x = torch.randn(b, v, generator=gen) * s
    hot = torch.randint(0, v, (b, 8), generator=gen)
    x.scatter_add_(1, hot, torch.rand(b, 8, generator=gen) * 12)
    return x.to(dtype)


def _check_rows(x, tokens, kept, temperature, top_p, top_k, seed, row_ids, step, max_rows=None):
    """-> (rows compared, rows matching exactly); asserts the per-row rules of the oracle matrix"""
    xs = x.float().cpu().numpy()
    rows = range(xs.shape[0]) if max_rows is None else range(min(max_rows, xs.shape[0]))
    n = exact = 0
    for r in rows:
        tok, kc, scores, info = R.sample(xs[r], temperature, top_p, top_k, seed, int(row_ids[r]), step)
        n += 1
        near = info.get("margin", float("inf")) < TOL * info.get("Z", 0)
        if not near:
            assert kept[r] == kc, (r, kept[r], kc, info)
        if kept[r] != kc:
            continue                       # the target sits on a cumulative-mass step: fp32 exp2 decides
        srt = np.sort(scores[np.isfinite(scores)])[::-1]
        gap = srt[0] - srt[1] if srt.size > 1 else float("inf")
        if gap > TOL:
            assert tokens[r] == tok, (r, tokens[r], tok, gap)
        else:
            assert np.isfinite(scores[tokens[r]]) and scores[tokens[r]] >= srt[0] - TOL, (r, tokens[r], tok)
        exact += int(tokens[r] == tok)
    return n, exact


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("v", VOCABS)
def test_oracle_matrix(dt, v):
    from visionselector_amd import ops
    gen = torch.Generator().manual_seed(v + (7 if dt == "fp32" else 0))
    combos = list(itertools.product([0, 1, 50, v], [1.0, 0.9, 0.5, 1e-3]))
    temps, batches = [0.3, 1.0, 1.5], [1, 7, 32]
    n = exact = 0
    for c, (top_k, top_p) in enumerate(combos):
        t, b = temps[c % 3], batches[(c // 3 + c) % 3]
        x = _logits(b, v, DTYPES[dt], gen).cuda()
        row_ids = torch.randint(0, 2 ** 32, (b,), generator=gen, dtype=torch.int64)
        seed, step = int(torch.randint(0, 2 ** 62, (1,), generator=gen)), c * 1000 + 3
        tok, kept = ops.sample_tokens(x, t, top_p=top_p, top_k=top_k, seed=seed, row_ids=row_ids.cuda(), step=step, return_kept=True)
        tok, kept = tok.cpu().numpy(), kept.cpu().numpy()
        dn, de = _check_rows(x, tok, kept, t, top_p, top_k, seed, row_ids.numpy(), step, max_rows=8 if v > 100_000 else None)
        n += dn
        exact += de
    assert exact >= 0.99 * n, (exact, n)


def test_bf16_ties_are_all_kept():
    from visionselector_amd import ops
    v = 4096
    x = torch.full((2, v), -20.0)
    # row 0: the 5th largest value (4.0) is tied 10 times -> top_k = 5 keeps 3 + 10
    x[0, 100:103] = 5.0
    x[0, 200:210] = 4.0
    # row 1: the top-p boundary falls inside a group of six equal values -> all six stay
    x[1, 7] = 3.0
    x[1, 1000:1006] = 2.0
    x = x.bfloat16().cuda()
    _, kept = ops.sample_tokens(x[:1], 1.0, top_k=5, return_kept=True)
    assert kept.item() == 13
    _, kept = ops.sample_tokens(x[1:], 1.0, top_p=0.5, return_kept=True)
    assert kept.item() == 7
    for r, (kw) in enumerate([dict(top_k=5), dict(top_p=0.5)]):
        want, _ = R.kept_set(x[r].float().cpu().numpy(), 1.0, kw.get("top_p", 1.0), kw.get("top_k", 0))
        assert int(want.sum()) == (13 if r == 0 else 7)


def test_deterministic_and_seeded():
    from visionselector_amd import ops
    gen = torch.Generator().manual_seed(11)
    x = _logits(256, 152_064, torch.bfloat16, gen).cuda()
    runs = [ops.sample_tokens(x, 0.9, top_p=0.95, top_k=200, seed=5, step=9, return_kept=True) for _ in range(3)]
    for tok, kept in runs[1:]:
        assert torch.equal(tok, runs[0][0]) and torch.equal(kept, runs[0][1])
    other = ops.sample_tokens(x, 0.9, top_p=0.95, top_k=200, seed=6, step=9)
    assert (other != runs[0][0]).sum().item() > 0


def test_rows_are_independent():
    from visionselector_amd import ops
    gen = torch.Generator().manual_seed(12)
    x = _logits(64, 32_000, torch.float32, gen).cuda()
    ids = torch.randint(0, 2 ** 32, (64,), generator=gen, dtype=torch.int64).cuda()
    kw = dict(top_p=0.9, top_k=0, seed=123, step=4, return_kept=True)
    tok, kept = ops.sample_tokens(x, 1.2, row_ids=ids, **kw)
    perm = torch.randperm(64, generator=gen).cuda()
    tp, kp = ops.sample_tokens(x[perm], 1.2, row_ids=ids[perm], **kw)
    assert torch.equal(tp, tok[perm]) and torch.equal(kp, kept[perm])
    sub = torch.tensor([3, 17, 40], device="cuda")
    ts, ks = ops.sample_tokens(x[sub], 1.2, row_ids=ids[sub], **kw)
    assert torch.equal(ts, tok[sub]) and torch.equal(ks, kept[sub])
    # default row ids are the row positions
    t0 = ops.sample_tokens(x, 1.2, top_p=0.9, seed=123, step=4)
    t1 = ops.sample_tokens(x, 1.2, top_p=0.9, seed=123, step=4, row_ids=torch.arange(64, device="cuda"))
    assert torch.equal(t0, t1)


def test_distribution_matches_renormalised_probabilities():
    from visionselector_amd import ops
    gen = torch.Generator().manual_seed(13)
    v, t, top_k, top_p = 32, 0.8, 20, 0.9
    row = (torch.randn(v, generator=gen) * 2).float()
    kept_mask, _ = R.kept_set(row.numpy(), t, top_p, top_k)
    p = np.where(kept_mask, np.exp((row.double().numpy() - row.max().item()) / np.float32(t)), 0.0)
    p /= p.sum()
    rows = 4096
    x = row[None].expand(rows, v).contiguous().cuda()
    counts = np.zeros(v, dtype=np.int64)
    for step in range(32):                                        # 2^17 draws over distinct (row_id, step)
        tok = ops.sample_tokens(x, t, top_p=top_p, top_k=top_k, seed=99, row_ids=torch.arange(rows, device="cuda"), step=step)
        counts += np.bincount(tok.cpu().numpy(), minlength=v)
    n = counts.sum()
    assert n == 2 ** 17
    assert counts[~kept_mask].sum() == 0
    sigma = np.sqrt(n * p * (1 - p))
    dev = np.abs(counts - n * p)
    assert (dev[kept_mask] <= 5 * sigma[kept_mask] + 1).all(), (counts, n * p)


def test_edge_cases():
    from visionselector_amd import ops
    one = torch.randn(3, 1).cuda()
    assert ops.sample_tokens(one, 1.0).tolist() == [0, 0, 0]
    assert ops.sample_tokens(one.bfloat16(), 0.5, top_p=0.1, top_k=1).tolist() == [0, 0, 0]
    # -inf entries are never drawn, whatever the filters
    gen = torch.Generator().manual_seed(14)
    x = torch.randn(512, 1000, generator=gen)
    x[:, ::2] = float("-inf")
    for kw in (dict(), dict(top_k=700), dict(top_p=0.999)):
        tok, kept = ops.sample_tokens(x.cuda(), 2.0, return_kept=True, **kw)
        assert (tok % 2 == 1).all() and (kept <= 500).all()
    # invalid rows -> -1; valid rows of the same call keep their oracle result
    y = _logits(6, 1003, torch.float32, gen)
    y[1] = float("-inf")
    y[3, 17] = float("nan")
    y[4, 500] = float("inf")
    for dtype in (torch.float32, torch.bfloat16):
        yd = y.to(dtype)
        tok, kept = ops.sample_tokens(yd.cuda(), 0.7, top_p=0.8, seed=3, step=1, return_kept=True)
        tok, kept = tok.cpu().numpy(), kept.cpu().numpy()
        assert [tok[r] for r in (1, 3, 4)] == [-1, -1, -1] and [kept[r] for r in (1, 3, 4)] == [0, 0, 0]
        n, exact = _check_rows(yd[[0, 2, 5]], tok[[0, 2, 5]], kept[[0, 2, 5]], 0.7, 0.8, 0, 3, [0, 2, 5], 1)
        assert n == 3


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("v", [1003, 152_064])
def test_strided_rows_match_contiguous(dt, v):
    from visionselector_amd import ops
    gen = torch.Generator().manual_seed(15)
    full = torch.randn(9, 3, v, generator=gen).to(DTYPES[dt]).cuda()
    last = full[:, -1, :]
    assert not last.is_contiguous()
    for kw in (dict(), dict(top_k=50), dict(top_p=0.9), dict(top_k=50, top_p=0.9)):
        a = ops.sample_tokens(last, 0.8, seed=1, step=2, return_kept=True, **kw)
        b = ops.sample_tokens(last.contiguous(), 0.8, seed=1, step=2, return_kept=True, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # a row that starts off a 16-byte boundary
    off = full.reshape(-1)[1:1 + 4 * v].view(4, v)
    a = ops.sample_tokens(off, 1.0, top_p=0.7, seed=4, return_kept=True)
    b = ops.sample_tokens(off.contiguous(), 1.0, top_p=0.7, seed=4, return_kept=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_top_k_1_is_argmax(dt):
    from visionselector_amd import ops
    gen = torch.Generator().manual_seed(16)
    x = _logits(64, 152_064, DTYPES[dt], gen).cuda()
    top2 = x.float().topk(2, dim=-1).values
    unique = top2[:, 0] > top2[:, 1]
    assert unique.sum() >= 32
    tok, kept = ops.sample_tokens(x, 1.3, top_k=1, top_p=0.9, seed=8, return_kept=True)
    assert torch.equal(tok[unique], x.argmax(-1)[unique])
    assert (kept[unique] == 1).all()
