"""vsel_sample_tokens_rows (ops.sample_tokens_rows) on the GPU ("per-row parameters"): bit-equal to ops.sample_tokens at
uniform parameters; a batch of 32 rows with their own temperature (0: greedy) / top-k / top-p / min-p against the numpy oracle
tests/sampling_rows_ref.py, kept sets, tokens and log-probabilities; row independence, ties, rejected values, determinism."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import sampling_rows_ref as RR

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
TOL = 1e-4                       # tests/test_sample_gpu.py's: a top-p target this close (in Z) to a cumulative-mass step is decided by exp2f
B = 32
SEED0 = 1000                     # fixed so that the oracle alone has no row within TOL of a cumulative-mass step (checked below)
# (temperature, top_k, top_p, min_p) of rows 0-7: greedy, min-p alone (loose, tied maxima only), no filter, all three, top-p, top-k with
# min-p, the tightest top-p
FIRST = [(0.0, 50, 0.9, 0.5), (0.3, 0, 1.0, 0.05), (1.0, 0, 1.0, 1.0), (1.5, 0, 1.0, 0.0), (1.0, 50, 0.9, 0.05), (0.3, 0, 0.9, 0.0),
         (1.5, 50, 1.0, 0.5), (1.0, 0, 1e-3, 0.0)]
TEMPS, TOP_KS, TOP_PS, MIN_PS = [0.0, 0.3, 1.0, 1.5], [0, 1, 50, None], [1.0, 0.9, 1e-3], [0.0, 0.05, 0.5, 1.0]      # None: V


def _lp_gate(ref: float) -> float:
    """fp32 exp2 terms good to about an ulp, the floor drops at most V * 2^-40 of the top mass, one fp32 rounding of the result"""
    return 1e-6 + 2.0 ** -22 * abs(ref)


def _logits(b, v, dtype, gen):
    """rows like an LM head's (tests/test_sample_gpu.py): N(0, s), s per row in [1, 4], a few boosted entries.  (On flat rows of a large
    vocabulary every top-p target is within TOL * Z of a cumulative-mass step, since no single entry weighs that much.)"""
    x = torch.randn(b, v, generator=gen) * torch.empty(b, 1).uniform_(1.0, 4.0, generator=gen)
    hot = torch.randint(0, v, (b, 8), generator=gen)
    x.scatter_add_(1, hot, torch.rand(b, 8, generator=gen) * 12)
    return x.to(dtype)


def _pick(values, n, gen):
    return [values[i] for i in torch.randint(0, len(values), (n,), generator=gen).tolist()]


@functools.lru_cache(maxsize=None)
def _mixed(dt, v):
    """The mixed batch of one dtype and vocabulary, and the oracle's rows (the first 8 when V > 100 000): computed once, never changed"""
    gen = torch.Generator().manual_seed(SEED0 + v + (7 if dt == "fp32" else 0))
    x = _logits(B, v, DTYPES[dt], gen)
    par = dict(temperature=_pick(TEMPS, B, gen), top_k=[v if k is None else k for k in _pick(TOP_KS, B, gen)],
               top_p=_pick(TOP_PS, B, gen), min_p=_pick(MIN_PS, B, gen))
    for r, (t, k, p, mp) in enumerate(FIRST):         # every kind of row among the eight that are compared at every vocabulary
        par["temperature"][r], par["top_k"][r], par["top_p"][r], par["min_p"][r] = t, k, p, mp
    row_ids = torch.randint(0, 2 ** 32, (B,), generator=gen, dtype=torch.int64)
    seed, step = int(torch.randint(0, 2 ** 62, (1,), generator=gen)), 2 ** 33 + v
    xs = x.float().numpy()
    n = 8 if v > 100_000 else B
    ref = [RR.sample_row(xs[r], par["temperature"][r], par["top_p"][r], par["top_k"][r], par["min_p"][r], seed, int(row_ids[r]), step)
           for r in range(n)]
    return x, par, row_ids, seed, step, ref


def _device_params(par, rows=None):
    sel = (lambda a: a) if rows is None else (lambda a: [a[r] for r in rows])
    return dict(temperature=torch.tensor(sel(par["temperature"]), dtype=torch.float32, device="cuda"),
                top_p=torch.tensor(sel(par["top_p"]), dtype=torch.float32, device="cuda"),
                top_k=torch.tensor(sel(par["top_k"]), dtype=torch.int32, device="cuda"),
                min_p=torch.tensor(sel(par["min_p"]), dtype=torch.float32, device="cuda"))


def _run(x, par, row_ids, seed, step, rows=None):
    from visionselector_amd import ops
    xs = x if rows is None else x[rows]
    ids = row_ids if rows is None else row_ids[rows]
    tok, kept, lp = ops.sample_tokens_rows(xs.cuda(), seed=seed, row_ids=ids.cuda(), step=step, return_kept=True, return_logprobs=True,
                                           **_device_params(par, rows))
    return tok.cpu().numpy(), kept.cpu().numpy(), lp.cpu().numpy()


def _near(ref_row) -> bool:
    info = ref_row["info"]
    return info.get("margin", float("inf")) < TOL * info.get("Z", 0)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("v", [1, 63, 1000, 100_003])
def test_uniform_parameters_match_the_scalar_entry_bit_for_bit(dt, v):
    from visionselector_amd import ops
    gen = torch.Generator().manual_seed(v + (7 if dt == "fp32" else 0))
    for c, (b, (top_k, top_p)) in enumerate(itertools.product([1, 7, 32], [(0, 1.0), (50, 1.0), (0, 0.9), (50, 0.5)])):
        t = [0.3, 1.0, 1.5][c % 3]
        x = _logits(b, v, DTYPES[dt], gen).cuda()
        ids = torch.randint(0, 2 ** 32, (b,), generator=gen, dtype=torch.int64).cuda()
        seed, step = int(torch.randint(0, 2 ** 62, (1,), generator=gen)), c * 1000 + 3
        want = ops.sample_tokens(x, t, top_p=top_p, top_k=top_k, seed=seed, row_ids=ids, step=step, return_kept=True)
        arrays = dict(temperature=torch.full((b,), t, device="cuda"), top_p=torch.full((b,), top_p, device="cuda"),
                      top_k=torch.full((b,), top_k, dtype=torch.int32, device="cuda"), min_p=torch.zeros(b, device="cuda"))
        got = ops.sample_tokens_rows(x, seed=seed, row_ids=ids, step=step, return_kept=True, **arrays)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (b, top_k, top_p)
        # numbers are broadcast, None switches a filter off, and asking for the log-probabilities changes neither output
        got = ops.sample_tokens_rows(x, t, top_p if top_p < 1 else None, top_k or None, None, seed=seed, row_ids=ids, step=step,
                                     return_kept=True, return_logprobs=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (b, top_k, top_p)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("v", [63, 1000, 100_003, 152_064])
def test_oracle_alone_stays_under_the_exemption_cap(dt, v):
    """(no device work) at most 2 % of the compared rows have a top-p target within TOL * Z of a cumulative-mass step"""
    ref = _mixed(dt, v)[5]
    assert sum(_near(r) for r in ref) <= 0.02 * len(ref)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("v", [63, 1000, 100_003, 152_064])
def test_mixed_batch_matches_the_oracle(dt, v):
    x, par, row_ids, seed, step, ref = _mixed(dt, v)
    tok, kept, lp = _run(x, par, row_ids, seed, step)
    n = len(ref)
    exempt = exact = 0
    worst = 0.0
    xs = x.float().numpy()
    for r, want in enumerate(ref):
        t, top_p = par["temperature"][r], par["top_p"][r]
        if want["greedy"]:
            assert tok[r] == want["token"] and kept[r] == 1, (r, tok[r], want["token"])
            exact += 1
        else:
            if top_p < 1.0 and _near(want) and kept[r] != want["kept"]:
                exempt += 1                                   # the target sits on a cumulative-mass step: fp32 exp2 decides
                continue
            assert kept[r] == want["kept"], (r, kept[r], want["kept"], {k: a[r] for k, a in par.items()})
            s = want["scores"]
            srt = np.sort(s[np.isfinite(s)])[::-1]
            gap = srt[0] - srt[1] if srt.size > 1 else float("inf")
            if gap > TOL:
                assert tok[r] == want["token"], (r, tok[r], want["token"], gap)
            else:
                assert np.isfinite(s[tok[r]]) and s[tok[r]] >= srt[0] - TOL, (r, tok[r], want["token"])
            exact += int(tok[r] == want["token"])
        # the log-probability of the token the device drew, under the oracle's set (greedy: all finite entries at T = 1)
        mask = np.isfinite(xs[r]) if want["greedy"] else want["mask"]
        lp_ref = RR.logprob(xs[r], 1.0 if want["greedy"] else t, mask, int(tok[r]))
        delta = abs(float(lp[r]) - lp_ref)
        worst = max(worst, delta)
        assert delta <= _lp_gate(lp_ref), (r, float(lp[r]), lp_ref, delta)
    print(f"sample_tokens_rows {dt} V={v}: rows {n}, exact tokens {exact}, exempt {exempt}, max |dlogprob| {worst:.3e}")
    assert exempt <= 0.02 * n, (exempt, n)
    assert exact >= 0.99 * (n - exempt), (exact, n)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_rows_are_independent(dt):
    """each row of the mixed batch (odd V) = that row alone with its parameters as numbers; = the same row at another position of a
    batch whose rows are strided and start off a 16-byte boundary"""
    from visionselector_amd import ops
    v = 1003 if dt == "fp32" else 63
    x, par, row_ids, seed, step, _ = _mixed(dt, 1000 if dt == "fp32" else 63)
    if v != x.shape[1]:
        x = torch.cat([x, x[:, :3]], dim=1)
    tok, kept, lp = _run(x, par, row_ids, seed, step)
    xd = x.cuda()
    for r in range(B):
        t1, k1, l1 = ops.sample_tokens_rows(xd[r:r + 1], par["temperature"][r], par["top_p"][r], par["top_k"][r], par["min_p"][r], seed=seed,
                                            row_ids=row_ids[r:r + 1].cuda(), step=step, return_kept=True, return_logprobs=True)
        assert (t1.item(), k1.item()) == (tok[r], kept[r]), r
        assert l1.cpu().numpy().view(np.int32)[0] == lp[r:r + 1].view(np.int32)[0], r
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3))
    wide = torch.zeros(B, v + 6, dtype=x.dtype)
    wide[:, 1:v + 1] = x[perm]
    view = wide.cuda()[:, 1:v + 1]
    assert view.data_ptr() % 16 != 0 and view.stride(0) == v + 6
    rows = perm.tolist()
    tp, kp, lpp = ops.sample_tokens_rows(view, seed=seed, row_ids=row_ids[perm].cuda(), step=step, return_kept=True, return_logprobs=True,
                                         **_device_params(par, rows))
    assert np.array_equal(tp.cpu().numpy(), tok[rows]) and np.array_equal(kp.cpu().numpy(), kept[rows])
    assert np.array_equal(lpp.cpu().numpy().view(np.int32), lp[rows].view(np.int32))


def test_ties_stay_together():
    from visionselector_amd import ops
    x = torch.full((3, 4096), -20.0)
    x[0, 100:106] = 5.0                                       # six equal maxima: min_p = 1 keeps exactly them
    x[1:, 7] = 3.0
    x[1:, 1000:1006] = 2.0                                    # d = -log2(e): exp(-1) = 0.3679 of the maximum
    xb = x.bfloat16()
    for xt in (x, xb):
        _, kept = ops.sample_tokens_rows(xt.cuda(), 1.0, min_p=torch.tensor([1.0, 0.36, 0.37], device="cuda"), return_kept=True)
        assert kept.tolist() == [6, 7, 1]                     # the threshold passes the group of six as a whole
    for r, mp in enumerate([1.0, 0.36, 0.37]):
        assert RR.sample_row(xb[r].float().numpy(), 1.0, min_p=mp)["kept"] == [6, 7, 1][r]


def test_bad_values_reject_their_row_only():
    from visionselector_amd import ops
    gen = torch.Generator().manual_seed(21)
    bad = [dict(temperature=-1.0), dict(temperature=float("nan")), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(min_p=-0.1),
           dict(min_p=2.0), dict(temperature=float("inf"))]
    n = 2 * len(bad) + 4
    par = dict(temperature=[0.8] * n, top_p=[0.9] * n, top_k=[40] * n, min_p=[0.05] * n)
    par["temperature"][1] = 0.0                               # a valid greedy row whose other values would be refused on a sampled row
    par["top_p"][1], par["top_k"][1], par["min_p"][1] = 7.0, -5, -1.0
    bad_rows = list(range(2, 2 + 2 * len(bad), 2))
    for r, kw in zip(bad_rows, bad):
        for k, val in kw.items():
            par[k][r] = val
    x = _logits(n, 1003, torch.float32, gen)
    x[n - 2, 17] = float("nan")                               # invalid logits on a sampled and on a greedy row
    x[n - 1, 500] = float("inf")
    par["temperature"][n - 1] = 0.0
    bad_rows += [n - 2, n - 1]
    ids = torch.arange(n, dtype=torch.int64) * 3
    for dtype in (torch.float32, torch.bfloat16):
        xd = x.to(dtype)
        tok, kept, lp = _run(xd, par, ids, 5, 2)
        for r in range(n):
            if r in bad_rows:
                assert tok[r] == -1 and kept[r] == 0 and math.isnan(lp[r]), (r, tok[r], kept[r], lp[r])
            else:
                t1, k1, l1 = _run(xd, par, ids, 5, 2, rows=[r])
                assert (t1[0], k1[0]) == (tok[r], kept[r]) and tok[r] >= 0 and l1.view(np.int32)[0] == lp[r:r + 1].view(np.int32)[0], r
        assert tok[1] == int(xd[1].float().argmax()) and kept[1] == 1


def test_mean_logprob_is_the_entropy_of_the_kept_distribution():
    """20 000 draws of a 6-entry row over distinct (row id, step): mean(-logprob) within 3 standard errors of the entropy"""
    from visionselector_amd import ops
    row = np.array([1.0, 2.5, -0.5, 2.0, 0.3, 1.7], dtype=np.float32)
    t, top_k = 0.8, 5
    mask, _ = RR.final_set(row, t, 1.0, top_k, 0.0)
    p = np.where(mask, np.exp2(RR.d_values(row, t).astype(np.float64)), 0.0)
    p /= p.sum()
    h = -(p[mask] * np.log(p[mask])).sum()
    se = math.sqrt(((p[mask] * np.log(p[mask]) ** 2).sum() - h * h) / 20_000)
    x = torch.from_numpy(row)[None].expand(2000, 6).contiguous().cuda()
    total = torch.zeros((), dtype=torch.float64, device="cuda")
    for step in range(10):
        tok, lp = ops.sample_tokens_rows(x, t, top_k=top_k, seed=77, step=step, return_logprobs=True)
        assert bool(mask[tok.cpu().numpy()].all())
        total -= lp.double().sum()
    assert abs(total.item() / 20_000 - h) <= 3 * se, (total.item() / 20_000, h, se)


def test_two_runs_are_bit_identical():
    x, par, row_ids, seed, step, _ = _mixed("bf16", 152_064)
    a, b = _run(x, par, row_ids, seed, step), _run(x, par, row_ids, seed, step)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
