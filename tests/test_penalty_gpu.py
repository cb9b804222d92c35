"""vsel_repetition_penalty / vsel_token_sets_build on the MI355X against transformers' RepetitionPenaltyLogitsProcessor run on the GPU:
the fp32 output bit for bit (NaN positions compared apart), the greedy token as torch.argmax of HF's output (ties, +-0, +-inf, NaN),
set edge cases, and several launches with permuted / compacted row ids and previous tokens."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _hf(x, ids_per_row, theta):
    """HF's processor on the GPU, row by row (rows have different id counts): the fp32 copy as generate() makes it"""
    from transformers import RepetitionPenaltyLogitsProcessor
    proc = RepetitionPenaltyLogitsProcessor(penalty=float(theta))
    s = x.float().clone()
    rows = []
    for r, ids in enumerate(ids_per_row):
        ids = torch.as_tensor(ids, dtype=torch.int64, device=x.device).reshape(1, -1)
        rows.append(proc(ids, s[r:r + 1]) if ids.numel() else s[r:r + 1])
    return torch.cat(rows)


def _same(got, want):
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    assert torch.equal(nan_g, nan_w)
    assert torch.equal(torch.where(nan_g, 0.0, got), torch.where(nan_w, 0.0, want))
    assert torch.equal(torch.signbit(got[~nan_g]), torch.signbit(want[~nan_w]))          # -0.0 stays -0.0


def _rows(b, v, dtype, gen, strided):
    x = torch.randn(b, v + (5 if strided else 0), device="cuda", generator=gen) * 4
    x = x.to(dtype)
    return x[:, 3:3 + v] if strided else x


def _ids(b, v, gen, n=40):
    return [torch.randint(0, v, (int(torch.randint(0, n, (1,), generator=gen)),), generator=gen).tolist() for _ in range(b)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("v", [1, 63, 1000, 151_936, 152_064])
@pytest.mark.parametrize("b", [1, 7, 64])
@pytest.mark.parametrize("theta", [1.05, 1.2, 0.8])
@pytest.mark.parametrize("strided", [False, True])
def test_matches_hf_processor_bit_for_bit(dtype, v, b, theta, strided):
    from visionselector_amd import ops
    g = torch.Generator(device="cpu").manual_seed(v * 131 + b * 7 + int(theta * 100) + strided)
    gd = torch.Generator(device="cuda").manual_seed(v + b)
    x = _rows(b, v, dtype, gd, strided)
    ids = _ids(b, v, g, n=min(3 * v, 2400))
    sets = ops.token_sets([torch.tensor(i, dtype=torch.int64) for i in ids], v, "cuda")
    want = _hf(x, ids, theta)
    y, tok = ops.repetition_penalty(x, theta, sets, out=torch.empty(b, v, device="cuda"), return_tokens=True)
    _same(y, want)
    assert torch.equal(tok, want.argmax(-1))
    assert torch.equal(ops.repetition_penalty(x, theta, sets), y)
    assert torch.equal(ops.repetition_penalty(x, theta, sets, return_tokens=True), tok)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_greedy_tie_and_special_values(dtype):
    """rows built so that the argmax is decided by ties, +-0.0, +-inf and NaN, before and after the penalty"""
    from visionselector_amd import ops
    v = 1000
    nan, inf = float("nan"), float("inf")
    cases = [  # (entries {index: value}, fill, ids)
        ({5: 2.0, 9: 2.0, 700: 2.0}, -1.0, []),                          # equal maxima: the lowest index
        ({5: 2.1, 9: 2.0}, -1.0, [5]),                                     # the penalty makes 9 the maximum
        ({5: 0.0, 9: -0.0, 3: -0.0}, -1.0, []),                            # +0 == -0: index 3
        ({5: 0.0, 9: -0.0, 3: -0.0}, -1.0, [3, 5, 9]),                     # -0 stays -0 and still ties with +0
        ({}, -inf, []),                                                    # all -inf: index 0
        ({17: -inf}, -2.0, [17]),                                          # -inf * theta stays -inf
        ({40: inf, 41: inf}, 0.5, [40]),                                   # +inf / theta stays +inf: the first +inf
        ({40: 3.0, 600: nan, 800: nan}, 0.5, []),                          # NaN is the largest: the first NaN
        ({40: 3.0, 600: nan, 800: nan}, 0.5, [600]),                       # NaN stays NaN
        ({999: 1.0}, 0.0, [999]),                                          # a penalised positive maximum at V - 1 stays the maximum
        ({0: 5.0, 999: 5.0}, 0.0, [0]),                                    # the penalty on index 0 hands the tie to V - 1
    ]
    x = torch.empty(len(cases), v, device="cuda")
    for r, (ent, fill, _) in enumerate(cases):
        x[r].fill_(fill)
        for i, val in ent.items():
            x[r, i] = val
    x = x.to(dtype)
    ids = [c[2] for c in cases]
    sets = ops.token_sets([torch.tensor(i, dtype=torch.int64) for i in ids], v, "cuda")
    for theta in (1.3, 0.8):
        want = _hf(x, ids, theta)
        y, tok = ops.repetition_penalty(x, theta, sets, out=torch.empty(len(cases), v, device="cuda"), return_tokens=True)
        _same(y, want)
        assert tok.tolist() == want.argmax(-1).tolist(), theta


def test_set_edge_cases():
    """empty set, duplicates, ids 0 and V - 1, all V ids; sets with unequal sizes in one build"""
    from visionselector_amd import ops
    v = 1001
    ids = [[], [7, 7, 7, 0, 0], [0, v - 1], list(range(v)), list(range(v - 1, -1, -3)) * 2]
    sets = ops.token_sets(ids, v, "cuda")
    words = sets.cpu().view(torch.uint8).numpy()
    for s, i in enumerate(ids):
        bits = {k for k in range(v) if (words[s, k >> 3] >> (k & 7)) & 1}                    # (little-endian uint32 words)
        assert bits == set(i), s
    x = torch.randn(len(ids), v, device="cuda")
    _same(ops.repetition_penalty(x, 1.2, sets), _hf(x, ids, 1.2))
    empty = ops.token_sets([], v, "cuda")
    assert empty.shape == (0, (v + 31) // 32)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_multi_step_permuted_and_compacted_rows(dtype):
    """Several launches as packed_generate makes them: row ids permuted, then compacted as prompts leave; each launch's prev_tokens
    join the sets.  At step s a row equals HF's processor on its prompt ids followed by the tokens of steps < s."""
    from visionselector_amd import ops
    v, n = 5000, 6
    g = torch.Generator().manual_seed(11)
    gd = torch.Generator(device="cuda").manual_seed(12)
    prompts = [torch.randint(0, v, (int(torch.randint(5, 300, (1,), generator=g)),), generator=g) for _ in range(n)]
    sets = ops.token_sets(prompts, v, "cuda")
    history = [p.tolist() for p in prompts]
    active = [3, 0, 5, 1, 4, 2]                                        # permuted
    prev = None
    for step in range(8):
        if step == 3:
            active = [a for a in active if a not in (0, 4)]           # two prompts leave
        if step == 5:
            active = active[:1] + active[2:]
        rid = torch.tensor(active, dtype=torch.int64, device="cuda")
        x = (torch.randn(len(active), v, device="cuda", generator=gd) * 3).to(dtype)
        if step % 2:   # make the previous token (and an old one) win unless penalised
            for r, a in enumerate(active):
                x[r, history[a][-1]] = 40.0
        want = _hf(x, [history[a] for a in active], 1.5)
        prev_t = None if prev is None else torch.tensor([prev[a] for a in active], dtype=torch.int64, device="cuda")
        if step % 2:
            y, tok = ops.repetition_penalty(x, 1.5, sets, row_ids=rid, prev_tokens=prev_t, out=torch.empty(len(active), v, device="cuda"),
                                            return_tokens=True)
            _same(y, want)
        else:
            tok = ops.repetition_penalty(x, 1.5, sets, row_ids=rid, prev_tokens=prev_t, return_tokens=True)
        assert torch.equal(tok, want.argmax(-1)), step
        # the next step's previous tokens: a random id (sometimes one already in the set)
        prev = {}
        for a in active:
            t = int(torch.randint(0, v, (1,), generator=g)) if step % 3 else history[a][0]
            prev[a] = t
            history[a].append(t)
    # the last tokens are in the sets only once a launch has taken them as prev_tokens
    rid = torch.tensor(active, dtype=torch.int64, device="cuda")
    ops.repetition_penalty(torch.zeros(len(active), v, device="cuda"), 1.5, sets, row_ids=rid,
                           prev_tokens=torch.tensor([prev[a] for a in active], dtype=torch.int64, device="cuda"), return_tokens=True)
    words = sets.cpu().view(torch.uint8).numpy()
    for a in active:
        bits = {k for k in range(v) if (words[a, k >> 3] >> (k & 7)) & 1}
        assert bits == set(history[a]), a
