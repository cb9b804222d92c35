"""CPU checks of tests/kvcache_ref.py, the reference the KV-cache GPU tests compare vsel_kvcache_attn_fwd against: its rotation against
an independent float64 complex rotation, its attention oracle against oracle/attention.py's varlen_attention, its stride forms
against the packed tensors, and its token-per-row prefill form against whole-prompt appends."""
import numpy as np
import pytest
import torch

from kvcache_ref import Case, PAD_VALUE, STRIDES, _tables, as_layout, layout_strides, rotate_np, token_rows, whole_prompt_caches
from oracle import attention as oattn
import parity

# every (head dim, rotary_dim) the GPU tests rotate at (tests/test_kvcache_gpu.py, tests/test_kvcache_forms_gpu.py)
ROTARY_DIMS = [(80, 80), (80, 20), (80, 2), (64, 64), (64, 32), (128, 128), (128, 64), (128, 100), (128, 20), (128, 2)]


@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("d,rotary_dim", ROTARY_DIMS)
def test_rotate_np_matches_a_float64_complex_rotation(d, rotary_dim, interleaved):
    """(x1 + i x2) exp(i theta) in float64, theta the angle whose float64 cosine / sine the fp32 table rows are rounded from:
    rotate_np (fp32 products, one bf16 rounding) lands within one bf16 ulp of it -- the gate check_all then applies to the
    kernel's rows -- and the elements from rotary_dim on come back bit for bit."""
    rng = np.random.default_rng(1000 * d + 2 * rotary_dim + interleaved)
    half = rotary_dim // 2
    inv = 1.0 / (10000.0 ** (np.arange(0, rotary_dim, 2, dtype=np.float64) / rotary_dim))
    theta = np.arange(400, dtype=np.float64)[:, None] * inv[None, :]
    cos, sin = np.cos(theta).astype(np.float32), np.sin(theta).astype(np.float32)
    x = torch.from_numpy(rng.standard_normal((6, d), dtype=np.float32)).bfloat16()
    for pos in (0, 1, 37, 299):
        got = rotate_np(x.float().numpy(), cos, sin, pos, interleaved)
        x64 = x.double().numpy()
        if interleaved:
            i1, i2 = np.arange(0, rotary_dim, 2), np.arange(1, rotary_dim, 2)
        else:
            i1, i2 = np.arange(half), np.arange(half, rotary_dim)
        z = (x64[:, i1] + 1j * x64[:, i2]) * np.exp(1j * theta[pos])[None, :]
        ref = x64.copy()
        ref[:, i1], ref[:, i2] = z.real, z.imag
        err = np.abs(got.double().numpy() - ref) / parity.bf16_ulp(np.abs(ref))
        assert err.max() <= 1.0, (pos, float(err.max()))
        assert torch.equal(got[:, rotary_dim:].view(torch.int16), x[:, rotary_dim:].view(torch.int16))
        if pos == 0:                                           # angle 0: the identity, bit for bit
            assert torch.equal(got.view(torch.int16), x.view(torch.int16))


def test_rotate_np_clamps_the_table_row_and_reads_bf16_tables_as_rounded():
    cos, sin = _tables(50, 64)
    x = np.random.default_rng(3).standard_normal((4, 128), dtype=np.float32)
    for inter in (True, False):
        assert torch.equal(rotate_np(x, cos, sin, 49, inter), rotate_np(x, cos, sin, 300, inter))
        assert torch.equal(rotate_np(x, cos, sin, 0, inter), rotate_np(x, cos, sin, -4, inter))
        assert not torch.equal(rotate_np(x, cos, sin, 48, inter), rotate_np(x, cos, sin, 49, inter))
    case = Case("paged64", 3, 3, 8, 2, seed=1, rotary=(cos, sin, True), table_dtype="bf16")
    c16 = torch.from_numpy(cos).bfloat16()
    assert np.array_equal(case.rotary[0], c16.float().numpy()) and not np.array_equal(case.rotary[0], cos)
    t = case.tables()
    assert t["rotary_cos"].dtype == torch.bfloat16 and torch.equal(t["rotary_cos"], c16) and t["rotary_interleaved"] is True
    ek, _ = case.expected_caches()                            # the new rows are rotated with the ROUNDED table
    p = case.ends[0]
    want = rotate_np(case.k[0, 0].float().numpy(), c16.float().numpy(), torch.from_numpy(sin).bfloat16().float().numpy(), p, True)
    assert torch.equal(ek.view(-1, 2, 128)[case.row_of(0, p)], want)


def _per_row_varlen(case, kc, vc, causal, scale):
    """The Case oracle's output restated through oracle/attention.py's varlen_attention, one square call per batch row (and chunk
    of queries) on the gathered visible keys.  varlen_attention takes as many queries as keys, so the row's queries sit at the
    END of a call padded in front with zero queries: under its top-left causal mask the last rows of a square call see what
    bottom-right alignment gives them, and a query that sees no key (more queries than keys) outputs zeros."""
    kf, vf = kc.view(-1, case.hkv, case.d).double().numpy(), vc.view(-1, case.hkv, case.d).double().numpy()
    q = case.rotated_q(causal).double().numpy()
    out = np.zeros((case.b, case.s_q, case.hq, case.d))
    for b, vis in enumerate(case.visible()):
        nk = len(vis)
        if nk == 0:
            continue
        rows = [case.row_of(b, p) for p in vis]
        if causal:                    # the last min(s_q, nk) queries against all keys; the earlier ones see nothing
            chunks = [(max(0, case.s_q - nk), case.s_q)]
        else:                         # every query sees every key: chunks of at most nk queries
            chunks = [(a, min(a + nk, case.s_q)) for a in range(0, case.s_q, nk)]
        for a, e in chunks:
            qq = np.zeros((nk, case.hq, case.d))
            qq[nk - (e - a):] = q[b, a:e]
            o = oattn.varlen_attention(qq, kf[rows], vf[rows], np.array([0, nk]), causal=causal, softmax_scale=scale)
            out[b, a:e] = o[nk - (e - a):]
    return out.reshape(-1, case.hq, case.d)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("layout,s_q,s_new", [("contig_leftpad", 5, 2), ("contig_leftpad", 1, 4), ("contig_bidx_leftpad", 2, 0),
                                              ("paged16", 5, 2)])
def test_case_oracle_matches_varlen_attention_per_row(layout, s_q, s_new, causal):
    """cache_leftpad, s_q != s_new and a non-default scale: float64 against float64."""
    case = Case(layout, s_new, s_q, 8, 2, seed=41 + s_q, d=80, batch=4, L=40, ends=[0, 3, 11, 40 - s_new])
    if case.leftpad is not None:
        lp = case.leftpad.tolist()
        lp[0], lp[2] = 0, case.ends[2] + s_new - 2            # row 0: at most s_new keys (fewer keys than queries); row 2: two keys
        case.leftpad = torch.tensor(lp, dtype=torch.int32)
    kc, vc = case.expected_caches()
    got, lse = case.oracle(kc, vc, causal, scale=0.2)
    ref = _per_row_varlen(case, kc, vc, causal, 0.2)
    assert np.abs(got - ref).max() <= 1e-12
    assert float(np.abs(ref).max()) > 0.1
    # rows without a visible key: zeros and lse -inf, and only those
    none = ~np.isfinite(lse).transpose(0, 2, 1).reshape(-1, case.hq)
    assert np.all(got[none] == 0) and np.all(np.abs(got[~none]).max(axis=-1) > 0)
    if case.leftpad is not None:
        assert none.reshape(case.b, case.s_q, case.hq)[1].all()          # the all-padding row
    # the scale is used: the default one gives another result
    assert np.abs(case.oracle(kc, vc, causal)[0] - got).max() > 1e-3


@pytest.mark.parametrize("strides", STRIDES)
@pytest.mark.parametrize("d", [64, 80, 128])
def test_stride_forms_hold_the_packed_values_at_the_promised_strides(strides, d):
    case = Case("paged16", 3, 2, 6, 2, seed=7, d=d, batch=5)
    q, k, v = case.views(strides)
    for name, view, packed in (("q", q, case.q), ("k", k, case.k), ("v", v, case.v)):
        assert view.shape == packed.shape and torch.equal(view, packed)
        b, s, h, _ = packed.shape
        assert view.stride() == layout_strides(strides, name, packed.shape) + (1,)
        assert all(x % 8 == 0 for x in view.stride()[:3])     # 16-byte rows: what the entry requires
        assert view.is_contiguous() == (strides == "packed")
    if strides == "head_major":
        # exactly generate.vsel_paged_attention_forward's views: [1, H, T, d].permute(2, 0, 1, 3) for one token per batch row
        one = Case("paged16", 1, 1, 6, 2, seed=8, d=d, batch=5)
        hm = torch.empty(1, 6, 5, d, dtype=torch.bfloat16).copy_(one.q.permute(1, 2, 0, 3)).permute(2, 0, 1, 3)
        got = as_layout(one.q, "head_major", "q")
        assert got.stride() == hm.stride() == (d, 6 * 5 * d, 5 * d, 1) and torch.equal(got, hm)
    if strides == "padded":
        assert k.stride(0) != v.stride(0) and k.stride(2) == d + 8 and k.stride(1) == 2 * case.k.shape[2] * d
        # the gaps hold the pad value, which no packed element has
        assert float(case.k.float().abs().max()) < PAD_VALUE
        assert int((k.as_strided((k.untyped_storage().nbytes() // 2,), (1,)) == PAD_VALUE).sum()) > 0
    assert as_layout(None, strides, "k") is None


@pytest.mark.parametrize("lengths,layout", [([1, 17, 130], "paged16"), ([64, 65], "paged64"), ([5, 1, 33], "contig_bidx")])
def test_token_rows_equal_whole_prompt_appends(lengths, layout):
    c = token_rows(lengths, layout, 2, seed=13, d=64)
    t = sum(lengths)
    assert c.q is None and c.b == t and c.s_new == 1 and c.k.shape == (t, 1, 2, 64)
    assert c.ends == [j for n in lengths for j in range(n)]
    if layout.startswith("paged"):
        assert c.block_table.shape[0] == t and c.block_table.is_contiguous()
        for i, p in enumerate(c.tok_prompt):
            assert torch.equal(c.block_table[i], c.prompt_table[p])
    else:
        assert c.batch_idx.tolist() == [int(c.prompt_rows[p]) for p in c.tok_prompt]
    ek, ev = c.expected_caches()
    wk, wv = whole_prompt_caches(c)
    assert torch.equal(ek.view(torch.int16), wk.view(torch.int16)) and torch.equal(ev.view(torch.int16), wv.view(torch.int16))
    changed = (ek.view(-1, 2 * 64) != c.kc.view(-1, 2 * 64)).any(dim=1)
    assert int(changed.sum()) == t                            # exactly one cache row per token
