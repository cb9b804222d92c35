"""GPU checks of flash_attn_with_kvcache / vsel_kvcache_attn_fwd (append launch + var-len attention) against the fp64 paged oracle
(oracle/attention.py, read-only) and a numpy restatement of the cache update and the rotary embedding.

Semantics restated here (flash-attn 2.7.4 docstring): new rows j of batch row b go to cache position cache_seqlens[b] + j; the
visible keys are positions [cache_leftpad[b], cache_seqlens[b] + s_new); causal masking is bottom-right aligned; new key j is
rotated at table row cache_seqlens[b] + j (with or without cache_leftpad -- the reading this library takes), query i at
cache_seqlens[b] + i when causal and at cache_seqlens[b] otherwise."""
import numpy as np
import pytest
import torch

from kvcache_ref import Case, _case, _tables, _without_row, check_all, rotate_np  # noqa: F401
import parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    assert torch.cuda.is_available()
    from visionselector_amd.flash_attn_compat import flash_attn_with_kvcache
    return flash_attn_with_kvcache


LAYOUTS = ["contig", "contig_bidx", "contig_leftpad", "paged16", "paged64", "paged256"]
HEADS = [(28, 4), (16, 2), (8, 8)]
MATRIX = [(lay, s_new, causal, hq, hkv) for lay in LAYOUTS for s_new in (0, 1, 7) for causal in (True, False) for hq, hkv in HEADS
          if (hq, hkv) == (28, 4) or s_new == 1]


@pytest.mark.parametrize("layout,s_new,causal,hq,hkv", MATRIX)
def test_kvcache_matches_oracle(fa, layout, s_new, causal, hq, hkv):
    s_q = s_new if s_new > 1 else (1 if s_new == 1 else 2)
    case = Case(layout, s_new, s_q, hq, hkv, seed=MATRIX.index((layout, s_new, causal, hq, hkv)))
    out, lse, kc, vc = case.run(fa, causal)
    assert out.shape == (case.b, s_q, hq, 128) and lse.shape == (case.b, hq, s_q) and lse.dtype == torch.float32
    check_all(case, out, lse, kc, vc, causal, f"[{layout} s_new={s_new} causal={causal} {hq}/{hkv}]")


@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("rotary_dim", [64, 128])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("layout", ["paged64", "contig_leftpad"])
def test_kvcache_rotary(fa, interleaved, rotary_dim, causal, layout):
    cos, sin = _tables(400, rotary_dim)
    case = Case(layout, 3, 3, 8, 2, seed=rotary_dim + 7 * interleaved + 3 * causal, rotary=(cos, sin, interleaved))
    out, lse, kc, vc = case.run(fa, causal)
    check_all(case, out, lse, kc, vc, causal, f"[rotary {layout} rd={rotary_dim} inter={interleaved} causal={causal}]", rotary=True)


def test_kvcache_int_seqlens_and_default_scale_equal_tensor_form(fa):
    """cache_seqlens as a Python int is broadcast; an explicit softmax_scale of d^-0.5 is the default."""
    case = Case("paged64", 1, 1, 16, 2, seed=5, ends=[37, 37, 37])
    a, la, ka, va = case.run(fa, True)
    b, lb, kb, vb = case.run(fa, True, seqlens_as_int=True, softmax_scale=128 ** -0.5)
    assert torch.equal(a, b) and torch.equal(la, lb) and torch.equal(ka, kb) and torch.equal(va, vb)


def test_kvcache_is_deterministic(fa):
    case = Case("paged16", 7, 7, 28, 4, seed=11)
    a, la, ka, va = case.run(fa, True)
    b, lb, kb, vb = case.run(fa, True)
    assert torch.equal(a, b) and torch.equal(la, lb) and torch.equal(ka, kb) and torch.equal(va, vb)


@pytest.mark.parametrize("layout", ["paged64", "contig_bidx"])
def test_kvcache_decode_step_is_graph_capturable(fa, layout):
    """Append + attention captured on one stream; replayed after cache_seqlens and the static inputs were advanced ON THE
    DEVICE, it matches the eager call: nothing in the path reads a device value on the host."""
    case = Case(layout, 1, 1, 28, 4, seed=21, batch=4, ends=[5, 70, 129, 250])
    kc, vc = case.kc.cuda(), case.vc.cuda()
    bt, bidx = case.dev(case.block_table), case.dev(case.batch_idx)
    q_s, k_s, v_s = case.q.cuda(), case.k.cuda(), case.v.cuda()
    seq_s = torch.tensor(case.ends, dtype=torch.int32).cuda()
    call = lambda q, k, v, sl, kc_, vc_: fa(q, kc_, vc_, k=k, v=v, cache_seqlens=sl, block_table=bt, cache_batch_idx=bidx,  # noqa: E731
                                            causal=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(q_s, k_s, v_s, seq_s, kc, vc)                # warm-up (also a real step: writes position ends[b])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out_g = call(q_s, k_s, v_s, seq_s, kc, vc)
    g = torch.Generator().manual_seed(3)
    q1, k1, v1 = (torch.randn(t.shape, generator=g).bfloat16().cuda() for t in (q_s, k_s, v_s))
    q_s.copy_(q1)
    k_s.copy_(k1)
    v_s.copy_(v1)
    seq_s.add_(1)                                          # advanced on the device
    kc_ref, vc_ref = kc.clone(), vc.clone()
    ref = call(q1, k1, v1, seq_s.clone(), kc_ref, vc_ref)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_g, ref) and torch.equal(kc, kc_ref) and torch.equal(vc, vc_ref)
    assert float(ref.float().abs().max()) > 0


@pytest.mark.parametrize("layout", ["contig", "paged16"])
def test_kvcache_overflowing_row_stays_inside_the_cache(fa, layout):
    """The caches are views inside one larger buffer whose guard regions hold a sentinel.  Row 1 asks for positions past its
    capacity (L_cache, or its allocated pages): the other rows are exact, and no guard element changes."""
    hq, hkv, d, s_new = 8, 2, 128, 7
    case = Case(layout, s_new, s_new, hq, hkv, seed=31, ends=[10, 100, 40])
    if layout == "contig":
        case.ends[1] = case.kc.shape[1] - 3                  # 3 rows fit, 4 do not
    else:
        bt = case.block_table.clone()
        n = int((bt[1] >= 0).sum())
        case.ends[1] = n * case.page - 2                      # the last 5 new rows would land past the allocated pages
    guard = 4096
    sentinel = torch.tensor(-12345.0).bfloat16()
    caches = []
    for c in (case.kc, case.vc):
        buf = torch.full((c.numel() + 2 * guard,), float(sentinel), dtype=torch.bfloat16).cuda()
        view = buf[guard:guard + c.numel()].view(c.shape)
        view.copy_(c.cuda())
        caches.append((buf, view))
    (kbuf, kc), (vbuf, vc) = caches
    out, lse, _, _ = case.run(fa, True, kc=kc, vc=vc)
    torch.cuda.synchronize()
    for buf in (kbuf, vbuf):
        assert bool((buf[:guard] == sentinel).all()) and bool((buf[-guard:] == sentinel).all())
    # rows 0 and 2 exactly as specified (the expected caches restricted to their rows; row 1 is the caller error)
    ek, ev = _without_row(case, 1).expected_caches()
    kf, ekf = kc.cpu().view(-1, hkv, d), ek.view(-1, hkv, d)
    for b in (0, 2):
        for p in range(case.ends[b] + s_new):
            r = case.row_of(b, p)
            assert torch.equal(kf[r], ekf[r]), (b, p)
    # row 1 wrote only inside its capacity: every element outside rows 1's own positions is unchanged
    own = {case.row_of(1, p) for p in range(case.ends[1], case.ends[1] + s_new)
           if (layout == "contig" and p < case.kc.shape[1]) or (layout != "contig" and p // case.page < int((case.block_table[1] >= 0).sum()))}
    others = torch.ones(kf.shape[0], dtype=torch.bool)
    others[list(own)] = False
    assert torch.equal(kf[others], ekf[others])
    ref, _ = case.oracle(kc.cpu(), vc.cpu(), True)
    got = out.float().cpu().numpy().reshape(ref.shape)
    for b in (0, 2):
        sl = slice(b * s_new, (b + 1) * s_new)
        parity.check_fwd(_case() + f"[row {b}]", got[sl].astype(np.float64), ref[sl])
