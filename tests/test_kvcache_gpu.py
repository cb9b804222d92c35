"""GPU checks of flash_attn_with_kvcache / vsel_kvcache_attn_fwd (append launch + var-len attention) against the fp64 paged oracle
(oracle/attention.py, read-only) and a numpy restatement of the cache update and the rotary embedding.

Semantics restated here (flash-attn 2.7.4 docstring): new rows j of batch row b go to cache position cache_seqlens[b] + j; the
visible keys are positions [cache_leftpad[b], cache_seqlens[b] + s_new); causal masking is bottom-right aligned; new key j is
rotated at table row cache_seqlens[b] + j (with or without cache_leftpad -- the reading this library takes), query i at
cache_seqlens[b] + i when causal and at cache_seqlens[b] otherwise."""
import numpy as np
import pytest
import torch

from oracle import attention as oattn
import parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    assert torch.cuda.is_available()
    from visionselector_amd.flash_attn_compat import flash_attn_with_kvcache
    return flash_attn_with_kvcache


def _case():
    import os
    return os.environ.get("PYTEST_CURRENT_TEST", "?").split("::")[-1].split(" ")[0]


def rotate_np(x, cos, sin, pos, interleaved):
    """x float32 [..., d] at table row pos; fp32 arithmetic, one bf16 rounding (returns a bf16 torch tensor)."""
    x = np.asarray(x, np.float32).copy()
    half = cos.shape[1]
    rd = 2 * half
    c, s = cos[pos].astype(np.float32), sin[pos].astype(np.float32)
    if interleaved:
        x1, x2 = x[..., 0:rd:2].copy(), x[..., 1:rd:2].copy()
        x[..., 0:rd:2], x[..., 1:rd:2] = x1 * c - x2 * s, x1 * s + x2 * c
    else:
        x1, x2 = x[..., :half].copy(), x[..., half:rd].copy()
        x[..., :half], x[..., half:rd] = x1 * c - x2 * s, x1 * s + x2 * c
    return torch.from_numpy(x).bfloat16()


class Case:
    """One batch against one cache layout; everything on the host until .dev()."""

    def __init__(self, layout, s_new, s_q, hq, hkv, seed, d=128, batch=3, ends=None, rotary=None):
        rng = np.random.default_rng(seed)
        self.layout, self.s_new, self.s_q, self.hq, self.hkv, self.d, self.b = layout, s_new, s_q, hq, hkv, d, batch
        f = lambda *sh: torch.from_numpy(rng.standard_normal(sh, dtype=np.float32)).bfloat16()  # noqa: E731
        L = 300
        if ends is None:
            ends = [int(rng.integers(0, L - s_new + 1)) for _ in range(batch)]
            ends[0] = 0 if s_new == 0 else ends[0]            # s_new == 0: one row without any key
            ends[-1] = L - s_new                             # one row filled to its capacity
        self.ends = ends
        self.batch_idx = self.leftpad = self.block_table = None
        if layout.startswith("paged"):
            self.page = int(layout[5:])
            need = [-(-(e + s_new) // self.page) for e in ends]
            n_blocks = sum(need) + 5
            perm = rng.permutation(n_blocks)
            width = max(max(need), 1) + 2
            bt = np.full((batch, width), -1, np.int32)        # -1-padded, scattered pages
            cur = 0
            for b, n in enumerate(need):
                bt[b, :n] = perm[cur:cur + n]
                cur += n
            self.block_table = torch.from_numpy(bt)
            self.kc, self.vc = f(n_blocks, self.page, hkv, d), f(n_blocks, self.page, hkv, d)
        else:
            rows = batch + (3 if layout == "contig_bidx" else 0)
            self.kc, self.vc = f(rows, L, hkv, d), f(rows, L, hkv, d)
            if layout == "contig_bidx":
                self.batch_idx = torch.from_numpy(rng.permutation(rows)[:batch].astype(np.int32))
            if layout == "contig_leftpad":
                lp = [int(rng.integers(0, e + s_new + 1)) for e in ends]
                lp[1] = ends[1] + s_new                      # one row whose keys are all padding
                self.leftpad = torch.tensor(lp, dtype=torch.int32)
        self.q = f(batch, s_q, hq, d)
        self.k = f(batch, s_new, hkv, d) if s_new else None
        self.v = f(batch, s_new, hkv, d) if s_new else None
        self.rotary = rotary                                  # (cos, sin, interleaved) numpy fp32 tables or None

    def row_of(self, b, p):
        """flat cache row ([*, Hkv, d] units) of position p of batch row b"""
        if self.block_table is not None:
            return int(self.block_table[b, p // self.page]) * self.page + p % self.page
        r = int(self.batch_idx[b]) if self.batch_idx is not None else b
        return r * self.kc.shape[1] + p

    def expected_caches(self):
        kc, vc = self.kc.clone(), self.vc.clone()
        kf, vf = kc.view(-1, self.hkv, self.d), vc.view(-1, self.hkv, self.d)
        for b in range(self.b):
            for j in range(self.s_new):
                p = self.ends[b] + j
                kn = self.k[b, j]
                if self.rotary is not None:
                    cos, sin, inter = self.rotary
                    kn = rotate_np(kn.float().numpy(), cos, sin, p, inter)
                kf[self.row_of(b, p)] = kn
                vf[self.row_of(b, p)] = self.v[b, j]
        return kc, vc

    def rotated_q(self, causal):
        if self.rotary is None:
            return self.q
        cos, sin, inter = self.rotary
        q = self.q.clone()
        for b in range(self.b):
            for i in range(self.s_q):
                q[b, i] = rotate_np(self.q[b, i].float().numpy(), cos, sin, self.ends[b] + (i if causal else 0), inter)
        return q

    def oracle(self, kc, vc, causal, scale=None):
        """-> (out fp64 [B * s_q, Hq, d], lse fp64 [B, Hq, s_q]) over the visible keys of the UPDATED caches kc / vc"""
        lp = self.leftpad.tolist() if self.leftpad is not None else [0] * self.b
        vis = [list(range(lp[b], self.ends[b] + self.s_new)) for b in range(self.b)]
        kmax = max(1, max(len(x) for x in vis))
        kf, vf = kc.view(-1, self.hkv, self.d).double().numpy(), vc.view(-1, self.hkv, self.d).double().numpy()
        kp = np.zeros((self.b, kmax, self.hkv, self.d))
        vp = np.zeros((self.b, kmax, self.hkv, self.d))
        for b in range(self.b):
            rows = [self.row_of(b, p) for p in vis[b]]
            kp[b, :len(rows)], vp[b, :len(rows)] = kf[rows], vf[rows]
        q = self.rotated_q(causal).double().numpy()
        cu_q = np.arange(0, (self.b + 1) * self.s_q, self.s_q)
        nk = np.array([len(x) for x in vis])
        out = oattn.paged_attention(q.reshape(-1, self.hq, self.d), kp, vp, cu_q, nk, np.arange(self.b)[:, None], causal=causal,
                                    softmax_scale=scale)
        scale = scale if scale is not None else self.d ** -0.5
        rep = self.hq // self.hkv
        lse = np.full((self.b, self.hq, self.s_q), -np.inf)
        for b in range(self.b):
            for h in range(self.hq):
                s = q[b, :, h] @ kp[b, :nk[b], h // rep].T * scale
                for i in range(self.s_q):
                    lim = min(nk[b], i + 1 + nk[b] - self.s_q) if causal else nk[b]
                    if lim > 0:
                        m = s[i, :lim].max()
                        lse[b, h, i] = m + np.log(np.exp(s[i, :lim] - m).sum())
        return out, lse

    def dev(self, t):
        return None if t is None else t.cuda()

    def run(self, fa, causal, kc=None, vc=None, seqlens_as_int=False, **kw):
        kc = self.kc.cuda() if kc is None else kc
        vc = self.vc.cuda() if vc is None else vc
        rot = {}
        if self.rotary is not None:
            cos, sin, inter = self.rotary
            rot = dict(rotary_cos=torch.from_numpy(cos).cuda(), rotary_sin=torch.from_numpy(sin).cuda(), rotary_interleaved=inter)
        seqlens = self.ends[0] if seqlens_as_int else torch.tensor(self.ends, dtype=torch.int32).cuda()
        q = self.q.cuda()
        out, lse = fa(q, kc, vc, k=self.dev(self.k), v=self.dev(self.v), cache_seqlens=seqlens, cache_batch_idx=self.dev(self.batch_idx),
                      cache_leftpad=self.dev(self.leftpad), block_table=self.dev(self.block_table), causal=causal,
                      return_softmax_lse=True, **rot, **kw)
        assert torch.equal(q.cpu(), self.q)                  # q is never modified
        return out, lse, kc, vc


LAYOUTS = ["contig", "contig_bidx", "contig_leftpad", "paged16", "paged64", "paged256"]
HEADS = [(28, 4), (16, 2), (8, 8)]
MATRIX = [(lay, s_new, causal, hq, hkv) for lay in LAYOUTS for s_new in (0, 1, 7) for causal in (True, False) for hq, hkv in HEADS
          if (hq, hkv) == (28, 4) or s_new == 1]


def check_all(case, got_out, got_lse, kc, vc, causal, tag, rotary=False):
    ek, ev = case.expected_caches()
    kc, vc = kc.cpu(), vc.cpu()
    if rotary:     # new rows within one bf16 ulp (fp32 rotation, fused or not), every other element bit-identical
        diff = (kc.float() - ek.float()).abs()
        assert float((diff / torch.from_numpy(parity.bf16_ulp(ek.float().abs().numpy()))).max()) <= 1.0, tag
        changed = torch.zeros(kc.view(-1, case.hkv, case.d).shape[0], dtype=torch.bool)
        for b in range(case.b):
            for j in range(case.s_new):
                changed[case.row_of(b, case.ends[b] + j)] = True
        assert torch.equal(kc.view(-1, case.hkv, case.d)[~changed], ek.view(-1, case.hkv, case.d)[~changed]), tag
        ek = kc                                                   # the attention saw the kernel's rotated keys
    else:
        assert torch.equal(kc.view(torch.int16), ek.view(torch.int16)), tag
    assert torch.equal(vc.view(torch.int16), ev.view(torch.int16)), tag
    ref, ref_lse = case.oracle(ek, ev, causal)
    parity.check_fwd(_case() + tag, got_out.float().cpu().numpy().reshape(ref.shape).astype(np.float64), ref)
    got_lse = got_lse.cpu().double().numpy()
    assert got_lse.shape == ref_lse.shape
    fin = np.isfinite(ref_lse)
    assert np.array_equal(np.isfinite(got_lse), fin) and np.all(got_lse[~fin] == -np.inf), tag
    assert np.abs(got_lse[fin] - ref_lse[fin]).max(initial=0.0) <= 2e-3, tag
    # rows without a visible key output zeros
    zero_rows = torch.from_numpy(np.ascontiguousarray(~fin.transpose(0, 2, 1).reshape(-1, case.hq)))
    if bool(zero_rows.any()):
        assert float(got_out.reshape(-1, case.hq, case.d).cpu()[zero_rows].float().abs().max()) == 0.0, tag


@pytest.mark.parametrize("layout,s_new,causal,hq,hkv", MATRIX)
def test_kvcache_matches_oracle(fa, layout, s_new, causal, hq, hkv):
    s_q = s_new if s_new > 1 else (1 if s_new == 1 else 2)
    case = Case(layout, s_new, s_q, hq, hkv, seed=MATRIX.index((layout, s_new, causal, hq, hkv)))
    out, lse, kc, vc = case.run(fa, causal)
    assert out.shape == (case.b, s_q, hq, 128) and lse.shape == (case.b, hq, s_q) and lse.dtype == torch.float32
    check_all(case, out, lse, kc, vc, causal, f"[{layout} s_new={s_new} causal={causal} {hq}/{hkv}]")


def _tables(seqlen_ro, rotary_dim, dtype=np.float32):
    inv = 1.0 / (10000.0 ** (np.arange(0, rotary_dim, 2, dtype=np.float32) / rotary_dim))
    ang = np.arange(seqlen_ro, dtype=np.float32)[:, None] * inv[None, :]
    return np.cos(ang).astype(dtype), np.sin(ang).astype(dtype)


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


def _without_row(case, drop):
    """a shallow copy of `case` whose row `drop` appends nothing (for the expected caches of the other rows)"""
    import copy
    c = copy.copy(case)
    k, v = case.k.clone(), case.v.clone()

    class _C(Case):
        def expected_caches(self):
            kc, vc = self.kc.clone(), self.vc.clone()
            kf, vf = kc.view(-1, self.hkv, self.d), vc.view(-1, self.hkv, self.d)
            for b in range(self.b):
                if b == drop:
                    continue
                for j in range(self.s_new):
                    kf[self.row_of(b, self.ends[b] + j)] = k[b, j]
                    vf[self.row_of(b, self.ends[b] + j)] = v[b, j]
            return kc, vc
    c.__class__ = _C
    return c
