"""numpy / torch-CPU reference of flash_attn_with_kvcache (vsel_kvcache_attn_fwd: append launch + var-len attention) and the case
builder its CPU and GPU tests share: test_kvcache_gpu.py, test_kvcache_forms_gpu.py, test_kvcache_ref_cpu.py.  Nothing here imports
the package; the entry under test is handed in as a callable.

Semantics restated here (flash-attn 2.7.4 docstring): new rows j of batch row b go to cache position cache_seqlens[b] + j; the
visible keys are positions [cache_leftpad[b], cache_seqlens[b] + s_new); causal masking is bottom-right aligned; new key j is
rotated at table row cache_seqlens[b] + j (with or without cache_leftpad -- the reading this library takes), query i at
cache_seqlens[b] + i when causal and at cache_seqlens[b] otherwise; table rows are clamped to [0, seqlen_ro) (csrc/kvcache.hip)."""
import copy
import os

import numpy as np
import torch

from oracle import attention as oattn
import parity

STRIDES = ("packed", "head_major", "padded")
PAD_VALUE = 777.0            # what the gaps of a "padded" allocation hold: a kernel that reads a wrong row or head meets it
# batch-stride padding (elements, multiples of 8: 16-byte rows) of q / k / v in the "padded" form: k and v differ
PADS = {"q": 16, "k": 8, "v": 24}


def _case():
    return os.environ.get("PYTEST_CURRENT_TEST", "?").split("::")[-1].split(" ")[0]


def rotate_np(x, cos, sin, pos, interleaved):
    """x float32 [..., d] at table row pos (clamped to the table's rows); fp32 arithmetic, one bf16 rounding (returns a bf16 torch
    tensor).  rotary_dim = 2 * cos.shape[1] may be any even value <= d: elements from rotary_dim on are copied."""
    x = np.asarray(x, np.float32).copy()
    half = cos.shape[1]
    rd = 2 * half
    pos = min(max(int(pos), 0), cos.shape[0] - 1)
    c, s = cos[pos].astype(np.float32), sin[pos].astype(np.float32)
    if interleaved:
        x1, x2 = x[..., 0:rd:2].copy(), x[..., 1:rd:2].copy()
        x[..., 0:rd:2], x[..., 1:rd:2] = x1 * c - x2 * s, x1 * s + x2 * c
    else:
        x1, x2 = x[..., :half].copy(), x[..., half:rd].copy()
        x[..., :half], x[..., half:rd] = x1 * c - x2 * s, x1 * s + x2 * c
    return torch.from_numpy(x).bfloat16()


def _tables(seqlen_ro, rotary_dim, dtype=np.float32):
    inv = 1.0 / (10000.0 ** (np.arange(0, rotary_dim, 2, dtype=np.float32) / rotary_dim))
    ang = np.arange(seqlen_ro, dtype=np.float32)[:, None] * inv[None, :]
    return np.cos(ang).astype(dtype), np.sin(ang).astype(dtype)


def _bf16_np(a):
    """fp32 numpy -> the nearest bf16 values, as fp32 numpy"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def layout_strides(strides, name, shape):
    """(batch, row, head) strides in elements that the form `strides` promises for tensor `name` ("q" / "k" / "v") of `shape`
    [B, s, H, d]"""
    b, s, h, d = shape
    if strides == "packed":
        return s * h * d, h * d, d
    if strides == "head_major":                               # storage [s, H, B, d]; generate.py: [1, H, T, d].permute(2, 0, 1, 3)
        return d, h * b * d, b * d
    if strides == "padded":
        return s * 2 * h * d + PADS[name], 2 * h * d, d + 8
    raise KeyError(strides)


def as_layout(t, strides, name, device="cpu"):
    """packed [B, s, H, d] bf16 -> a tensor of the same shape and values on `device`, laid out as `strides` names it"""
    if t is None:
        return None
    assert t.is_contiguous() and t.dim() == 4
    if strides == "packed":
        return t.to(device)
    if strides == "head_major":
        b, s, h, d = t.shape                                   # (a fresh allocation: canonical strides also for dimensions of size 1)
        return torch.empty((s, h, b, d), dtype=t.dtype).copy_(t.permute(1, 2, 0, 3)).to(device).permute(2, 0, 1, 3)
    b, s, h, d = t.shape
    st = layout_strides(strides, name, t.shape)
    n = (b - 1) * st[0] + (s - 1) * st[1] + (h - 1) * st[2] + d
    buf = torch.full((n,), PAD_VALUE, dtype=t.dtype)
    buf.as_strided(t.shape, st + (1,)).copy_(t)
    return buf.to(device).as_strided(t.shape, st + (1,))


class Case:
    """One batch against one cache layout; everything on the host until .dev() / .call().

    layout: contig, contig_bidx, contig_leftpad, contig_bidx_leftpad, paged<page size>.  d in {64, 80, 128}; s_q is independent of
    s_new.  rotary=(cos, sin, interleaved): numpy fp32 tables [seqlen_ro, rotary_dim / 2], any even rotary_dim <= d; seqlen_ro may be
    smaller than the largest position (rows are clamped); table_dtype="bf16" rounds the tables to bf16 first (the reference then
    computes in fp32 on the rounded values, as the kernel reads them) and uploads them as bf16.  The same seed and arguments give
    the same tensors as before the class moved here: every addition draws after, or instead of, nothing that existed."""

    def __init__(self, layout, s_new, s_q, hq, hkv, seed, d=128, batch=3, ends=None, rotary=None, table_dtype="f32", L=300):
        rng = np.random.default_rng(seed)
        self.layout, self.s_new, self.s_q, self.hq, self.hkv, self.d, self.b = layout, s_new, s_q, hq, hkv, d, batch
        f = lambda *sh: torch.from_numpy(rng.standard_normal(sh, dtype=np.float32)).bfloat16()  # noqa: E731
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
            rows = batch + (3 if "bidx" in layout else 0)
            self.kc, self.vc = f(rows, L, hkv, d), f(rows, L, hkv, d)
            if "bidx" in layout:
                self.batch_idx = torch.from_numpy(rng.permutation(rows)[:batch].astype(np.int32))
            if "leftpad" in layout:
                lp = [int(rng.integers(0, e + s_new + 1)) for e in ends]
                lp[1] = ends[1] + s_new                      # one row whose keys are all padding
                self.leftpad = torch.tensor(lp, dtype=torch.int32)
        self.q = f(batch, s_q, hq, d)
        self.k = f(batch, s_new, hkv, d) if s_new else None
        self.v = f(batch, s_new, hkv, d) if s_new else None
        self.table_dtype = table_dtype
        if rotary is not None and table_dtype == "bf16":
            rotary = (_bf16_np(rotary[0]), _bf16_np(rotary[1]), rotary[2])
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
        if self.rotary is None or self.s_new == 0:            # tables are applied with k / v only
            return self.q
        cos, sin, inter = self.rotary
        q = self.q.clone()
        for b in range(self.b):
            for i in range(self.s_q):
                q[b, i] = rotate_np(self.q[b, i].float().numpy(), cos, sin, self.ends[b] + (i if causal else 0), inter)
        return q

    def visible(self):
        """per batch row, the visible cache positions [cache_leftpad, cache_seqlens + s_new)"""
        lp = self.leftpad.tolist() if self.leftpad is not None else [0] * self.b
        return [list(range(lp[b], self.ends[b] + self.s_new)) for b in range(self.b)]

    def oracle(self, kc, vc, causal, scale=None):
        """-> (out fp64 [B * s_q, Hq, d], lse fp64 [B, Hq, s_q]) over the visible keys of the UPDATED caches kc / vc"""
        vis = self.visible()
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

    def views(self, strides, device="cpu"):
        """(q, k, v) on `device` in the form `strides`: the values of the packed tensors, whatever the form"""
        return as_layout(self.q, strides, "q", device), as_layout(self.k, strides, "k", device), as_layout(self.v, strides, "v", device)

    def tables(self, device="cpu"):
        """the rotary keyword arguments of the entry ({} without tables), tables in table_dtype"""
        if self.rotary is None:
            return {}
        cos, sin, inter = self.rotary
        up = (lambda a: torch.from_numpy(a).bfloat16().to(device)) if self.table_dtype == "bf16" else (lambda a: torch.from_numpy(a).to(device))
        return dict(rotary_cos=up(cos), rotary_sin=up(sin), rotary_interleaved=inter)

    def call(self, entry, causal, strides="packed", lse=True, kc=None, vc=None, tables=True, **kw):
        """entry = ops.kvcache_attn (or flash_attn_with_kvcache) on q / k / v in the form `strides`; q=None: append only.
        -> (out, lse or None, kc, vc) on the device; q is checked to be unmodified."""
        kc = self.kc.cuda() if kc is None else kc
        vc = self.vc.cuda() if vc is None else vc
        q, k, v = self.views(strides, "cuda")
        for name, t in (("q", q), ("k", k), ("v", v)):       # the kernel really gets the promised strides
            assert t is None or t.stride()[:3] == layout_strides(strides, name, t.shape), (name, t.stride())
        res = entry(q, kc, vc, k=k, v=v, cache_seqlens=torch.tensor(self.ends, dtype=torch.int32).cuda(),
                    cache_batch_idx=self.dev(self.batch_idx), cache_leftpad=self.dev(self.leftpad), block_table=self.dev(self.block_table),
                    causal=causal, return_softmax_lse=lse, **(self.tables("cuda") if tables else {}), **kw)
        if q is None:
            return res, None, kc, vc
        assert torch.equal(q.cpu(), self.q)                  # q is never modified
        out, got_lse = res if lse else (res, None)
        return out, got_lse, kc, vc


def token_rows(lengths, layout, hkv, seed, d=128):
    """The prefill form (generate.vsel_paged_attention_forward): the prompts of `lengths` tokens appended one token per batch row.
    -> a Case with q = None, T = sum(lengths) batch rows, s_new = 1, ends = tok_pos (the token's position in its prompt) and, for a
    paged layout, block_table = tok_table [T, max_pages] (each token's row is its prompt's block-table row); for "contig_bidx",
    batch_idx = each token's prompt's cache row.  .lengths / .tok_prompt / .prompt_table (or .prompt_rows) keep the lists."""
    rng = np.random.default_rng(seed)
    f = lambda *sh: torch.from_numpy(rng.standard_normal(sh, dtype=np.float32)).bfloat16()  # noqa: E731
    c = Case.__new__(Case)
    t = sum(lengths)
    c.layout, c.s_new, c.s_q, c.hq, c.hkv, c.d, c.b = layout, 1, 1, hkv, hkv, d, t
    c.lengths = list(lengths)
    c.tok_prompt = [p for p, n in enumerate(lengths) for _ in range(n)]
    c.ends = [j for n in lengths for j in range(n)]
    c.batch_idx = c.leftpad = c.block_table = None
    c.rotary, c.table_dtype, c.q = None, "f32", None
    if layout.startswith("paged"):
        c.page = int(layout[5:])
        need = [-(-n // c.page) for n in lengths]
        n_blocks = sum(need) + 5
        perm = rng.permutation(n_blocks)
        table = np.full((len(lengths), max(need) + 2), -1, np.int32)
        cur = 0
        for p, n in enumerate(need):
            table[p, :n] = perm[cur:cur + n]
            cur += n
        c.prompt_table = torch.from_numpy(table)
        c.block_table = c.prompt_table[c.tok_prompt].contiguous()
        c.kc, c.vc = f(n_blocks, c.page, hkv, d), f(n_blocks, c.page, hkv, d)
    else:
        assert layout == "contig_bidx"
        rows = len(lengths) + 3
        c.prompt_rows = torch.from_numpy(rng.permutation(rows)[:len(lengths)].astype(np.int32))
        c.batch_idx = c.prompt_rows[c.tok_prompt].contiguous()
        c.kc, c.vc = f(rows, max(lengths) + 5, hkv, d), f(rows, max(lengths) + 5, hkv, d)
    c.k, c.v = f(t, 1, hkv, d), f(t, 1, hkv, d)
    return c


def whole_prompt_caches(c):
    """The caches of token_rows() case `c` after appending each prompt WHOLE (one batch row, s_new = its length) through
    Case.expected_caches, one prompt after the other."""
    kc, vc = c.kc, c.vc
    t0 = 0
    for p, n in enumerate(c.lengths):
        one = copy.copy(c)
        one.b, one.s_new, one.ends, one.kc, one.vc = 1, n, [0], kc, vc
        one.k, one.v = c.k[t0:t0 + n, 0][None], c.v[t0:t0 + n, 0][None]          # [1, n, Hkv, d]
        if c.block_table is not None:
            one.block_table = c.prompt_table[p:p + 1]
        else:
            one.batch_idx = c.prompt_rows[p:p + 1]
        kc, vc = one.expected_caches()
        t0 += n
    return kc, vc


def check_all(case, got_out, got_lse, kc, vc, causal, tag, rotary=False, scale=None):
    """The gates of the entry: caches bit-exact (rotated rows within one bf16 ulp, everything else bit-identical), out within
    parity.check_fwd of the fp64 oracle on the updated caches, LSE (when given) within 2e-3 and -inf exactly where no key is
    visible; those rows output zeros."""
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
        rd = 2 * case.rotary[0].shape[1]                          # ... also the elements of the new rows past rotary_dim
        assert torch.equal(kc.view(-1, case.hkv, case.d)[..., rd:], ek.view(-1, case.hkv, case.d)[..., rd:]), tag
        ek = kc                                                   # the attention saw the kernel's rotated keys
    else:
        assert torch.equal(kc.view(torch.int16), ek.view(torch.int16)), tag
    assert torch.equal(vc.view(torch.int16), ev.view(torch.int16)), tag
    ref, ref_lse = case.oracle(ek, ev, causal, scale)
    parity.check_fwd(_case() + tag, got_out.float().cpu().numpy().reshape(ref.shape).astype(np.float64), ref)
    fin = np.isfinite(ref_lse)
    if got_lse is not None:
        got_lse = got_lse.cpu().double().numpy()
        assert got_lse.shape == ref_lse.shape
        assert np.array_equal(np.isfinite(got_lse), fin) and np.all(got_lse[~fin] == -np.inf), tag
        assert np.abs(got_lse[fin] - ref_lse[fin]).max(initial=0.0) <= 2e-3, tag
    # rows without a visible key output zeros
    zero_rows = torch.from_numpy(np.ascontiguousarray(~fin.transpose(0, 2, 1).reshape(-1, case.hq)))
    if bool(zero_rows.any()):
        assert float(got_out.reshape(-1, case.hq, case.d).cpu()[zero_rows].float().abs().max()) == 0.0, tag


def _without_row(case, drop):
    """a shallow copy of `case` whose row `drop` appends nothing (for the expected caches of the other rows)"""
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
