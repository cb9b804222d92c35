"""GPU value tests of vsel_kvcache_attn_fwd (csrc/kvcache.hip, ops.kvcache_attn) in the forms tests/test_kvcache_gpu.py does not reach:
the strided q / k / v views generation hands it (decode and append-only prefill), head dims 64 and 80, rotary edges (bf16 tables,
rotary_dim off the 16-byte vector, clamped table rows, s_q != s_new) and every attention form attn_launch (csrc/attn.hip) picks by
default under this entry.  Reference and gates are tests/kvcache_ref.py's (float64 oracle on the updated caches; check_all): caches
bit-exact without rotary, rotated rows within one bf16 ulp and everything else bit-identical, out within parity.check_fwd, LSE
within 2e-3 and -inf exactly on the rows that see no key, which output zeros.

The attention form of a case follows from (batch, s_q, heads, d, LSE wanted, cache kind); expected_form() restates attn_launch's
switches under default knobs, and every form case asserts the form it was built for from that restatement, next to the kernel name
the profiler saw.  Forms that the default dispatch reaches only from 2048 queries per row (8-wave, attn_fwd64_kernel over cu_k) are
forced by knob on small shapes, as said at those tests."""
import numpy as np
import pytest
import torch

from kvcache_ref import Case, _tables, check_all, token_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def entry():
    assert torch.cuda.is_available()
    from visionselector_amd import ops
    return ops.kvcache_attn


def _profiled(fn, knobs, want):
    """Run fn() under the knobs; the attention kernels the profiler saw must be exactly `want`, one launch each."""
    from visionselector_amd import _native as N
    with N.debug_knob(**knobs):
        N.profile_start()
        res = fn()
        prof = N.profile_stop()
    ran = {n: c for n, (_, c) in prof.items() if n.startswith("attn_") or n.startswith("varlen_attn")}
    assert ran == {n: 1 for n in want}, (knobs, prof)
    return res


def _same(a, b):
    """two (out, lse, kc, vc) results, bit for bit"""
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def _bits(t):
    return t.view(torch.int16)


# ---- a. the forms generation calls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [None, 0.2])
@pytest.mark.parametrize("hq,hkv", [(28, 4), (2, 1)])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("layout", ["paged16", "paged64"])
def test_decode_form_head_major_views(entry, layout, batch, hq, hkv, scale):
    """generate.vsel_paged_attention_forward's decode call: q / k / v are permute(2, 0, 1, 3) views of [1, H, B, d] tensors (batch
    stride d, head stride B d), one token per row.  B = 1 is read in place (the view is packed), B = 5 goes through the workspace
    copy of q.  With and without the LSE (without it, these grids take the two-KV-stream form): against the oracle, and bit for
    bit against the same call on contiguous copies."""
    case = Case(layout, 1, 1, hq, hkv, seed=700 + 10 * batch + hq, batch=batch)
    tag = f"[decode {layout} B={batch} {hq}/{hkv} scale={scale}]"
    kw = {} if scale is None else dict(softmax_scale=scale)
    for lse in (True, False):
        assert expected_form(batch, 1, hq, hkv, 128, lse, True) == ("direct" if lse else "split_q64")
        hm = case.call(entry, True, strides="head_major", lse=lse, **kw)
        assert hm[0].shape == (batch, 1, hq, 128) and hm[0].is_contiguous()
        check_all(case, *hm, True, tag + f"[lse={lse}]", scale=scale)
        assert _same(hm, case.call(entry, True, strides="packed", lse=lse, **kw)), tag


def test_decode_form_packed_wave_is_graph_capturable(entry):
    """The decode step of 19 prompts (19 x 28 > 512 (sequence, head) pairs: the packed GQA wave) on head-major views, captured on
    one stream and replayed after cache_seqlens and the static inputs were advanced ON THE DEVICE: it matches the eager call."""
    from kvcache_ref import as_layout
    case = Case("paged64", 1, 1, 28, 4, seed=23, batch=19, ends=[5 + 15 * i for i in range(19)])     # no end at 63 mod 64: two steps fit the pages
    assert expected_form(19, 1, 28, 4, 128, lse=False, paged=True) == "pack"
    kc, vc = case.kc.cuda(), case.vc.cuda()
    bt = case.dev(case.block_table)
    q_s, k_s, v_s = case.views("head_major", "cuda")
    seq_s = torch.tensor(case.ends, dtype=torch.int32).cuda()
    call = lambda q, k, v, sl, kc_, vc_: entry(q, kc_, vc_, k=k, v=v, cache_seqlens=sl, block_table=bt, causal=True)  # noqa: E731
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(q_s, k_s, v_s, seq_s, kc, vc)                # warm-up (also a real step: writes position ends[b])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out_g = call(q_s, k_s, v_s, seq_s, kc, vc)
    g = torch.Generator().manual_seed(3)
    new = [torch.randn(t.shape, generator=g).bfloat16() for t in (case.q, case.k, case.v)]
    q1, k1, v1 = (as_layout(t, "head_major", n, "cuda") for t, n in zip(new, "qkv"))
    assert q1.stride() == q_s.stride() and not q1.is_contiguous()
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
    # ... and the replayed step is the right one: the caches hold both appended tokens, the output is the oracle's
    step = Case("paged64", 1, 1, 28, 4, seed=23, batch=19, ends=[e + 1 for e in case.ends])
    step.block_table = case.block_table
    step.kc, step.vc = case.expected_caches()
    step.q, step.k, step.v = new
    check_all(step, out_g, None, kc, vc, True, "[replayed step]")


@pytest.mark.parametrize("lengths,layout", [([1, 17, 130], "paged16"), ([64, 65], "paged64"), ([5, 1, 33], "contig_bidx")])
def test_prefill_form_appends_one_token_per_row(entry, lengths, layout):
    """generate's prefill call: q=None, one batch row per prompt token, cache_seqlens = the token's position, block_table = its
    prompt's row repeated (or, on a contiguous cache, cache_batch_idx = its prompt's cache row); k / v head-major views.  Returns
    None; the caches equal the expectation bit for bit, so every element outside the written rows is untouched."""
    case = token_rows(lengths, layout, 4, seed=sum(lengths))
    res, _, kc, vc = case.call(entry, False, strides="head_major", lse=False)
    assert res is None
    ek, ev = case.expected_caches()
    assert torch.equal(_bits(kc.cpu()), _bits(ek)) and torch.equal(_bits(vc.cpu()), _bits(ev))
    assert not torch.equal(ek, case.kc)


def test_prefill_form_token_past_its_prompts_pages_writes_nothing(entry):
    """The caller error of the prefill form: a token whose position lies past its prompt's allocated pages (a -1 entry of its
    table row) or past the table's width.  Those tokens write nothing, every other token lands exactly, and the guard regions
    around the caches keep their sentinel."""
    case = token_rows([1, 17, 130], "paged16", 4, seed=9)
    bad = {17: 2 * 16 + 1,                                   # last token of the 17-token prompt: 2 pages allocated, entry 2 is -1
           18 + 100: case.block_table.shape[1] * 16 + 5}     # a token of the 130-token prompt: past the table's width
    assert int(case.block_table[17, 2]) == -1 and case.tok_prompt[17] == 1 and case.tok_prompt[118] == 2
    for t, pos in bad.items():
        case.ends[t] = pos
    guard = 4096
    sentinel = torch.tensor(-12345.0).bfloat16()
    caches = []
    for c in (case.kc, case.vc):
        buf = torch.full((c.numel() + 2 * guard,), float(sentinel), dtype=torch.bfloat16).cuda()
        view = buf[guard:guard + c.numel()].view(c.shape)
        view.copy_(c.cuda())
        caches.append((buf, view))
    (kbuf, kc), (vbuf, vc) = caches
    res, _, _, _ = case.call(entry, False, strides="head_major", lse=False, kc=kc, vc=vc)
    torch.cuda.synchronize()
    assert res is None
    for buf in (kbuf, vbuf):
        assert bool((buf[:guard] == sentinel).all()) and bool((buf[-guard:] == sentinel).all())
    ek, ev = case.kc.clone(), case.vc.clone()
    for t in range(case.b):
        if t not in bad:
            ek.view(-1, 4, 128)[case.row_of(t, case.ends[t])] = case.k[t, 0]
            ev.view(-1, 4, 128)[case.row_of(t, case.ends[t])] = case.v[t, 0]
    assert torch.equal(_bits(kc.cpu()), _bits(ek)) and torch.equal(_bits(vc.cpu()), _bits(ev))


@pytest.mark.parametrize("rot", [None, "interleaved", "neox"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("layout", ["paged64", "contig_leftpad"])
def test_padded_strides_equal_the_packed_call(entry, layout, causal, rot):
    """q / k / v sliced out of wider allocations (head stride d + 8, row stride twice the packed one, padded batch strides that
    differ between k and v; the gaps hold a value no tensor has): bit-identical to the packed call, without rotary and with it in
    both pairings -- the NeoX partner rotary_dim / 2 away is read from the strided source."""
    rotary = None if rot is None else (*_tables(400, 64), rot == "interleaved")
    case = Case(layout, 3, 3, 8, 2, seed=300 + 3 * causal + len(rot or ""), rotary=rotary)
    pad = case.call(entry, causal, strides="padded")
    check_all(case, *pad, causal, f"[padded {layout} causal={causal} rot={rot}]", rotary=rot is not None)
    assert _same(pad, case.call(entry, causal, strides="packed"))


# ---- b. head dims 64 and 80 -----------------------------------------------------------------------------------------------------------
LAYOUTS = ["contig", "contig_bidx", "contig_leftpad", "paged16", "paged64", "paged256"]
DIM_MATRIX = [(d, lay, s_new, causal, hq, hkv) for d in (64, 80) for lay in LAYOUTS for s_new in (0, 1, 7) for causal in (True, False)
              for hq, hkv in [(16, 16), (8, 2)]]


@pytest.mark.parametrize("d,layout,s_new,causal,hq,hkv", DIM_MATRIX)
def test_head_dims_64_and_80_match_oracle(entry, d, layout, s_new, causal, hq, hkv):
    """test_kvcache_matches_oracle's matrix at the other two head dims the entry dispatches: copy_row with 8 / 10 vectors per head,
    varlen_attn_fwd_kernel<4, 64 | 80> over a page table or a cu_k key offset."""
    s_q = s_new if s_new > 1 else (1 if s_new == 1 else 2)
    case = Case(layout, s_new, s_q, hq, hkv, seed=5000 + DIM_MATRIX.index((d, layout, s_new, causal, hq, hkv)), d=d)
    out, lse, kc, vc = case.call(entry, causal)
    assert out.shape == (case.b, s_q, hq, case.d) and lse.shape == (case.b, hq, s_q) and lse.dtype == torch.float32
    check_all(case, out, lse, kc, vc, causal, f"[d={d} {layout} s_new={s_new} causal={causal} {hq}/{hkv}]")


# rotary_dim equal to d, a multiple of 8 below it, off the 16-byte vector (20, 100: the copy branch fires inside a vector) and 2
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("d,rotary_dim", [(80, 80), (80, 20), (80, 2), (64, 64), (64, 32), (128, 100), (128, 20), (128, 2)])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("layout", ["paged16", "contig_leftpad"])
def test_rotary_dims_and_head_dims(entry, layout, causal, d, rotary_dim, interleaved):
    cos, sin = _tables(400, rotary_dim)
    case = Case(layout, 3, 3, 8, 2, seed=d + rotary_dim + 7 * interleaved + 3 * causal, d=d, rotary=(cos, sin, interleaved))
    out, lse, kc, vc = case.call(entry, causal)
    check_all(case, out, lse, kc, vc, causal, f"[rotary {layout} d={d} rd={rotary_dim} inter={interleaved} causal={causal}]", rotary=True)
    # the rotation did something: the new rows differ from the unrotated expectation inside rotary_dim
    plain = Case(layout, 3, 3, 8, 2, seed=d + rotary_dim + 7 * interleaved + 3 * causal, d=d).expected_caches()[0]
    assert not torch.equal(kc.cpu()[..., :rotary_dim], plain[..., :rotary_dim])


# ---- c. rotary edges at d = 128 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("layout", ["paged64", "contig_leftpad"])
def test_rotary_bf16_tables(entry, layout, interleaved):
    """bf16 tables (rot_f32 == 0): the reference rotates in fp32 with the bf16-rounded table values, as the kernel reads them."""
    cos, sin = _tables(400, 64)
    case = Case(layout, 3, 3, 8, 2, seed=61 + interleaved, rotary=(cos, sin, interleaved), table_dtype="bf16")
    assert case.tables()["rotary_cos"].dtype == torch.bfloat16 and not np.array_equal(case.rotary[0], cos)
    out, lse, kc, vc = case.call(entry, True)
    check_all(case, out, lse, kc, vc, True, f"[bf16 tables {layout} inter={interleaved}]", rotary=True)


@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("layout", ["paged64", "contig_leftpad"])
def test_rotary_table_rows_are_clamped_to_seqlen_ro(entry, layout, causal, interleaved):
    """seqlen_ro = 50 under positions up to 300: every row past the table rotates at its last row (kvcache.hip's header), keys and
    queries alike; the reference clamps the same way."""
    cos, sin = _tables(50, 64)
    case = Case(layout, 3, 3, 8, 2, seed=71 + interleaved + 2 * causal, ends=[10, 48, 297], rotary=(cos, sin, interleaved))   # 48, 49 | 50
    out, lse, kc, vc = case.call(entry, causal)
    check_all(case, out, lse, kc, vc, causal, f"[seqlen_ro=50 {layout} causal={causal} inter={interleaved}]", rotary=True)


@pytest.mark.parametrize("s_q,s_new", [(5, 2), (1, 4), (2, 0)])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("layout", ["paged64", "contig_leftpad"])
def test_rotary_query_positions_with_s_q_unequal_s_new(entry, layout, causal, s_q, s_new):
    """Query i rotates at cache_seqlens + i when causal and at cache_seqlens otherwise, whatever s_new is, and the causal mask is
    bottom-right aligned over cache_seqlens + s_new keys.  s_new = 0: the tables come without k / v and are dropped -- the result
    is the call without tables, bit for bit."""
    cos, sin = _tables(400, 64)
    case = Case(layout, s_new, s_q, 8, 2, seed=81 + s_q + 2 * causal, rotary=(cos, sin, False))
    res = case.call(entry, causal)
    check_all(case, *res, causal, f"[{layout} s_q={s_q} s_new={s_new} causal={causal}]", rotary=True)
    if s_new == 0:
        assert _same(res, case.call(entry, causal, tables=False))
    else:                                                     # the rule matters: the two settings rotate q differently
        assert not torch.equal(case.rotated_q(True), case.rotated_q(False)) or s_q == 1


# ---- d. every attention form the default dispatch reaches under this entry ------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def expected_form(batch, s_q, hq, hkv, d, lse, paged, causal=False):
    """attn_launch (csrc/attn.hip) under default knobs, for the calls of vsel_kvcache_attn_fwd (seqlens_k always given; a page table or
    cu_k): the form it picks, by the conditions documented there."""
    rep = hq // hkv
    items8 = _cdiv(s_q, 256) * hq * batch
    big = (s_q >= 2048 and items8 >= 1024) or (s_q >= 4096 and items8 >= 400)            # 8-wave workgroups, 256 queries each
    pack = d == 128 and s_q * rep <= 32 and batch * hq > 512                              # one wave serves a kv head's whole q-head group
    items4 = _cdiv(s_q, 128) * hq * batch
    split2 = d == 128 and not pack and not big and items4 <= 256 and not lse            # two KV streams per workgroup
    if d == 128 and not pack and not paged and s_q >= 2048 and not split2:
        return "rows64"                                                                   # attn_fwd64_kernel, contiguous keys at cu_k
    if pack:
        return "pack"
    if split2:
        return "split_q64" if _cdiv(s_q, 64) * hq * batch <= 256 else "split_q128"
    if big:
        return "waves8"
    slots = 512                                                                           # resident 4-wave workgroups
    if items4 <= slots:
        return "direct"                                                                   # one item per workgroup
    if d == 128 and 20 * items4 <= 47 * slots:
        return "static"                                                                   # few rounds: the item list dealt out
    return "queue_tail_first" if causal and d == 128 and items4 > 2 * slots else "queue"


# heads (28, 4) (rep 7), d = 128, s_q = s_new; the derivation of each case from attn_launch's switches:
FORMS = {
    # A  pack: s_q * rep = 7 <= 32 and B * hq = 19 * 28 = 532 > 512 (B = 18: 504, the per-head grid still fits one round)
    "A": dict(batch=19, s=1, heads=(28, 4), form="pack"),
    # A  at rep 1: 65 * 8 = 520 > 512; a 96-position cache keeps the 65 + 3 cache rows small
    "A_rep1": dict(batch=65, s=1, heads=(8, 8), form="pack", L=96),
    # B  two streams, 128-query workgroups: 4-wave items ceil(70 / 128) * 28 * 5 = 140 <= 256 (no LSE wanted), 64-query items
    #    ceil(70 / 64) * 28 * 5 = 280 > 256; 70 * 7 > 32 is not packable
    "B": dict(batch=5, s=70, heads=(28, 4), form="split_q128"),
    # C  4-wave, one item per workgroup: 256 < 28 * 12 = 336 <= 512; 7 * 7 = 49 > 32 is not packable
    "C": dict(batch=12, s=7, heads=(28, 4), form="direct"),
    # D  4-wave, static deal: 512 < 28 * 20 = 560, 20 * 560 = 11200 <= 47 * 512 = 24064
    "D": dict(batch=20, s=7, heads=(28, 4), form="static"),
    # E  4-wave behind the work queue: 28 * 44 = 1232, 20 * 1232 = 24640 > 24064 (B = 42: 23520, still dealt); 1232 > 2 * 512:
    #    tail-first tiling when causal
    "E": dict(batch=44, s=7, heads=(28, 4), form="queue"),
}
FORM_LAYOUTS = ["paged64", "contig_leftpad"]


def _form_case(name, layout, causal, d=128):
    f = FORMS[name]
    if name.startswith("A") and layout == "contig_leftpad":
        layout = "contig_bidx_leftpad"           # the entry allows cache_batch_idx and cache_leftpad together on a contiguous cache
    hq, hkv = f["heads"]
    seed = 9000 + 16 * sorted(FORMS).index(name) + 4 * FORM_LAYOUTS.index(layout.replace("_bidx", "")) + 2 * causal
    return Case(layout, f["s"], f["s"], hq, hkv, seed=seed, d=d, batch=f["batch"], L=f.get("L", 300))


def test_form_table_reaches_every_default_form():
    """The switch restated: each case sits in the regime it was built for, its neighbour on the other side of the threshold does
    not, and the forms that need 2048 queries per row (forced by knob below) are reached by default from there."""
    for name, f in FORMS.items():
        hq, hkv = f["heads"]
        for paged in (True, False):
            for causal in (True, False):
                lse = name != "B"
                want = "queue_tail_first" if f["form"] == "queue" and causal else f["form"]
                assert expected_form(f["batch"], f["s"], hq, hkv, 128, lse, paged, causal) == want, (name, paged, causal)
    ef = lambda b, s, **kw: expected_form(b, s, 28, 4, 128, kw.pop("lse", True), True, **kw)  # noqa: E731
    assert ef(18, 1) == "direct" and ef(19, 1) == "pack" and ef(19, 5) == "static"           # 5 * 7 > 32: not packable
    assert expected_form(64, 1, 8, 8, 128, True, True) == "direct"
    assert ef(5, 70, lse=False) == "split_q128" and ef(5, 70) == "direct" and ef(5, 64, lse=False) == "split_q64"
    assert ef(9, 7, lse=False) == "split_q64" and ef(10, 7, lse=False) == "direct"          # 252 <= 256 < 280
    assert ef(18, 7) == "direct" and ef(19, 7) == "static" and ef(42, 7) == "static" and ef(43, 7) == "queue"
    assert ef(43, 7, causal=True) == "queue_tail_first" and ef(36, 7, causal=True) == "static"
    assert expected_form(12, 7, 28, 4, 80, True, True) == "direct" and expected_form(44, 7, 28, 4, 80, True, True, True) == "queue"
    assert expected_form(1, 2048, 28, 4, 128, True, False) == "rows64" and expected_form(40, 2048, 28, 4, 128, True, True) == "waves8"


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("layout", FORM_LAYOUTS)
@pytest.mark.parametrize("name", sorted(FORMS))
def test_default_forms_match_oracle(entry, name, layout, causal):
    """A to E under default knobs (form B without the LSE: the two-stream form is not taken when it is wanted).  Against the oracle;
    the profiler saw one varlen_attn_fwd_kernel launch and no attn_fwd64_kernel; and against the neighbouring form where the
    attention tests establish the relation for the pair: packed == per-head and tail-first == start-aligned tiling bit for bit,
    two streams within 2^-6 of one stream."""
    case = _form_case(name, layout, causal)
    f = FORMS[name]
    lse = name != "B"
    want = "queue_tail_first" if f["form"] == "queue" and causal else f["form"]
    assert expected_form(case.b, case.s_q, case.hq, case.hkv, case.d, lse, case.block_table is not None, causal) == want
    res = _profiled(lambda: case.call(entry, causal, lse=lse), {}, ["varlen_attn_fwd_kernel"])
    check_all(case, *res, causal, f"[form {name} {layout} causal={causal}]")
    if f["form"] == "pack":
        other = _profiled(lambda: case.call(entry, causal), dict(attn_pack=0, attn_split=0), ["varlen_attn_fwd_kernel"])
        assert _same(res, other)
    elif f["form"] == "split_q128":
        one = _profiled(lambda: case.call(entry, causal, lse=False), dict(attn_split=0), ["varlen_attn_fwd_kernel"])
        assert torch.equal(res[2], one[2]) and torch.equal(res[3], one[3])
        assert float((res[0].float() - one[0].float()).abs().max()) <= 2 ** -6 * float(one[0].float().abs().max())
        with_lse = _profiled(lambda: case.call(entry, causal), {}, ["varlen_attn_fwd_kernel"])     # LSE wanted: the 4-wave form
        assert torch.equal(with_lse[0], one[0])
        check_all(case, *with_lse, causal, f"[form {name} with lse]")
    elif want == "queue_tail_first":
        assert _same(res, _profiled(lambda: case.call(entry, causal), dict(attn_tail_first=0), ["varlen_attn_fwd_kernel"]))


@pytest.mark.parametrize("name", ["A", "C", "E"])
def test_default_forms_at_another_scale_with_lse(entry, name):
    case = _form_case(name, "contig_leftpad", True)
    res = _profiled(lambda: case.call(entry, True, softmax_scale=0.2), {}, ["varlen_attn_fwd_kernel"])
    assert res[1] is not None
    check_all(case, *res, True, f"[form {name} scale=0.2]", scale=0.2)
    assert not torch.equal(res[0], case.call(entry, True)[0])


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("d,layout", [(128, "paged64"), (128, "contig_leftpad"), (80, "paged64"), (80, "contig_leftpad")])
def test_forced_eight_wave_form(entry, d, layout, causal):
    """Form F.  By default the 8-wave form needs s_q >= 2048 and at least 400 items, and the float64 oracle of such a call takes
    tens of seconds on the host; so it is forced (attn_waves=8) on case C's shape, where it runs 256-query items behind the work
    queue.  Same arithmetic per query as the 4-wave form: bit-identical to the default call."""
    case = _form_case("C", layout, causal, d=d)
    res = _profiled(lambda: case.call(entry, causal), dict(attn_waves=8), ["varlen_attn_fwd_kernel"])
    check_all(case, *res, causal, f"[8 waves d={d} {layout} causal={causal}]")
    assert _same(res, _profiled(lambda: case.call(entry, causal), {}, ["varlen_attn_fwd_kernel"]))


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("layout", ["contig_leftpad", "contig_bidx_leftpad", "contig"])
def test_forced_rows64_form_over_cu_k(entry, layout, causal):
    """Form G.  attn_fwd64_kernel is what a CONTIGUOUS cache gets from s_q >= 2048 (a page table never does); the float64 oracle
    of that shape takes tens of seconds on the host, so the form is forced (attn_rows64=1) on case B's shape.  It reads the keys
    at cu_k[b] = cache_batch_idx[b] * L_cache + cache_leftpad[b] with seqlens_k[b] of them.  Bit-identical to the 4-wave form."""
    f = FORMS["B"]
    case = Case(layout, f["s"], f["s"], *f["heads"], seed=9500 + len(layout) + causal, batch=f["batch"])
    res = _profiled(lambda: case.call(entry, causal), dict(attn_rows64=1), ["attn_fwd64_kernel"])
    check_all(case, *res, causal, f"[rows64 {layout} causal={causal}]")
    assert _same(res, _profiled(lambda: case.call(entry, causal), dict(attn_rows64=0, attn_split=0), ["varlen_attn_fwd_kernel"]))
