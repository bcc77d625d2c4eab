"""GPU tests of the append for a latent (MLA) KV cache: kvcache_append_mla, kvcache_append_mla_varlen and the fused form of flash_attention_decode_mla.

Correctness needs no tolerance: every stored element is a source element bit for bit or the one rounding of kvappend_refs.rotary_f32
(tests/mla_append_refs.py builds the images; tests/test_kvappend_mla.py holds the builder to fa2_rotary_eval).  In every case the cache and q_out start
from a poison pattern and the WHOLE cache image and the WHOLE q_out are compared as int16, so a stray write anywhere fails.  The fused decode call is
held bit for bit to append-then-decode, and to mla_refs' float64 bars against a cache built by the float64 rotation."""
import pytest
import torch

import decode_calls as dc
import decode_refs as dr
import far_layouts as fl
import kvappend_refs as kr
import mla_append_refs as ar
import mla_refs as mr
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention_decode_mla, kvcache_append_mla, kvcache_append_mla_varlen
from test_kvappend_varlen import HOSTILE

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
LN2 = 0.6931471805599453
D, DV = ar.D, ar.DV
SEQLEN_RO = 180                     # shorter than the caches: positions at or beyond it are rotated by the last table row


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(ar.bits(a.cpu()), ar.bits(b.cpu()))


def layout(kind, B, dtype, g):
    """-> (poisoned cache image (CPU), block table or None, capacity in keys).  contig: [B, 200, 576]; page64 / page128: a pool of 256 keys per
    sequence in shuffled pages, two spare pages nobody names"""
    if kind == "contig":
        return ar.poisoned((B, 200, D), dtype), None, 200
    page = 64 if kind == "page64" else 128
    per = 256 // page
    order = torch.randperm(B * per + 2, generator=g)
    bt = order[:B * per].view(B, per).to(torch.int32)
    return ar.poisoned((B * per + 2, page, D), dtype), bt, 256


def lengths(B, nnew, cap, variant):
    """Lengths AFTER the append that, over the variants, are 0, below Nnew, equal to the capacity, above it (the tail of the chunk lies outside) and
    in the middle (Nnew = 130 from position 10 on crosses two boundaries of 64-key pages)."""
    pool = [[nnew - 1, cap + 1, 10 + nnew], [0, cap, cap + nnew // 2 + 3], [10 + nnew, nnew - 1 if nnew > 1 else 0, cap]][variant % 3]
    return pool[:B] if B == 3 else [pool[(variant // 3 + variant) % 3]]


def run_uniform(dev, dtype, B, nnew, H, kind, tab, inter, variant, seed):
    g = torch.Generator().manual_seed(seed)
    cache, bt, cap = layout(kind, B, dtype, g)
    lens = lengths(B, nnew, cap, variant)
    kv_c, k_pe, q = ar.inputs(B * nnew, H, dtype, seed)
    cos, sin = (None, None) if tab == "none" else ar.tables(SEQLEN_RO, torch.float32 if tab == "f32" else dtype)
    if cos is None:
        q = None                                                 # q needs tables
    want_img, want_q = ar.expect(cache, kv_c, k_pe, ar.uniform_owners(B, nnew), lens, bt, q, cos, sin, inter)
    cache_d = cache.to(dev)
    up = lambda t: None if t is None else t.to(dev)              # noqa: E731
    got_q = kvcache_append_mla(cache_d, kv_c.view(B, nnew, DV).to(dev), k_pe.view(B, nnew, D - DV).to(dev), torch.tensor(lens, dtype=torch.int32, device=dev),
                               block_table=up(bt), rotary_cos=up(cos), rotary_sin=up(sin), rotary_interleaved=inter,
                               q=None if q is None else q.view(B, nnew, H, D).to(dev))
    torch.cuda.synchronize()
    tag = (dtype, B, nnew, H, kind, tab, inter, lens)
    assert same_bits(cache_d, want_img), ("cache image", tag)
    if q is None:
        assert got_q is None
    else:
        assert same_bits(got_q.view(B * nnew, H, D), want_q), ("q_out", tag)


KINDS, TABS = ("contig", "page64", "page128"), ("f32", "16bit", "none")
UNIFORM = []
for n, (H, nnew, B) in enumerate((H, nnew, B) for H in (0, 1, 5, 16, 128) for nnew in (1, 3, 130) for B in (1, 3)):
    # 30 (H, Nnew, B): the layouts, table kinds, pairings, dtypes and length variants cycle at different periods, so that every value of each meets
    # every H and every Nnew at least once over the list
    UNIFORM.append((H, nnew, B, KINDS[(n + n // 6) % 3], TABS[(n // 2 + n // 6) % 3] if H == 0 else TABS[(n // 2) % 2], bool((n // 3 + n) % 2), (F16, BF16)[(n + n // 2) % 2], n))


def test_the_uniform_cases_cover_every_axis():
    for i, vals in enumerate((KINDS, None, (True, False), (F16, BF16))):
        for H in (0, 1, 5, 16, 128):
            if vals is not None:
                assert {c[3 + i] for c in UNIFORM if c[0] == H} == set(vals), (i, H)
    assert {c[4] for c in UNIFORM} == set(TABS) and {c[4] for c in UNIFORM if c[0]} == {"f32", "16bit"}
    assert any(c[1] == 130 and c[3] == "page64" for c in UNIFORM) and any(c[1] == 130 and c[0] == 128 for c in UNIFORM)
    seen = set()
    for (H, nnew, B, kind, tab, inter, dtype, n) in UNIFORM:
        cap = 200 if kind == "contig" else 256
        for ln in lengths(B, nnew, cap, n):
            seen |= {"zero"} if ln == 0 else set()
            seen |= {"short"} if 0 < ln < nnew else set()
            seen |= {"full"} if ln == cap else set()
            seen |= {"over"} if ln > cap else set()
    assert seen == {"zero", "short", "full", "over"}


@pytest.mark.parametrize("case", UNIFORM, ids=lambda c: "H%d-N%d-B%d-%s-%s-%s-%s" % (c[0], c[1], c[2], c[3], c[4], "gptj" if c[5] else "neox", "f16" if c[6] == F16 else "bf16"))
def test_uniform(case):
    H, nnew, B, kind, tab, inter, dtype, n = case
    run_uniform(dc.dev(), dtype, B, nnew, H, kind, tab, inter, n, 1000 + n)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("inter", [True, False], ids=["gptj", "neox"])
def test_shared_pages_and_page_ids_outside_the_pool(dtype, inter):
    """Pages of 64, five sequences of 3 new tokens.  Sequences 0 and 1 name ONE page in slot 3 of their tables, which neither writes; sequence 3's first
    token (position 63) meets page id -1 and sequence 4's first (position 127) page id num_pages: both are skipped — nothing is clamped onto a live
    page — while the tokens behind them, in the next slot, are written."""
    dev = dc.dev()
    B, nnew, H, page, per = 5, 3, 5, 64, 4
    g = torch.Generator().manual_seed(77)
    pages = B * per + 1
    bt = torch.randperm(pages, generator=g)[:B * per].view(B, per).to(torch.int32)
    lens = [70, 130, 200, 66, 130]
    bt[1, 3] = bt[0, 3]
    bt[3, 0], bt[4, 1] = -1, pages
    cache = ar.poisoned((pages, page, D), dtype)
    kv_c, k_pe, q = ar.inputs(B * nnew, H, dtype, 78)
    cos, sin = ar.tables(SEQLEN_RO)
    want_img, want_q = ar.expect(cache, kv_c, k_pe, ar.uniform_owners(B, nnew), lens, bt, q, cos, sin, inter)
    written = int((ar.bits(want_img) != ar.POISON).any(-1).sum())
    assert written == B * nnew - 2, "two tokens are skipped"
    cache_d = cache.to(dev)
    got_q = kvcache_append_mla(cache_d, kv_c.view(B, nnew, DV).to(dev), k_pe.view(B, nnew, 64).to(dev), torch.tensor(lens, dtype=torch.int32, device=dev),
                               block_table=bt.to(dev), rotary_cos=cos.to(dev), rotary_sin=sin.to(dev), rotary_interleaved=inter, q=q.view(B, nnew, H, D).to(dev))
    assert same_bits(cache_d, want_img) and same_bits(got_q.view(B * nnew, H, D), want_q)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_strided_sources_cache_and_q(dtype):
    """kv_c and k_pe as the two slices of one [B, Nnew, 584] buffer, the cache as a view with a row stride of 584 inside a poisoned buffer, q a view of
    [B, Nnew, H, 584]: nothing is copied, and the buffer's pad columns stay poison."""
    dev = dc.dev()
    B, nnew, H, cap = 3, 3, 5, 200
    lens = [2, 200, 77]
    kv_c, k_pe, q = ar.inputs(B * nnew, H, dtype, 31)
    cos, sin = ar.tables(SEQLEN_RO, dtype)
    under = ar.poisoned((B, cap, 584), dtype)
    img, want_q = ar.expect(under[..., :D], kv_c, k_pe, ar.uniform_owners(B, nnew), lens, None, q, cos, sin, False)
    want_under = under.clone()
    want_under[..., :D] = img
    proj = ar.poisoned((B, nnew, 584), dtype)
    proj[..., :DV], proj[..., DV:D] = kv_c.view(B, nnew, DV), k_pe.view(B, nnew, 64)
    qw = ar.poisoned((B, nnew, H, 584), dtype)
    qw[..., :D] = q.view(B, nnew, H, D)
    under_d, proj_d, qw_d = under.to(dev), proj.to(dev), qw.to(dev)
    got_q = kvcache_append_mla(under_d[..., :D], proj_d[..., :DV], proj_d[..., DV:D], torch.tensor(lens, dtype=torch.int32, device=dev), rotary_cos=cos.to(dev),
                               rotary_sin=sin.to(dev), rotary_interleaved=False, q=qw_d[..., :D])
    assert same_bits(under_d, want_under) and same_bits(got_q.view(B * nnew, H, D), want_q)
    assert same_bits(proj_d, proj) and same_bits(qw_d, qw), "the sources are not touched"


# ---------------------------------------------------------------------------------------------------------------- packed
COUNTS = (0, 1, 130, 3, 0, 64)


def packed_owners(counts, total):
    owners = [(s, i, c) for s, c in enumerate(counts) for i in range(c)]
    return owners + [None] * (total - len(owners))


def run_packed(dev, dtype, cu, owners, total, lens, kind, H, tab, inter, seed):
    B = len(cu) - 1
    g = torch.Generator().manual_seed(seed)
    cache, bt, cap = layout(kind, B, dtype, g)
    kv_c, k_pe, q = ar.inputs(total, H, dtype, seed)
    cos, sin = (None, None) if tab == "none" else ar.tables(SEQLEN_RO, torch.float32 if tab == "f32" else dtype)
    want_img, want_q = ar.expect(cache, kv_c, k_pe, owners, lens, bt, q, cos, sin, inter)
    up = lambda t: None if t is None else t.to(dev)              # noqa: E731
    cache_d = cache.to(dev)
    got_q = kvcache_append_mla_varlen(cache_d, kv_c.to(dev), k_pe.to(dev), torch.tensor(cu, dtype=torch.int32, device=dev),
                                      torch.tensor(lens, dtype=torch.int32, device=dev), block_table=up(bt), rotary_cos=up(cos), rotary_sin=up(sin),
                                      rotary_interleaved=inter, q=up(q))
    torch.cuda.synchronize()
    assert same_bits(cache_d, want_img), ("cache image", dtype, cu, lens, kind, H)
    assert (got_q is None) if q is None else same_bits(got_q, want_q), ("q_out", dtype, cu, lens, kind, H)
    return cache_d, got_q


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind,H,tab,inter", [("contig", 5, "f32", True), ("page64", 16, "16bit", False), ("page128", 0, "none", True), ("page64", 128, "f32", False)])
def test_packed_counts(kind, H, tab, inter, dtype):
    """Counts (0, 1, 130, 3, 0, 64): leading, trailing-inside and consecutive empty sequences, a decode row, a chunk that crosses two page boundaries.
    Lengths: a sequence without new tokens, one at the capacity, the chunk from position 10 on, one shorter than its count, an empty one, one in the middle."""
    cap = 200 if kind == "contig" else 256
    cu = [0]
    for c in COUNTS:
        cu.append(cu[-1] + c)
    lens = [50, cap, 140, 2, 0, 150]
    run_packed(dc.dev(), dtype, cu, packed_owners(COUNTS, cu[-1]), cu[-1], lens, kind, H if tab != "none" else 0, tab, inter, 500 + H)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", ["contig", "page64"])
def test_packed_equals_uniform_on_equal_counts(kind, dtype):
    dev = dc.dev()
    B, nnew, H = 3, 3, 5
    g = torch.Generator().manual_seed(5)
    cache, bt, cap = layout(kind, B, dtype, g)
    lens = [2, cap, 77]
    kv_c, k_pe, q = ar.inputs(B * nnew, H, dtype, 6)
    cos, sin = ar.tables(SEQLEN_RO)
    up = lambda t: None if t is None else t.to(dev)              # noqa: E731
    lens_d, c1, c2 = torch.tensor(lens, dtype=torch.int32, device=dev), cache.to(dev), cache.to(dev)
    q1 = kvcache_append_mla(c1, kv_c.view(B, nnew, DV).to(dev), k_pe.view(B, nnew, 64).to(dev), lens_d, up(bt), cos.to(dev), sin.to(dev), False, q.view(B, nnew, H, D).to(dev))
    q2 = kvcache_append_mla_varlen(c2, kv_c.to(dev), k_pe.to(dev), torch.arange(0, (B + 1) * nnew, nnew, dtype=torch.int32, device=dev), lens_d, up(bt), cos.to(dev),
                                   sin.to(dev), False, q.to(dev))
    assert same_bits(c1, c2) and same_bits(q1.view(B * nnew, H, D), q2)
    assert not same_bits(c1, cache), "something was written"


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_a_partly_filled_token_buffer(dtype):
    """cu[B] < total: the rows behind cu[B] (and in front of cu[0]) belong to no sequence — no latent row is written for them and their q rows come back
    bit for bit."""
    cu, total = [2, 5, 5, 9], 16
    owners = [None] * 2 + [(0, i, 3) for i in range(3)] + [(2, i, 4) for i in range(4)] + [None] * 7
    _, got_q = run_packed(dc.dev(), dtype, cu, owners, total, [40, 9, 100], "page64", 5, "f32", True, 41)
    _, _, q = ar.inputs(total, 5, dtype, 41)
    for t in (0, 1, 9, 15):
        assert torch.equal(ar.bits(got_q[t].cpu()), ar.bits(q[t]))


@pytest.mark.parametrize("which", range(len(HOSTILE)))
def test_hostile_cu_seqlens_stay_inside_the_predicted_rows(which):
    """The arrays of tests/test_kvappend_varlen.py: only the rows the host side of the search (fa2_kvappend_varlen_token) gives to a sequence may change;
    every other q row comes back bit for bit, and the whole cache image is the predicted one."""
    cu = HOSTILE[which]
    B, total = len(cu) - 1, 24
    owners = [_fa2_lib.kvappend_varlen_token(cu, t) for t in range(total)]
    lens = [30, 12, 64, 5]
    run_packed(dc.dev(), BF16 if which % 2 else F16, cu, owners, total, lens, "contig" if which % 2 else "page64", 4, "f32", bool(which % 3), 900 + which)


# ---------------------------------------------------------------------------------------------------------------- fused
def fused_case(dtype, Nq, kind, inter, seed):
    """-> CPU pieces of a step: q, kv_c, k_pe, the lengths after the append, the cache before (the new rows and everything at or beyond a length hold
    NaN), the block table, the tables, and the float64-rotated reference (q_ref, kv_ref [B, nmax, 576])"""
    B, H, nmax = 3, 16, 256
    lens = [130, 65, 200]
    q, kv = mr.inputs(B, H, Nq, nmax, lens, dtype, seed)
    g = torch.Generator().manual_seed(seed + 1)
    k_pe = (torch.randn(B, Nq, 64, generator=g) * 2.0).to(dtype)
    kv_c = torch.stack([kv[b, n - Nq:n, :DV] for b, n in enumerate(lens)])
    cos, sin = ar.tables(nmax)
    pos = torch.tensor([[n - Nq + i for i in range(Nq)] for n in lens])
    c64, s64 = cos[pos].double(), sin[pos].double()
    kv_ref, q_ref, before = kv.clone(), q.clone(), kv.clone()
    for b, n in enumerate(lens):
        kv_ref[b, n - Nq:n, DV:] = kr.rotary_ref64(k_pe[b].double(), c64[b], s64[b], 64, inter)[0].to(dtype)
        before[b, n - Nq:n] = float("nan")
    q_ref[..., DV:] = kr.rotary_ref64(q[..., DV:].double(), c64[:, :, None], s64[:, :, None], 64, inter)[0].to(dtype)
    bt = None
    if kind == "page64":
        before, bt = mr.paged(before, [nmax] * B, 64, g, spare=2)
    return q, kv_c, k_pe, lens, before, bt, cos, sin, q_ref, kv_ref


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("kind", ["contig", "page64"])
@pytest.mark.parametrize("Nq", [1, 2])
def test_fused_is_append_then_decode_and_meets_the_float64_bars(Nq, kind, split, dtype):
    dev = dc.dev()
    inter = Nq == 1
    q, kv_c, k_pe, lens, before, bt, cos, sin, q_ref, kv_ref = fused_case(dtype, Nq, kind, inter, 300 + Nq)
    up = lambda t: None if t is None else t.to(dev)              # noqa: E731
    lens_d, c1, c2 = torch.tensor(lens, dtype=torch.int32, device=dev), before.to(dev), before.to(dev)
    kw = dict(block_table=up(bt), rotary_cos=cos.to(dev), rotary_sin=sin.to(dev), rotary_interleaved=inter)
    o1, l1 = flash_attention_decode_mla(q.to(dev), c1, lens_d, return_lse=True, num_splits=split, scale=mr.SCALE, kv_c=kv_c.to(dev), k_pe=k_pe.to(dev), **kw)
    q_out = kvcache_append_mla(c2, kv_c.to(dev), k_pe.to(dev), lens_d, q=q.to(dev), **kw)
    o2, l2 = flash_attention_decode_mla(q_out, c2, lens_d, block_table=up(bt), return_lse=True, num_splits=split, scale=mr.SCALE)
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)) and torch.equal(l1, l2), "fused == append, then decode on q_out"
    want_img, want_q = ar.expect(before, kv_c.reshape(-1, DV), k_pe.reshape(-1, 64), ar.uniform_owners(3, Nq), lens, bt, q.reshape(3 * Nq, 16, D), cos, sin, inter)
    assert same_bits(c1, want_img) and same_bits(c2, want_img) and same_bits(q_out.view(3 * Nq, 16, D), want_q)
    code = dc.code(dtype)
    dr.check(o1, l1 / LN2, mr.refs(q_ref, kv_ref, lens, code), lens, code, ("fused", Nq, kind, split))


@pytest.mark.parametrize("kind", ["contig", "page64"])
def test_a_refused_fused_call_leaves_the_cache_untouched_and_the_plain_call_is_todays(kind):
    dev = dc.dev()
    dtype, Nq = BF16, 2
    q, kv_c, k_pe, lens, before, bt, cos, sin, _, _ = fused_case(dtype, Nq, kind, True, 350)
    up = lambda t: None if t is None else t.to(dev)              # noqa: E731
    lens_d, cache = torch.tensor(lens, dtype=torch.int32, device=dev), before.to(dev)
    for bad in (129, -1):
        with pytest.raises(ValueError, match="num_splits"):
            flash_attention_decode_mla(q.to(dev), cache, lens_d, block_table=up(bt), num_splits=bad, kv_c=kv_c.to(dev), k_pe=k_pe.to(dev), rotary_cos=cos.to(dev),
                                       rotary_sin=sin.to(dev))
    with pytest.raises(ValueError):
        flash_attention_decode_mla(q.to(dev), cache, lens_d, block_table=up(bt), kv_c=kv_c.to(dev), k_pe=k_pe.to(dev), rotary_cos=cos[:, :16].to(dev),
                                   rotary_sin=sin[:, :16].to(dev))
    torch.cuda.synchronize()
    assert same_bits(cache, before), "a refused call writes nothing"
    # without the five keywords: the entry's own result, bit for bit, and the cache as it was (a cache whose new rows are in place: no NaN among the keys)
    full, _ = ar.expect(before, kv_c.reshape(-1, DV), k_pe.reshape(-1, 64), ar.uniform_owners(3, Nq), lens, bt)
    full_d, qd = full.to(dev), q.to(dev)
    o, lse = flash_attention_decode_mla(qd, full_d, lens_d, block_table=up(bt), return_lse=True, num_splits=3, scale=mr.SCALE)
    o_c, lse_c = mr.mla_c(qd, full_d, lens_d, 3, block_table=up(bt))
    assert torch.equal(o.view(torch.int16), o_c.view(torch.int16)) and torch.equal(lse, lse_c * LN2) and same_bits(full_d, full)


def test_graph_replay_of_a_whole_step():
    """Captured once: the lengths incremented in place, then the fused call.  Replayed for three steps while the new tokens, the lengths and — before the
    last step — the block table change in place: the cache image, o and lse equal an eager trace of the same steps on a cache of its own."""
    dev = dc.dev()
    dtype, B, H, Nq, page = BF16, 3, 16, 1, 64
    g = torch.Generator().manual_seed(17)
    start = [62, 127, 5]                                          # the steps cross a page boundary in two of the sequences
    pages = B * 4 + 1
    bt = torch.randperm(pages, generator=g)[:B * 4].view(B, 4).to(torch.int32)
    pool = (torch.randn(pages, page, D, generator=g)).to(dtype)
    cos, sin = (t.to(dev) for t in ar.tables(256))
    steps = [tuple(t.to(dev) for t in ((torch.randn(B, Nq, H, D, generator=g)).to(dtype), torch.randn(B, Nq, DV, generator=g).to(dtype),
                                       torch.randn(B, Nq, 64, generator=g).to(dtype))) for _ in range(3)]
    q_s, c_s, pe_s = (t.clone() for t in steps[0])
    pool_g, pool_e = pool.to(dev), pool.to(dev)
    lens_g, lens_e = (torch.tensor(start, dtype=torch.int32, device=dev) for _ in range(2))
    bt_g, bt_e = bt.to(dev), bt.to(dev)

    def step(qq, cc, pp, cache, lens, table):
        lens.add_(Nq)
        return flash_attention_decode_mla(qq, cache, lens, block_table=table, return_lse=True, num_splits=3, kv_c=cc, k_pe=pp, rotary_cos=cos, rotary_sin=sin,
                                          rotary_interleaved=False)
    warm = pool.to(dev)
    step(q_s, c_s, pe_s, warm, torch.tensor(start, dtype=torch.int32, device=dev), bt_g)      # (warm-up: the library is loaded outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = step(q_s, c_s, pe_s, pool_g, lens_g, bt_g)
    lens_g.copy_(torch.tensor(start, dtype=torch.int32))          # the capture itself ran nothing: the lengths are where they started
    for n, (qq, cc, pp) in enumerate(steps):
        if n == 2:
            for table in (bt_g, bt_e):
                table.copy_(table[:, [1, 0, 2, 3]])
        q_s.copy_(qq), c_s.copy_(cc), pe_s.copy_(pp)
        graph.replay()
        torch.cuda.synchronize()
        o_e, lse_e = step(qq, cc, pp, pool_e, lens_e, bt_e)
        torch.cuda.synchronize()
        assert torch.equal(lens_g, lens_e) and lens_e.tolist() == [s + (n + 1) * Nq for s in start]
        assert torch.equal(o.view(torch.int16), o_e.view(torch.int16)) and torch.equal(lse, lse_e), n
        assert same_bits(pool_g, pool_e), n
    assert not same_bits(pool_g, pool), "the steps wrote their tokens"


# ---------------------------------------------------------------------------------------------------------------- far offsets
PAGE_STRIDE = 64 * fl.MIB + 5 * 4096          # bytes from page to page
POOL_BASE = 8 * fl.MIB
NUM_PAGES = 67                                # pages 32 .. 63 start between 2^31 and 2^32, pages 64 .. 66 past 2^32
SMALL = 1 * fl.MIB                            # the sources, q and cache_seqlens: in front of the pool
FAR_SMALL = POOL_BASE + NUM_PAGES * PAGE_STRIDE + fl.MIB      # the block table: behind it, past 2^32


def test_target_pages_past_2_and_4_gib_and_nothing_else_is_written():
    """One poisoned buffer of 4.25 GiB (tests/test_decode_mla_far_gpu.py's layout): the pages the new tokens land in start past byte offsets 2^31 and
    2^32, the block table lies past 2^32.  The written rows equal the expected rows bit for bit; with them and the inputs poisoned again, every byte of
    the buffer is poison — one pass over the whole buffer, which stands in for windows and samples and stays in seconds."""
    dev = dc.dev()
    if torch.cuda.get_device_properties(dev).total_memory < 3 * fl.ARENA_BYTES:
        pytest.skip("needs %d GiB of device memory" % (3 * fl.ARENA_BYTES // fl.GIB))
    dtype, B, nnew, H, page = BF16, 3, 2, 4, 64
    lens = [130, 65, 200]                                         # positions 128 129 | 63 64 | 198 199: slots 2 | 0 and 1 | 3
    assert POOL_BASE + 32 * PAGE_STRIDE > 2 ** 31 and POOL_BASE + 64 * PAGE_STRIDE > 2 ** 32 and FAR_SMALL > 2 ** 32 and FAR_SMALL + fl.MIB <= fl.ARENA_BYTES
    bt = torch.tensor([[-3, NUM_PAGES + 9][i % 2] for i in range(B * 4)], dtype=torch.int32).view(B, 4)      # unused entries: ids outside the pool
    bt[0, 2], bt[1, 0], bt[1, 1], bt[2, 3] = 33, 64, 40, 66
    kv_c, k_pe, q = ar.inputs(B * nnew, H, dtype, 71)
    cos, sin = ar.tables(SEQLEN_RO)
    arena = fl.new_arena(fl.ARENA_BYTES, dev)
    pool = arena.view(dtype).as_strided((NUM_PAGES, page, D), (PAGE_STRIDE // 2, D, 1), POOL_BASE // 2)

    def small(t, at):           # a copy of t inside the arena at byte offset `at` (16-byte aligned)
        raw = arena[at:at + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
        raw.copy_(t)
        return raw
    at = [SMALL + i * 512 * 1024 for i in range(4)]
    ca, pa = small(kv_c.view(B, nnew, DV).to(dev), at[0]), small(k_pe.view(B, nnew, 64).to(dev), at[1])
    qa, la = small(q.view(B, nnew, H, D).to(dev), at[2]), small(torch.tensor(lens, dtype=torch.int32, device=dev), at[3])
    bta = small(bt.to(dev), FAR_SMALL)
    got_q = kvcache_append_mla(pool, ca, pa, la, block_table=bta, rotary_cos=cos.to(dev), rotary_sin=sin.to(dev), rotary_interleaved=False, q=qa)
    torch.cuda.synchronize()
    # the expected rows, from a compact image of the four target pages under a table of its own numbering
    ids = [33, 64, 40, 66]
    bt_c = torch.zeros(B, 4, dtype=torch.int32)
    bt_c[0, 2], bt_c[1, 0], bt_c[1, 1], bt_c[2, 3] = 0, 1, 2, 3
    blank = torch.full((4, page, D), -1, dtype=torch.int16).view(dtype)                      # the arena's poison: 0xFF bytes
    want, want_q = ar.expect(blank, kv_c, k_pe, ar.uniform_owners(B, nnew), lens, bt_c, q, cos, sin, False)
    assert same_bits(got_q.view(B * nnew, H, D), want_q)
    for n, pid in enumerate(ids):
        assert same_bits(pool[pid], want[n]), pid
    assert int((ar.bits(want) != -1).any(-1).sum()) == B * nnew
    assert same_bits(ca, kv_c.view(B, nnew, DV)) and same_bits(pa, k_pe.view(B, nnew, 64)) and same_bits(qa, q.view(B, nnew, H, D)) and torch.equal(bta.cpu(), bt)
    for t in [pool[pid] for pid in ids] + [ca, pa, qa, la, bta]:
        t.view(torch.int16 if t.element_size() == 2 else torch.int32).fill_(-1)
    assert fl.arena_is_poison(arena), "first stray byte at %r" % fl.first_stray_byte(arena)
