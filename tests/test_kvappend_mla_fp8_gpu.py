"""GPU tests of the quantising append for an e4m3 latent (MLA) cache of 656-byte rows: kvcache_append_mla / kvcache_append_mla_varlen on a uint8 /
float8_e4m3fn cache (C-ABI fa2_kvcache_append_mla_fp8, fa2_kvcache_append_mla_varlen_fp8).

The expected image has no machinery: mla_append_refs.expect on a poisoned 16-bit shadow cache; every row it changed becomes mla_cache_to_fp8(row) on
the CPU, every other row keeps the uint8 poison.  The WHOLE uint8 cache and the WHOLE q_out are compared bit for bit.  kv_c is scaled so that a swapped
or neighbouring scale shows: the four column groups by (1, 4, 1/4, 16) / 112, token t by 1 + t % 7, and one group of one token is all zeros (scale: the
bits of 1.0, codes 0)."""
import pytest
import torch

import decode_calls as dc
import decode_refs as dr
import far_layouts as fl
import mla_append_refs as ar
import mla_refs as mr
from rocwmma_fattn.FlashAttn import flash_attention_decode_mla, kvcache_append_mla, kvcache_append_mla_varlen, mla_cache_from_fp8, mla_cache_to_fp8
from test_kvappend_mla_gpu import COUNTS, FAR_SMALL, NUM_PAGES, PAGE_STRIDE, POOL_BASE, SEQLEN_RO, SMALL, fused_case, layout, lengths, packed_owners

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
LN2 = 0.6931471805599453
D, DV, ROW = ar.D, ar.DV, 656
POISON8 = 0x5A


def inputs(tokens, H, dtype, seed):
    kv_c, k_pe, q = ar.inputs(tokens, H, dtype, seed)
    group = (torch.tensor([1.0, 4.0, 0.25, 16.0]) / 112.0).repeat_interleave(128)
    kv_c = (kv_c.float() * group * (1 + torch.arange(tokens) % 7)[:, None]).to(dtype)
    if tokens:
        kv_c[tokens // 2, 128:256] = 0.0
    return kv_c, k_pe, q


def image8(shadow, img, poison=POISON8):
    """the uint8 image: the rows expect() changed in the 16-bit shadow, quantised on the CPU; every other row poison"""
    want = torch.full(tuple(shadow.shape[:-1]) + (ROW,), poison, dtype=torch.uint8)
    changed = (ar.bits(img) != ar.bits(shadow)).any(-1)
    want[changed] = mla_cache_to_fp8(img[changed])
    return want, changed


def tabs(tab, dtype):
    return (None, None) if tab == "none" else ar.tables(SEQLEN_RO, torch.float32 if tab == "f32" else dtype)


def run(dev, dtype, shadow, bt, owners, lens, kv_c, k_pe, q, cos, sin, inter, cu=None, B=None, as_e4m3=False):
    """One append, uniform (B given: the tokens are [B, Nnew]) or packed (cu given), checked against the image.  -> (cache, q_out) on the device"""
    img, want_q = ar.expect(shadow, kv_c, k_pe, owners, lens, bt, q, cos, sin, inter)
    want, changed = image8(shadow, img)
    up = lambda t: None if t is None else t.to(dev)              # noqa: E731
    cache = torch.full_like(want, POISON8).to(dev)
    arg = cache.view(torch.float8_e4m3fn) if as_e4m3 else cache
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    kw = dict(block_table=up(bt), rotary_cos=up(cos), rotary_sin=up(sin), rotary_interleaved=inter)
    if cu is None:
        sh = lambda t, *w: None if t is None else t.view(B, -1, *w).to(dev)       # noqa: E731
        got_q = kvcache_append_mla(arg, sh(kv_c, DV), sh(k_pe, D - DV), lens_d, q=None if q is None else sh(q, q.shape[1], D), **kw)
    else:
        got_q = kvcache_append_mla_varlen(arg, kv_c.to(dev), k_pe.to(dev), torch.tensor(cu, dtype=torch.int32, device=dev), lens_d, q=up(q), **kw)
    torch.cuda.synchronize()
    got = cache.cpu()
    assert torch.equal(got, want), ("cache image", dtype, lens, int((got != want).any(-1).sum()), int(changed.sum()))
    assert (got_q is None) if q is None else torch.equal(ar.bits(got_q.cpu().view(want_q.shape)), ar.bits(want_q)), ("q_out", dtype, lens)
    return cache, got_q


KINDS, TABS = ("contig", "page64", "page128"), ("f32", "16bit", "none")
SHAPES = [(H, nnew, (3, 1)[n % 2]) for n, (H, nnew) in enumerate((H, nnew) for H in (0, 5, 128) for nnew in (1, 3, 130))] + [(5, 130, 3), (128, 3, 3), (0, 1, 1)]
UNIFORM = [(H, nnew, B, KINDS[n % 3], TABS[n % 3] if H == 0 else TABS[(n // 2) % 2], bool((n // 4 + n) % 2), (F16, BF16)[n % 2], n) for n, (H, nnew, B) in enumerate(SHAPES)]


@pytest.mark.parametrize("case", UNIFORM, ids=lambda c: "H%d-N%d-B%d-%s-%s-%s-%s" % (c[0], c[1], c[2], c[3], c[4], "gptj" if c[5] else "neox", "f16" if c[6] == F16 else "bf16"))
def test_uniform(case):
    H, nnew, B, kind, tab, inter, dtype, n = case
    shadow, bt, cap = layout(kind, B, dtype, torch.Generator().manual_seed(2000 + n))
    kv_c, k_pe, q = inputs(B * nnew, H, dtype, 2000 + n)
    cos, sin = tabs(tab, dtype)
    run(dc.dev(), dtype, shadow, bt, ar.uniform_owners(B, nnew), lengths(B, nnew, cap, n), kv_c, k_pe, q if cos is not None else None, cos, sin, inter, B=B,
        as_e4m3=bool(n % 2))


def test_page_ids_outside_the_pool_are_skipped_and_the_tokens_behind_them_written():
    B, nnew, H, per = 5, 3, 5, 4
    pages = B * per + 1
    bt = torch.randperm(pages, generator=torch.Generator().manual_seed(77))[:B * per].view(B, per).to(torch.int32)
    bt[3, 0], bt[4, 1] = -1, pages                               # sequence 3's first token (position 63), sequence 4's first (position 127)
    shadow = ar.poisoned((pages, 64, D), BF16)
    kv_c, k_pe, q = inputs(B * nnew, H, BF16, 78)
    cos, sin = ar.tables(SEQLEN_RO)
    cache, _ = run(dc.dev(), BF16, shadow, bt, ar.uniform_owners(B, nnew), [70, 130, 200, 66, 130], kv_c, k_pe, q, cos, sin, False, B=B)
    assert int((cache.cpu() != POISON8).any(-1).sum()) == B * nnew - 2, "two tokens are skipped"


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind,H,tab,inter", [("contig", 5, "f32", True), ("page64", 128, "16bit", False)])
def test_packed_counts(kind, H, tab, inter, dtype):
    cap = 200 if kind == "contig" else 256
    cu = [0]
    for c in COUNTS:
        cu.append(cu[-1] + c)
    shadow, bt, _ = layout(kind, len(COUNTS), dtype, torch.Generator().manual_seed(500 + H))
    kv_c, k_pe, q = inputs(cu[-1], H, dtype, 500 + H)
    cos, sin = tabs(tab, dtype)
    run(dc.dev(), dtype, shadow, bt, packed_owners(COUNTS, cu[-1]), [50, cap, 140, 2, 0, 150], kv_c, k_pe, q, cos, sin, inter, cu=cu)


def test_a_partly_filled_token_buffer_and_packed_equals_uniform():
    dev = dc.dev()
    cu, total = [2, 5, 5, 9], 16
    owners = [None] * 2 + [(0, i, 3) for i in range(3)] + [(2, i, 4) for i in range(4)] + [None] * 7
    shadow, bt, _ = layout("page64", 3, F16, torch.Generator().manual_seed(41))
    kv_c, k_pe, q = inputs(total, 5, F16, 41)
    cos, sin = ar.tables(SEQLEN_RO)
    _, got_q = run(dev, F16, shadow, bt, owners, [40, 9, 100], kv_c, k_pe, q, cos, sin, True, cu=cu)
    for t in (0, 1, 9, 15):                                      # rows no sequence owns: q comes back bit for bit
        assert torch.equal(ar.bits(got_q[t].cpu()), ar.bits(q[t]))
    B, nnew = 3, 3                                               # equal counts: both calls are held to one image, so they agree
    kv_c, k_pe, q = inputs(B * nnew, 5, F16, 6)
    c1, q1 = run(dev, F16, shadow, bt, ar.uniform_owners(B, nnew), [2, 256, 77], kv_c, k_pe, q, cos, sin, False, B=B)
    c2, q2 = run(dev, F16, shadow, bt, ar.uniform_owners(B, nnew), [2, 256, 77], kv_c, k_pe, q, cos, sin, False, cu=[0, 3, 6, 9])
    assert torch.equal(c1, c2) and torch.equal(ar.bits(q1.cpu()).view(-1), ar.bits(q2.cpu()).view(-1)) and bool((c1 != POISON8).any())


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_strided_cache_and_sources(dtype):
    """The cache a view with a 672-byte row pitch inside a poisoned buffer: the 16 bytes between rows stay poison.  kv_c and k_pe the two slices of one
    [B, Nnew, 584] buffer: not copied, not touched."""
    dev = dc.dev()
    B, nnew, H, cap = 3, 3, 5, 200
    lens = [2, 200, 77]
    kv_c, k_pe, q = inputs(B * nnew, H, dtype, 31)
    cos, sin = ar.tables(SEQLEN_RO, dtype)
    shadow = ar.poisoned((B, cap, D), dtype)
    img, want_q = ar.expect(shadow, kv_c, k_pe, ar.uniform_owners(B, nnew), lens, None, q, cos, sin, False)
    want = torch.full((B, cap, 672), POISON8, dtype=torch.uint8)
    want[..., :ROW] = image8(shadow, img)[0]
    proj = ar.poisoned((B, nnew, 584), dtype)
    proj[..., :DV], proj[..., DV:D] = kv_c.view(B, nnew, DV), k_pe.view(B, nnew, 64)
    under, proj_d = torch.full_like(want, POISON8).to(dev), proj.to(dev)
    got_q = kvcache_append_mla(under[..., :ROW], proj_d[..., :DV], proj_d[..., DV:D], torch.tensor(lens, dtype=torch.int32, device=dev), rotary_cos=cos.to(dev),
                               rotary_sin=sin.to(dev), rotary_interleaved=False, q=q.view(B, nnew, H, D).to(dev))
    assert torch.equal(under.cpu(), want) and torch.equal(ar.bits(got_q.cpu().view(want_q.shape)), ar.bits(want_q))
    assert torch.equal(ar.bits(proj_d.cpu()), ar.bits(proj)), "the sources are not touched"


def test_one_nan_becomes_a_nan_code_and_no_other_row_differs():
    dev = dc.dev()
    B, nnew = 2, 3
    shadow, bt, _ = layout("page64", B, BF16, torch.Generator().manual_seed(9))
    kv_c, k_pe, _ = inputs(B * nnew, 0, BF16, 9)
    kv_c[4, 300] = float("nan")
    lens = [70, 130]                                             # every token is written
    img, _ = ar.expect(shadow, kv_c, k_pe, ar.uniform_owners(B, nnew), lens, bt)
    want, changed = image8(shadow, img)
    cache = torch.full_like(want, POISON8).to(dev)
    kvcache_append_mla(cache, kv_c.view(B, nnew, DV).to(dev), k_pe.view(B, nnew, 64).to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), block_table=bt.to(dev))
    got = cache.cpu()
    at = tuple(torch.isnan(img.float()).any(-1).nonzero()[0].tolist())      # the row that holds the NaN
    assert int(got[at][300]) & 0x7F == 0x7F, "a NaN is stored as a NaN code"
    got[at], want[at] = 0, 0
    assert torch.equal(got, want) and int(changed.sum()) == B * nnew


def test_target_pages_past_2_and_4_gib_and_nothing_else_is_written():
    """tests/test_kvappend_mla_gpu.py's far layout with pages of 64 rows of 656 bytes: the target pages start past byte offsets 2^31 and 2^32, the block
    table lies past 2^32.  The written rows are exact; with them and the inputs poisoned again, every byte of the arena is poison."""
    dev = dc.dev()
    if torch.cuda.get_device_properties(dev).total_memory < 3 * fl.ARENA_BYTES:
        pytest.skip("needs %d GiB of device memory" % (3 * fl.ARENA_BYTES // fl.GIB))
    dtype, B, nnew, H, page = BF16, 3, 2, 4, 64
    lens = [130, 65, 200]                                         # positions 128 129 | 63 64 | 198 199: slots 2 | 0 and 1 | 3
    bt = torch.tensor([[-3, NUM_PAGES + 9][i % 2] for i in range(B * 4)], dtype=torch.int32).view(B, 4)      # unused entries: ids outside the pool
    ids = [33, 64, 40, 66]
    bt[0, 2], bt[1, 0], bt[1, 1], bt[2, 3] = ids
    kv_c, k_pe, q = inputs(B * nnew, H, dtype, 71)
    cos, sin = ar.tables(SEQLEN_RO)
    arena = fl.new_arena(fl.ARENA_BYTES, dev)
    pool = arena.as_strided((NUM_PAGES, page, ROW), (PAGE_STRIDE, ROW, 1), POOL_BASE)
    assert POOL_BASE + 32 * PAGE_STRIDE > 2 ** 31 and POOL_BASE + 64 * PAGE_STRIDE > 2 ** 32 and PAGE_STRIDE % 16 == 0 and page * ROW <= PAGE_STRIDE

    def small(t, at):           # a copy of t inside the arena at byte offset `at` (16-byte aligned)
        raw = arena[at:at + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
        raw.copy_(t)
        return raw
    ca, pa = small(kv_c.view(B, nnew, DV).to(dev), SMALL), small(k_pe.view(B, nnew, 64).to(dev), SMALL + 512 * 1024)
    qa, la = small(q.view(B, nnew, H, D).to(dev), SMALL + 1024 * 1024), small(torch.tensor(lens, dtype=torch.int32, device=dev), SMALL + 1536 * 1024)
    bta = small(bt.to(dev), FAR_SMALL)
    got_q = kvcache_append_mla(pool, ca, pa, la, block_table=bta, rotary_cos=cos.to(dev), rotary_sin=sin.to(dev), rotary_interleaved=False, q=qa)
    torch.cuda.synchronize()
    bt_c = torch.zeros(B, 4, dtype=torch.int32)                  # the expected rows: a compact image of the four target pages
    bt_c[0, 2], bt_c[1, 0], bt_c[1, 1], bt_c[2, 3] = 0, 1, 2, 3
    blank = torch.full((4, page, D), -1, dtype=torch.int16).view(dtype)
    img, want_q = ar.expect(blank, kv_c, k_pe, ar.uniform_owners(B, nnew), lens, bt_c, q, cos, sin, False)
    want, changed = image8(blank, img, fl.POISON)
    assert int(changed.sum()) == B * nnew and torch.equal(ar.bits(got_q.cpu().view(want_q.shape)), ar.bits(want_q))
    for n, pid in enumerate(ids):
        assert torch.equal(pool[pid].cpu(), want[n]), pid
    for t in [pool[pid] for pid in ids] + [ca, pa, qa, la, bta]:
        t.view(torch.uint8).fill_(fl.POISON)
    assert fl.arena_is_poison(arena), "first stray byte at %r" % fl.first_stray_byte(arena)


# ---------------------------------------------------------------------------------------------------------------- the step, end to end
def logical(pool, bt, nmax):
    return pool if bt is None else torch.stack([pool[bt[b].long()].reshape(-1, pool.shape[-1])[:nmax] for b in range(bt.shape[0])])


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", ["contig", "page64"])
@pytest.mark.parametrize("Nq", [1, 2])
def test_append_then_decode_is_the_16_bit_call_on_the_dequantised_cache_and_meets_the_float64_bars(Nq, kind, dtype):
    dev = dc.dev()
    inter = Nq == 1
    q, kv_c, k_pe, lens, before, bt, cos, sin, q_ref, _ = fused_case(dtype, Nq, kind, inter, 300 + Nq)
    up = lambda t: None if t is None else t.to(dev)              # noqa: E731
    lens_d, cache8 = torch.tensor(lens, dtype=torch.int32, device=dev), mla_cache_to_fp8(before).to(dev)
    q_rot = kvcache_append_mla(cache8, kv_c.to(dev), k_pe.to(dev), lens_d, block_table=up(bt), rotary_cos=cos.to(dev), rotary_sin=sin.to(dev), rotary_interleaved=inter,
                               q=q.to(dev))
    o, lse = flash_attention_decode_mla(q_rot, cache8, lens_d, block_table=up(bt), num_splits=3, return_lse=True, scale=mr.SCALE)
    deq = mla_cache_from_fp8(cache8, dtype)
    o2, l2 = flash_attention_decode_mla(q_rot, deq, lens_d, block_table=up(bt), num_splits=3, return_lse=True, scale=mr.SCALE)
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16)) and torch.equal(lse, l2)
    code = dc.code(dtype)
    dr.check(o, lse / LN2, mr.refs(q_ref, logical(deq.cpu(), bt, 256), lens, code), lens, code, ("fp8 step", Nq, kind))


def test_graph_replay_of_a_whole_step():
    """Captured once: the lengths incremented in place, the quantising append, the e4m3 decode.  Replayed for three steps while the new tokens, the
    lengths and — before the last step — the block table change in place: the cache bytes, o and lse equal an eager trace on a cache of its own."""
    dev = dc.dev()
    dtype, B, H, Nq, page = BF16, 3, 16, 1, 64
    g = torch.Generator().manual_seed(17)
    start = [62, 127, 5]                                          # the steps cross a page boundary in two of the sequences
    pages = B * 4 + 1
    bt = torch.randperm(pages, generator=g)[:B * 4].view(B, 4).to(torch.int32)
    pool = mla_cache_to_fp8(torch.randn(pages, page, D, generator=g).to(dtype))
    cos, sin = (t.to(dev) for t in ar.tables(256))
    steps = [tuple(t.to(dev) for t in (torch.randn(B, Nq, H, D, generator=g).to(dtype), torch.randn(B, Nq, DV, generator=g).to(dtype),
                                       torch.randn(B, Nq, 64, generator=g).to(dtype))) for _ in range(3)]
    q_s, c_s, pe_s = (t.clone() for t in steps[0])
    pool_g, pool_e = pool.to(dev), pool.to(dev)
    lens_g, lens_e = (torch.tensor(start, dtype=torch.int32, device=dev) for _ in range(2))
    bt_g, bt_e = bt.to(dev), bt.to(dev)

    def step(qq, cc, pp, cache, lens, table):
        lens.add_(Nq)
        q_rot = kvcache_append_mla(cache, cc, pp, lens, block_table=table, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=False, q=qq)
        return flash_attention_decode_mla(q_rot, cache, lens, block_table=table, return_lse=True, num_splits=3)
    step(q_s, c_s, pe_s, pool.to(dev), torch.tensor(start, dtype=torch.int32, device=dev), bt_g)      # (warm-up: the library is loaded outside the capture)
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
        assert torch.equal(pool_g, pool_e), n
    assert not torch.equal(pool_g.cpu(), pool), "the steps wrote their tokens"
