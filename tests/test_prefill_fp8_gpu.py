"""Chunked prefill on e4m3 KV caches on the GPU (fa2_fwd_prefill_fp8, flash_attention_prefill_fp8).  Every case runs with option "rows" at 128 and at 256; every
cache is a NaN-filled 16-bit cache of prefill_calls' builders converted to e4m3, so every dead slot, spare page and page behind an unused block-table entry
(-1 / 2**30) holds the e4m3 NaN code 0x7f; o and lse start as NaN.  Two yardsticks, both the project's own:
  1. with descales that are null or powers of two in [1/8, 8] per (sequence, K / V head), fa2_fwd_prefill on the 16-bit cache (float(code) * descale) — exact in
     fp16 and bf16 — BIT FOR BIT, o and lse: the factors commute with every rounding, and everything after the staging is shared;
  2. with general descales (0.37 .. 2.9, different per sequence and head), float64 on the exact dequantised values with tools/key_bars.py's per-element O bar and
     conftest's LSE_TOL (prefill_calls.check_float64)."""
import pytest
import torch

import prefill_calls as pc
import prefill_fp8_calls as p8
from conftest import LSE_TOL
from rocwmma_fattn import FlashAttn, _fa2_lib

pytestmark = pytest.mark.gpu

LENS = (700, 300, 129, 65, 64, 2, 1, 0, 40)
NQS = (300, 257, 129, 65, 1, 2, 1, 0, 64)          # the last sequence has more queries than keys; the first two cross a 128- and a 256-row block
NMAX = 717
F16, BF16 = torch.float16, torch.bfloat16
E4M3 = p8.E4M3


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    return torch.device("cuda", 0)


@pytest.fixture(params=[128, 256])
def rows(request):
    before = _fa2_lib.load().fa2_get_option(b"rows")
    _fa2_lib.set_option("rows", request.param)
    yield request.param
    _fa2_lib.set_option("rows", before)


def lens_t(lens):
    return torch.tensor(lens, dtype=torch.int32, device=dev())


def slopes_bh(B, H):
    g = torch.Generator().manual_seed(5)
    return (torch.rand((B, H), generator=g) * 0.05).to(dev())


def cache8(c, page=0, per=0, nmax=NMAX, **kw):
    """The case's codes as an e4m3 cache -> (kc, vc, bt): contiguous (page = 0) or a shuffled pool of `page`-key pages under a table of `per` entries."""
    if page == 0:
        k16, v16 = pc.contiguous_cache(c["kc"], c["vc"], nmax)
        return p8.to_e4m3(k16), p8.to_e4m3(v16), None
    k16, v16, bt = pc.paged_cache(c["kc"], c["vc"], page, per, **kw)
    return p8.to_e4m3(k16), p8.to_e4m3(v16), bt


def run8(c, cache, max_q, scale, window_left=-1, softcap=0.0, slopes=None, lens=None):
    kc, vc, bt = cache
    return p8.prefill_fp8_c(c["q"], kc, vc, c["cu"], lens_t(c["lens"]) if lens is None else lens, bt, max_q, scale, c["kd"], c["vd"], window_left, softcap, slopes)


def twin16(c, max_q, scale, window_left=-1, softcap=0.0, slopes=None, nmax=None):
    """fa2_fwd_prefill on the contiguous 16-bit cache of the exact dequantised values (paging is invisible to that call: tests/test_prefill_gpu.py)."""
    dtype = c["q"].dtype
    kt, vt = p8.as_dtype(c["kt"], dtype), p8.as_dtype(c["vt"], dtype)
    k16, v16 = pc.contiguous_cache(kt, vt, nmax if nmax is not None else max(max(c["lens"]), 1))
    return pc.prefill_c(c["q"], k16, v16, c["cu"], lens_t(c["lens"]), None, max_q, scale, window_left, softcap, slopes)


def assert_same_bits(tag, got, want):
    assert pc.bits_equal(got[0], want[0]), "%s: o differs in %d elements" % (tag, int((got[0].float() != want[0].float()).sum()))
    assert pc.bits_equal(got[1], want[1]), "%s: lse differs in %d elements" % (tag, int((got[1] != want[1]).sum()))


BASE_SHAPES = [(4, 2, 64, F16), (4, 2, 64, BF16), (4, 1, 128, F16), (4, 2, 128, BF16), (4, 2, 80, F16), (2, 1, 256, BF16)]


@pytest.mark.parametrize("H,Hkv,D,dtype", BASE_SHAPES, ids=lambda v: str(v).replace("torch.", ""))
def test_base_case_equals_the_16_bit_twin_bit_for_bit_and_meets_the_float64_bars(rows, H, Hkv, D, dtype):
    scale, max_q = D ** -0.5, max(NQS)
    exact = p8.make_case(LENS, NQS, H, Hkv, D, dtype, 11, dev(), descales="pow2")
    plain = p8.make_case(LENS, NQS, H, Hkv, D, dtype, 11, dev(), descales=None)
    general = p8.make_case(LENS, NQS, H, Hkv, D, dtype, 11, dev(), descales="general")
    layouts = {"contiguous": dict(), "pages64": dict(page=64, per=13, seed=3, share=(0, 1))}
    dead = slice(int(exact["cu"][8]), int(exact["cu"][8]) + 24)          # the last sequence: 64 queries on 40 keys, the first 24 rows sit at negative positions
    for softcap, slopes in ((0.0, None), (30.0, slopes_bh(len(LENS), H))):
        for c, kind in ((exact, "pow2"), (plain, "null")):
            want = twin16(c, max_q, scale, -1, softcap, slopes)
            for name, kw in layouts.items():
                if kind == "null" and name != "contiguous":
                    continue
                assert_same_bits("%s %s descales softcap %g" % (name, kind, softcap), run8(c, cache8(c, **kw), max_q, scale, -1, softcap, slopes), want)
        ref = pc.reference(general["q"], general["cu"], general["kt"], general["vt"], scale, -1, softcap, slopes)
        for name, kw in layouts.items():
            got = run8(general, cache8(general, **kw), max_q, scale, -1, softcap, slopes)
            assert not pc.check_float64("%s general descales softcap %g" % (name, softcap), got[0], got[1], ref)
            assert float(got[0][dead].abs().max()) == 0.0 and bool(torch.isinf(got[1][:, dead]).all()) and bool((got[1][:, dead] < 0).all())


def test_paging_is_invisible(rows):
    H, Hkv, D, dtype = 4, 2, 128, F16
    c = p8.make_case(LENS, NQS, H, Hkv, D, dtype, 11, dev(), descales="general")
    scale, max_q = D ** -0.5, max(NQS)
    kc, vc, _ = cache8(c)
    want = run8(c, (kc, vc, None), max_q, scale)
    for page in (64, 128, 192):
        pk, pv, bt = cache8(c, page=page, per=-(-NMAX // page) + 1, seed=page, share=(0, 1))
        assert int(bt[0, 0]) == int(bt[1, 0])
        assert_same_bits("page %d" % page, run8(c, (pk, pv, bt), max_q, scale), want)
    # K and V as column slices of ONE wider byte tensor whose other bytes are NaN codes
    wide = torch.full((len(LENS), NMAX, Hkv, 2 * D + 32), p8.NAN_BYTE, dtype=torch.uint8, device=kc.device)
    wide[..., 16:16 + D], wide[..., D + 32:2 * D + 32] = kc.view(torch.uint8), vc.view(torch.uint8)
    views = wide[..., 16:16 + D].view(E4M3), wide[..., D + 32:2 * D + 32].view(E4M3)
    assert_same_bits("strided view", run8(c, views + (None,), max_q, scale), want)


def test_lengths_and_page_ids_are_clamped(rows):
    H, Hkv, D, dtype = 4, 2, 64, BF16
    nqs, cap = (130, 40, 3), 320
    c = p8.make_case((cap, cap, cap), nqs, H, Hkv, D, dtype, 21, dev(), descales="general", prefix=False)
    scale = D ** -0.5
    kc, vc, _ = cache8(c, nmax=cap)
    want = run8(c, (kc, vc, None), 130, scale, lens=lens_t((cap, cap, 0)))
    assert_same_bits("lengths", run8(c, (kc, vc, None), 130, scale, lens=lens_t((cap + 80, 2 ** 31 - 1, -5))), want)
    # page ids: a pool of 15 pages, every one of them valid data; ids below 0 read page 0, ids at or above 15 read page 14
    pool = [p8.to_e4m3(torch.cat(t).view(15, 64, Hkv, D)) for t in (c["kc"], c["vc"])]
    good = torch.tensor([[0, 3, 14, 7, 0], [14, 14, 2, 0, 9], [1, 0, 14, 4, 5]], dtype=torch.int32, device=kc.device)
    wild = torch.tensor([[-7, 3, 15, 7, -2 ** 31], [2 ** 31 - 1, 14, 2, -1, 9], [1, -3, 2 ** 30, 4, 5]], dtype=torch.int32, device=kc.device)
    lens = lens_t((cap, 300, 170))
    assert_same_bits("page ids", run8(c, (pool[0], pool[1], wild), 130, scale, lens=lens), run8(c, (pool[0], pool[1], good), 130, scale, lens=lens))


def test_pages_below_the_window_are_never_addressed(rows):
    H, Hkv, D, dtype, W = 4, 2, 128, BF16, 100
    c = p8.make_case(LENS, NQS, H, Hkv, D, dtype, 11, dev(), descales="pow2")
    scale, max_q = D ** -0.5, max(NQS)
    clean = cache8(c, page=64, per=13, seed=8)
    holed = cache8(c, page=64, per=13, seed=8, visible=lambda b, j: (j + 1) * 64 > LENS[b] - NQS[b] - W)
    assert int((holed[2] != clean[2]).sum()) >= 4          # sequence 0: keys below 300 are out of every row's sight — pages 0 .. 3
    assert int((holed[0].view(torch.uint8) == p8.NAN_BYTE).sum()) > int((clean[0].view(torch.uint8) == p8.NAN_BYTE).sum())
    got = run8(c, holed, max_q, scale, W)
    assert_same_bits("clean cache", got, run8(c, clean, max_q, scale, W))
    assert_same_bits("16-bit twin", got, twin16(c, max_q, scale, W))
    assert not pc.check_float64("window", got[0], got[1], pc.reference(c["q"], c["cu"], c["kt"], c["vt"], scale, W))


def test_a_captured_graph_follows_lengths_table_cache_and_descales_changed_in_place(rows):
    H, Hkv, D, dtype = 4, 2, 128, F16
    lens0, nqs = (300, 129, 64), (100, 129, 1)
    full = p8.make_case((448, 448, 448), nqs, H, Hkv, D, dtype, 41, dev(), descales="general", prefix=False)
    q, cu, scale, per = full["q"], full["cu"], D ** -0.5, 8

    def pool(cur_lens, seed, spare):
        cut = dict(full, kc=[t[:n] for t, n in zip(full["kc"], cur_lens)], vc=[t[:n] for t, n in zip(full["vc"], cur_lens)])
        return cache8(cut, page=64, per=per, seed=seed, spare=spare)

    pk, pv, bt = pool(lens0, 1, 12)
    lens, kd, vd = lens_t(lens0), full["kd"].clone(), full["vd"].clone()
    out = pc.nan_out(q)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        p8.prefill_fp8_c(q, pk, pv, cu, lens, bt, max(nqs), scale, kd, vd, out=out)          # (loads the code objects before the capture)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            p8.prefill_fp8_c(q, pk, pv, cu, lens, bt, max(nqs), scale, kd, vd, out=out)
    for step, new_lens in enumerate(((300, 129, 64), (448, 130, 200), (101, 400, 1))):
        nk, nv, nbt = pool(new_lens, 50 + step, pk.shape[0] - sum(-(-n // 64) for n in new_lens))
        assert nk.shape == pk.shape
        pk.view(torch.uint8).copy_(nk.view(torch.uint8)), pv.view(torch.uint8).copy_(nv.view(torch.uint8)), bt.copy_(nbt), lens.copy_(lens_t(new_lens))
        kd.copy_(p8.general_descales(3, Hkv, 70 + step, kd.device)), vd.copy_(p8.general_descales(3, Hkv, 80 + step, kd.device))
        out[0].fill_(float("nan")), out[1].fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        fresh = p8.prefill_fp8_c(q, pk, pv, cu, lens, bt, max(nqs), scale, kd, vd)
        assert_same_bits("replay %d" % step, out, fresh)
        if step:                  # the descales that were captured are not the ones in use
            stale = p8.prefill_fp8_c(q, pk, pv, cu, lens, bt, max(nqs), scale, full["kd"], full["vd"])
            assert not pc.bits_equal(stale[0], fresh[0])
    # a NaN k_descale for one (sequence, K / V head) poisons the query heads of that group in that sequence, and nothing else
    clean = (out[0].clone(), out[1].clone())
    kd[1, 1] = float("nan")
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    g, r0, r1 = H // Hkv, int(cu[1]), int(cu[2])
    hit_o = torch.zeros(out[0].shape[:2], dtype=torch.bool, device=q.device)
    hit_o[r0:r1, g:2 * g] = True                    # (sequence 1 has 400 keys and 129 queries: every row sees a key)
    assert bool(torch.isnan(out[0][hit_o]).all()) and bool(torch.isnan(out[1].t()[hit_o]).all())
    assert pc.bits_equal(out[0][~hit_o], clean[0][~hit_o]) and pc.bits_equal(out[1].t()[~hit_o], clean[1].t()[~hit_o])


def test_fused_append_equals_append_then_attend(rows):
    H, Hkv, D, dtype = 4, 2, 128, BF16
    lens, nqs = (300, 129, 65, 64), (100, 129, 1, 0)
    c = p8.make_case(lens, nqs, H, Hkv, D, dtype, 51, dev(), descales="general", prefix=False)
    d, q, cu, lt = dev(), c["q"], c["cu"], lens_t(lens)
    g = torch.Generator().manual_seed(52)
    k_new, v_new = (torch.randn((sum(nqs), Hkv, D), generator=g).to(dtype).to(d) for _ in range(2))
    ang = torch.arange(512, dtype=torch.float32)[:, None] * (10000.0 ** (-torch.arange(32, dtype=torch.float32) / 32.0))[None]
    cos, sin = ang.cos().to(d), ang.sin().to(d)
    for page in (0, 64):
        base = cache8(c, page=page, per=7, nmax=320, seed=4)
        caches = [tuple(t.clone() if t is not None else None for t in base) for _ in range(3)]
        kw = dict(max_seqlen_q=max(nqs), window=200, softcap=20.0, k_descale=c["kd"], v_descale=c["vd"], return_lse=True)
        fused = FlashAttn.flash_attention_prefill_fp8(q, caches[0][0], caches[0][1], cu, lt, caches[0][2], k=k_new, v=v_new, rotary_cos=cos, rotary_sin=sin, **kw)
        q_rot = FlashAttn.kvcache_append_varlen(caches[1][0], caches[1][1], k_new, v_new, cu, lt, caches[1][2], cos, sin, True, c["kd"], c["vd"], q=q)
        split = FlashAttn.flash_attention_prefill_fp8(q_rot, caches[1][0], caches[1][1], cu, lt, caches[1][2], **kw)
        assert pc.bits_equal(fused[0], split[0]) and pc.bits_equal(fused[1], split[1]), page
        for a, b in zip(caches[0][:2], caches[1][:2]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), page
        assert not torch.equal(caches[0][0].view(torch.uint8), base[0].view(torch.uint8))          # (the append wrote something)
        # a refused call leaves the caches untouched
        with pytest.raises(ValueError):
            FlashAttn.flash_attention_prefill_fp8(q, caches[2][0], caches[2][1], cu, lt, caches[2][2], k=k_new, v=v_new, rotary_cos=cos, rotary_sin=sin,
                                                  **dict(kw, softcap=-1.0))
        with pytest.raises(ValueError):
            FlashAttn.flash_attention_prefill_fp8(q, caches[2][0], caches[2][1], cu, lt, caches[2][2], k=k_new, v=v_new, rotary_cos=cos, rotary_sin=sin,
                                                  **dict(kw, k_descale=c["kd"][:, :1]))
        torch.cuda.synchronize()
        for a, b in zip(caches[2][:2], base[:2]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), page


def test_decode_rows_agree_with_flash_attention_decode(rows):
    H, Hkv, D, dtype = 4, 2, 128, BF16
    g = torch.Generator().manual_seed(61)
    lens = tuple(int(x) for x in torch.randint(1, 500, (24,), generator=g)) + (400, 130)
    nqs = (1,) * 24 + (130, 130)
    c = p8.make_case(lens, nqs, H, Hkv, D, dtype, 62, dev(), descales="general", prefix=False)
    scale, lt = D ** -0.5, lens_t(lens)
    kc, vc, _ = cache8(c, nmax=512)
    ref = pc.reference(c["q"], c["cu"], c["kt"], c["vt"], scale)
    o, lse = FlashAttn.flash_attention_prefill_fp8(c["q"], kc, vc, c["cu"], lt, max_seqlen_q=130, k_descale=c["kd"], v_descale=c["vd"], return_lse=True)
    assert not pc.check_float64("ragged step", o, lse * pc.LOG2E, ref)
    od, ld = FlashAttn.flash_attention_decode(c["q"][:24].unsqueeze(1), kc[:24], vc[:24], lt[:24], k_descale=c["kd"][:24], v_descale=c["vd"][:24], return_lse=True)
    ref24 = tuple(t[..., :24, :, :] if i != 1 else t[:, :24] for i, t in enumerate(ref))
    assert not pc.check_float64("decode rows", od[:, 0], ld[:, :, 0].transpose(0, 1) * pc.LOG2E, ref24)
    assert not pc.check_float64("prefill's decode rows", o[:24], lse[:, :24] * pc.LOG2E, ref24)


def test_a_seeded_random_slice_equals_the_twin_and_float64(rows):
    g = torch.Generator().manual_seed(2025)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))       # noqa: E731
    fails = []
    for draw in range(20):
        B, H, D = ri(1, 5), (2, 4, 8)[ri(0, 2)], (64, 128)[ri(0, 1)]
        divs = [h for h in (1, 2, 4, 8) if H % h == 0]
        Hkv = divs[ri(0, len(divs) - 1)]
        page = (0, 64, 128, 320)[ri(0, 3)]
        lens = [ri(0, 600) for _ in range(B)]
        nqs = [ri(0, n + 3) for n in lens]
        W = ri(0, 200) if ri(0, 1) else -1
        smod = ri(0, 1)
        dtype = (F16, BF16)[ri(0, 1)]
        if sum(nqs) == 0:
            nqs[0] = 1
        cap = max(max(lens), 1)
        nmax, per, max_q = cap + ri(0, 70), -(-cap // max(page, 1)) + ri(0, 2), max(max(nqs), 1)
        softcap, slopes = (float(ri(5, 50)), slopes_bh(B, H) if ri(0, 1) else slopes_bh(1, H)[0]) if smod else (0.0, None)
        scale = D ** -0.5
        tag = "draw %d B%d H%d Hkv%d D%d page %d lens %s nq %s W %d smod %d %s" % (draw, B, H, Hkv, D, page, lens, nqs, W, smod, dtype)
        layout = dict(nmax=nmax) if page == 0 else dict(page=page, per=per, seed=draw)
        exact = p8.make_case(lens, nqs, H, Hkv, D, dtype, 1000 + draw, dev(), descales="pow2", prefix=False)
        got = run8(exact, cache8(exact, **layout), max_q, scale, W, softcap, slopes)
        want = twin16(exact, max_q, scale, W, softcap, slopes)
        if not (pc.bits_equal(got[0], want[0]) and pc.bits_equal(got[1], want[1])):
            fails.append(tag + ": differs from the 16-bit twin")
        general = p8.make_case(lens, nqs, H, Hkv, D, dtype, 1000 + draw, dev(), descales="general", prefix=False)
        got = run8(general, cache8(general, **layout), max_q, scale, W, softcap, slopes)
        fails += pc.check_float64(tag, got[0], got[1], pc.reference(general["q"], general["cu"], general["kt"], general["vt"], scale, W, softcap, slopes))
    assert not fails, "\n".join(fails)
    assert LSE_TOL == 1e-3
