"""Chunked prefill against a KV cache on the GPU (fa2_fwd_prefill, flash_attention_prefill).  Every case runs with option "rows" at 128 and at 256; every cache
holds NaN at and beyond every length, in spare pages and in pages behind unused block-table entries, which hold -1 and 2**30; o and lse start as NaN.
The yardsticks: fa2_fwd_varlen (causal, bottom-right, the same window; fa2_fwd_varlen_scoremod with a cap or slopes) on the keys gathered into a packed
copy, BIT FOR BIT — the two calls stage the same 64-key tiles in the same order and share every later instruction — and float64 with tools/key_bars.py's
per-element O bar and conftest's LSE_TOL."""
import pytest
import torch

import key_probes as kp
import prefill_calls as pc
from conftest import LSE_TOL
from rocwmma_fattn import FlashAttn, _fa2_lib

pytestmark = pytest.mark.gpu

LENS = (700, 300, 129, 65, 64, 2, 1, 0, 40)
NQS = (300, 257, 129, 65, 1, 2, 1, 0, 64)          # the last sequence has more queries than keys; the first two cross a 128- and a 256-row block
NMAX = 717
F16, BF16 = torch.float16, torch.bfloat16


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


def base_inputs(H, Hkv, D, dtype, seed=11, lens=LENS, nqs=NQS):
    q, cu, ks, vs = pc.make_inputs(lens, nqs, H, Hkv, D, dtype, seed, dev())
    if len(lens) > 1 and lens[1] >= 192 and lens[0] >= 192:      # a common prefix: the first 192 keys of sequence 1 are sequence 0's
        ks[1][:192], vs[1][:192] = ks[0][:192], vs[0][:192]
    return q, cu, ks, vs


def lens_t(lens):
    return torch.tensor(lens, dtype=torch.int32, device=dev())


def slopes_bh(B, H):
    g = torch.Generator().manual_seed(5)
    return (torch.rand((B, H), generator=g) * 0.05).to(dev())


def run_both(q, cu, ks, vs, cache, max_q, scale, window_left=-1, softcap=0.0, slopes=None):
    """-> (o, lse) of the prefill call on `cache` = (kc, vc, bt) and of the gathered packed twin."""
    kc, vc, bt = cache
    lens = lens_t([t.shape[0] for t in ks])
    got = pc.prefill_c(q, kc, vc, cu, lens, bt, max_q, scale, window_left, softcap, slopes)
    kpk, vpk, cu_k = pc.packed_copy(ks, vs)
    twin = pc.varlen_c(q, kpk, vpk, cu, cu_k, max_q, max(max(t.shape[0] for t in ks), 1), scale, window_left, softcap, slopes)
    return got, twin


def assert_same_bits(tag, got, want):
    assert pc.bits_equal(got[0], want[0]), "%s: o differs in %d elements" % (tag, int((got[0].float() != want[0].float()).sum()))
    assert pc.bits_equal(got[1], want[1]), "%s: lse differs in %d elements" % (tag, int((got[1] != want[1]).sum()))


BASE_SHAPES = [(4, 2, 64, F16), (4, 2, 64, BF16), (4, 1, 64, F16), (4, 1, 64, BF16), (4, 2, 128, F16), (4, 2, 128, BF16), (4, 1, 128, F16), (4, 1, 128, BF16),
               (4, 2, 80, F16), (2, 1, 256, BF16), (2, 1, 512, F16)]


@pytest.mark.parametrize("H,Hkv,D,dtype", BASE_SHAPES, ids=lambda v: str(v).replace("torch.", ""))
def test_base_case_equals_the_packed_twin_bit_for_bit_and_meets_the_float64_bars(rows, H, Hkv, D, dtype):
    q, cu, ks, vs = base_inputs(H, Hkv, D, dtype)
    scale = D ** -0.5
    caches = {"contiguous": tuple(pc.contiguous_cache(ks, vs, NMAX)) + (None,), "pages64": pc.paged_cache(ks, vs, 64, 13, seed=3, share=(0, 1))}
    for softcap, slopes in ((0.0, None), (30.0, slopes_bh(len(LENS), H))):
        ref = pc.reference(q, cu, ks, vs, scale, -1, softcap, slopes)
        for name, cache in caches.items():
            tag = "%s softcap %g" % (name, softcap)
            got, twin = run_both(q, cu, ks, vs, cache, max(NQS), scale, -1, softcap, slopes)
            assert_same_bits(tag, got, twin)
            assert not pc.check_float64(tag, got[0], got[1], ref)
        dead = slice(int(cu[8]), int(cu[8]) + 24)          # the last sequence: 64 queries on 40 keys, the first 24 rows sit at negative positions
        assert float(got[0][dead].abs().max()) == 0.0 and bool(torch.isinf(got[1][:, dead]).all())


def test_paging_is_invisible(rows):
    H, Hkv, D, dtype = 4, 2, 128, F16
    q, cu, ks, vs = base_inputs(H, Hkv, D, dtype)
    lens, scale = lens_t(LENS), D ** -0.5
    kc, vc = pc.contiguous_cache(ks, vs, NMAX)
    want = pc.prefill_c(q, kc, vc, cu, lens, None, max(NQS), scale)
    for page in (64, 128, 192):
        pk, pv, bt = pc.paged_cache(ks, vs, page, -(-NMAX // page) + 1, seed=page, share=(0, 1))
        assert int(bt[0, 0]) == int(bt[1, 0])
        assert_same_bits("page %d" % page, pc.prefill_c(q, pk, pv, cu, lens, bt, max(NQS), scale), want)
    wide = [torch.full((len(LENS), NMAX, Hkv, 2 * D + 8), float("nan"), dtype=dtype, device=q.device) for _ in range(2)]
    wide[0][..., 8:8 + D], wide[1][..., D:2 * D] = kc, vc
    assert_same_bits("strided view", pc.prefill_c(q, wide[0][..., 8:8 + D], wide[1][..., D:2 * D], cu, lens, None, max(NQS), scale), want)


def test_lengths_and_page_ids_are_clamped(rows):
    H, Hkv, D, dtype = 4, 2, 64, BF16
    nqs, cap = (130, 40, 3), 320
    q, cu, ks, vs = pc.make_inputs((cap, cap, cap), nqs, H, Hkv, D, dtype, 21, dev())
    kc, vc = pc.contiguous_cache(ks, vs, cap)
    scale = D ** -0.5
    want = pc.prefill_c(q, kc, vc, cu, lens_t((cap, cap, 0)), None, 130, scale)
    assert_same_bits("lengths", pc.prefill_c(q, kc, vc, cu, lens_t((cap + 80, 2 ** 31 - 1, -5)), None, 130, scale), want)
    # page ids: a pool of 15 pages, every one of them valid data; ids below 0 read page 0, ids at or above 15 read page 14
    pool = [torch.cat(t).view(15, 64, Hkv, D) for t in (ks, vs)]
    good = torch.tensor([[0, 3, 14, 7, 0], [14, 14, 2, 0, 9], [1, 0, 14, 4, 5]], dtype=torch.int32, device=q.device)
    wild = torch.tensor([[-7, 3, 15, 7, -2 ** 31], [2 ** 31 - 1, 14, 2, -1, 9], [1, -3, 2 ** 30, 4, 5]], dtype=torch.int32, device=q.device)
    lens = lens_t((cap, 300, 170))
    assert_same_bits("page ids", pc.prefill_c(q, pool[0], pool[1], cu, lens, wild, 130, scale), pc.prefill_c(q, pool[0], pool[1], cu, lens, good, 130, scale))


def test_pages_below_the_window_are_never_addressed(rows):
    H, Hkv, D, dtype, W = 4, 2, 128, BF16, 100
    q, cu, ks, vs = base_inputs(H, Hkv, D, dtype)
    lens, scale = lens_t(LENS), D ** -0.5
    clean = pc.paged_cache(ks, vs, 64, 13, seed=8)
    holed = pc.paged_cache(ks, vs, 64, 13, seed=8, visible=lambda b, j: (j + 1) * 64 > LENS[b] - NQS[b] - W)
    assert int((holed[2] != clean[2]).sum()) >= 4          # sequence 0: keys below 300 are out of every row's sight — pages 0 .. 3
    got = pc.prefill_c(q, holed[0], holed[1], cu, lens, holed[2], max(NQS), scale, W)
    assert_same_bits("clean cache", got, pc.prefill_c(q, clean[0], clean[1], cu, lens, clean[2], max(NQS), scale, W))
    kpk, vpk, cu_k = pc.packed_copy(ks, vs)
    assert_same_bits("windowed twin", got, pc.varlen_c(q, kpk, vpk, cu, cu_k, max(NQS), max(LENS), scale, W))
    assert not pc.check_float64("window", got[0], got[1], pc.reference(q, cu, ks, vs, scale, W))


def _probe_cache(inp, Nkv):
    """[1, Hkv, N, D] probe tensors -> packed q, per-sequence keys / values and a shuffled pool of 64-key pages."""
    q = inp["q"][0].transpose(0, 1).contiguous()
    ks, vs = [inp["k"][0].transpose(0, 1).contiguous()], [inp["v"][0].transpose(0, 1).contiguous()]
    return q, ks, vs, pc.paged_cache(ks, vs, 64, Nkv // 64 + 2, seed=77)


def test_key_probes_resolve_single_keys_across_64_pages(rows):
    B, H, Hkv, Nq, Nkv, D, dtype = 1, 2, 1, 256, 4096, 128, F16
    d = dev()
    cu, lens = torch.tensor([0, Nq], dtype=torch.int32, device=d), lens_t((Nkv,))
    # counting: k = 0, integer v — a row's O is the mean of the keys it sees and its LSE their count: a skipped or repeated tile changes both
    qc, kc_, vc_ = kp.counting_inputs(B, H, Hkv, Nq, Nkv, D, dtype, 31, d)
    q, ks, vs, (pk, pv, bt) = _probe_cache(dict(q=qc, k=kc_, v=vc_), Nkv)
    o, lse = pc.prefill_c(q, pk, pv, cu, lens, bt, Nq, D ** -0.5)
    # (the expectation and its 1-ulp bar are formed on the CPU: the bar is a power of two there, exactly, and an O that is exactly one ulp off — the
    #  reciprocal-then-round case the bar exists for, 2 of 65 536 elements here — compares equal to it)
    lo, hi = kp.row_ranges(Nq, Nkv, causal=True, bottom_right=True)
    o_exp, lse_exp, o_bar = kp.counting_expect(vc_.cpu(), lo, hi, H, dtype)
    assert not kp.check_counting(o.transpose(0, 1)[None].cpu(), lse[None].cpu(), o_exp, lse_exp, o_bar)
    # pointer: row i's query is c times key pi(i), one key in each of 60 different pages: O is that key's value row, to an ulp
    pi = (torch.arange(Nq, dtype=torch.int64) * 15 + 7) % (Nkv - Nq)
    inp = kp.pointer_inputs(B, H, Hkv, Nq, Nkv, D, dtype, pi, 32, d, visible=kp.brute_mask(Nq, Nkv, causal=True, bottom_right=True, device=d))
    q, ks, vs, (pk, pv, bt) = _probe_cache(inp, Nkv)
    o, lse = pc.prefill_c(q, pk, pv, cu, lens, bt, Nq, inp["scale"])
    o_exp, o_bar = kp.pointer_expect_o(inp, dtype)
    assert not kp.check_elements("O", o.transpose(0, 1)[None], o_exp, o_bar)
    lerr = float((lse.double() - kp.pointer_expect_lse(inp, dtype)).abs().max())
    assert lerr <= kp.pointer_lse_bar(inp, dtype, False), lerr


def test_a_captured_graph_follows_lengths_table_and_cache_changed_in_place(rows):
    H, Hkv, D, dtype = 4, 2, 128, F16
    lens0, nqs = (300, 129, 64), (100, 129, 1)
    q, cu, ks, vs = pc.make_inputs((448, 448, 448), nqs, H, Hkv, D, dtype, 41, dev())
    scale, per = D ** -0.5, 8
    first = [t[:n] for t, n in zip(ks, lens0)], [t[:n] for t, n in zip(vs, lens0)]
    pk, pv, bt = pc.paged_cache(first[0], first[1], 64, per, seed=1, spare=12)
    lens = lens_t(lens0)
    out = pc.nan_out(q)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pc.prefill_c(q, pk, pv, cu, lens, bt, max(nqs), scale, out=out)          # (loads the code objects before the capture)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            pc.prefill_c(q, pk, pv, cu, lens, bt, max(nqs), scale, out=out)
    for step, new_lens in enumerate(((300, 129, 64), (448, 130, 200), (101, 400, 1))):
        cur = [t[:n] for t, n in zip(ks, new_lens)], [t[:n] for t, n in zip(vs, new_lens)]
        nk, nv, nbt = pc.paged_cache(cur[0], cur[1], 64, per, seed=50 + step, spare=pk.shape[0] - sum(-(-n // 64) for n in new_lens))
        assert nk.shape == pk.shape
        pk.copy_(nk), pv.copy_(nv), bt.copy_(nbt), lens.copy_(lens_t(new_lens))
        out[0].fill_(float("nan")), out[1].fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert_same_bits("replay %d" % step, out, pc.prefill_c(q, pk, pv, cu, lens, bt, max(nqs), scale))


def test_operator_lse_merges_max_seqlen_none_and_decode_rows(rows):
    H, Hkv, D, dtype = 4, 2, 128, BF16
    lens, scale = (700, 300, 129, 65, 64, 2, 1, 40), D ** -0.5
    # a batch of decode rows (Nq_s = 1): every row sees all its keys, so the keys split into [0, 192) and [192, ..) by two calls on views and merged
    # are one call; and the call equals flash_attention_decode
    q, cu, ks, vs = base_inputs(H, Hkv, D, dtype, seed=12, lens=lens, nqs=(1,) * len(lens))
    kc, vc = pc.contiguous_cache(ks, vs, NMAX)
    lt = lens_t(lens)
    ref = pc.reference(q, cu, ks, vs, scale)
    o, lse = FlashAttn.flash_attention_prefill(q, kc, vc, cu, lt, max_seqlen_q=1, return_lse=True)
    assert not pc.check_float64("one call", o, lse * pc.LOG2E, ref)
    parts = [FlashAttn.flash_attention_prefill(q, kc[:, :192], vc[:, :192], cu, lt.clamp(max=192), max_seqlen_q=1, return_lse=True),
             FlashAttn.flash_attention_prefill(q, kc[:, 192:], vc[:, 192:], cu, (lt - 192).clamp(min=0), max_seqlen_q=1, return_lse=True)]
    om, lm = FlashAttn.merge_attention([p[0].unsqueeze(0).transpose(1, 2).contiguous() for p in parts], [p[1].unsqueeze(0).contiguous() for p in parts])
    assert not pc.check_float64("merged", om[0].transpose(0, 1), lm[0] * pc.LOG2E, ref)
    od, ld = FlashAttn.flash_attention_decode(q.unsqueeze(1), kc, vc, lt, return_lse=True)
    assert not pc.check_float64("decode", od[:, 0], ld[:, :, 0].transpose(0, 1) * pc.LOG2E, ref)
    # max_seqlen_q=None: the maximum read from cu_seqlens_q (a synchronisation) gives what the stated maximum gives
    q, cu, ks, vs = base_inputs(H, Hkv, D, dtype)
    pk, pv, bt = pc.paged_cache(ks, vs, 128, 7, seed=2)
    a = FlashAttn.flash_attention_prefill(q, pk, pv, cu, lens_t(LENS), bt, max_seqlen_q=max(NQS), window=(100, 0), softcap=30.0, return_lse=True)
    b = FlashAttn.flash_attention_prefill(q, pk, pv, cu, lens_t(LENS), bt, window=100, softcap=30.0, return_lse=True)
    assert pc.bits_equal(a[0], b[0]) and pc.bits_equal(a[1], b[1])
    assert not pc.check_float64("operator", a[0], a[1] * pc.LOG2E, pc.reference(q, cu, ks, vs, scale, 100, 30.0))


def test_a_seeded_random_slice_equals_the_twin_and_float64(rows):
    g = torch.Generator().manual_seed(2024)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))       # noqa: E731
    fails = []
    for draw in range(32):
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
        q, cu, ks, vs = pc.make_inputs(lens, nqs, H, Hkv, D, dtype, 1000 + draw, dev())
        cap = max(max(lens), 1)
        cache = tuple(pc.contiguous_cache(ks, vs, cap + ri(0, 70))) + (None,) if page == 0 else pc.paged_cache(ks, vs, page, -(-cap // page) + ri(0, 2), seed=draw)
        softcap, slopes = (float(ri(5, 50)), slopes_bh(B, H) if ri(0, 1) else slopes_bh(1, H)[0]) if smod else (0.0, None)
        scale = D ** -0.5
        tag = "draw %d B%d H%d Hkv%d D%d page %d lens %s nq %s W %d smod %d %s" % (draw, B, H, Hkv, D, page, lens, nqs, W, smod, dtype)
        got, twin = run_both(q, cu, ks, vs, cache, max(max(nqs), 1), scale, W, softcap, slopes)
        if not (pc.bits_equal(got[0], twin[0]) and pc.bits_equal(got[1], twin[1])):
            fails.append(tag + ": differs from the packed twin")
        fails += pc.check_float64(tag, got[0], got[1], pc.reference(q, cu, ks, vs, scale, W, softcap, slopes))
    assert not fails, "\n".join(fails)
    assert LSE_TOL == 1e-3
