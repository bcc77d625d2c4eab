"""Decode attention with a sliding window, soft-capping and ALiBi slopes on the GPU: fa2_fwd_decode_window and flash_attention_decode(window=, softcap=,
alibi_slopes=).

The layout is tests/test_decode_gpu.py's: nine sequences of lengths (1, 63, 64, 65, 127, 129, 1000, 0, 2) in a cache of 1 024 slots, NaN in K and in V at
or beyond every length AND below every sequence's lowest visible key, outputs and workspace pre-filled with NaN.  The references are dense float64 of the
contract per sequence and a same-contract emulation (tests/decode_window_refs.py), computed once per (shape, case) and shared; the bars are the
project's rule (tools/fuzz_features.py: error_and_bar).  That every parity case differs from the plain call by at least 5 bars is asserted on the CPU
(tests/test_decode_window.py).  No test feeds an out-of-range length or page id to the GPU."""
import pytest
import torch

import decode_calls as dc
import decode_refs as dr
import decode_window_refs as wr
from rocwmma_fattn.FlashAttn import flash_attention_decode, kvcache_append

pytestmark = pytest.mark.gpu

F16, BF16 = wr.F16, wr.BF16
LENS, NMAX, SPLITS = wr.LENS, wr.NMAX, wr.SPLITS
LOG2E = 1.4426950408889634
E4M3 = torch.float8_e4m3fn


def _device_case(shape, name, dev):
    """q, the dirty caches, the lengths and the slopes of (shape, case) on the device"""
    H, Hkv, Nq, D, dt = shape
    wl, cap, kind = wr.CASES[name]
    q, k, v = wr.inputs(*shape)
    sl = wr.slopes_of(kind, len(LENS), H)
    return (q.to(dev), wr.dirty(k, Nq, wl).to(dev), wr.dirty(v, Nq, wl).to(dev), torch.tensor(LENS, dtype=torch.int32, device=dev),
            None if sl is None else sl.to(dev), wl, cap)


@pytest.mark.parametrize("name", list(wr.CASES))
@pytest.mark.parametrize("shape", wr.SHAPES, ids=wr.IDS)
def test_parity_with_float64(shape, name):
    dev = dc.dev()
    refs = wr.case_refs(shape, name)
    q, k, v, lens, sl, wl, cap = _device_case(shape, name, dev)
    lses = {}
    for ns in SPLITS:
        o, lses[ns] = dc.decode_c("window", q, k, v, lens, ns, wl, cap, sl)
        wr.check(o, lses[ns], refs, (wr.IDS[wr.SHAPES.index(shape)], name, "splits", ns))
    for ns in SPLITS:                                # the plan's own split (0) included
        assert dr.same_lse(lses[ns], lses[1]), (shape[:4], name, ns, "LSE of the split against split 1")


@pytest.mark.parametrize("shape", wr.EDGE_SHAPES, ids=wr.EDGE_IDS)
def test_windows_between_row_0s_reach_and_the_last_rows(shape):
    """window_left in {NMAX - Nq, NMAX - 2} on full sequences: such a window masks nothing for row 0, but row i still drops the keys below
    i + NMAX - Nq - window_left.  Alone and with all-zero slopes beside it (idle, so that the float64 reference and its margin are the window's
    alone): neither the plain kernels nor a windowless launch of the banded ones may serve these calls."""
    dev = dc.dev()
    H, Hkv, Nq, D, dt = shape
    q, k, v = wr.edge_inputs(*shape)
    lens = torch.tensor(wr.EDGE_LENS, dtype=torch.int32, device=dev)
    zero = torch.zeros(H, dtype=torch.float32, device=dev)
    for name, wl in wr.edge_windows(Nq):
        refs = wr.edge_refs(shape, wl)
        args = (q.to(dev), wr.dirty(k, Nq, wl, lens=wr.EDGE_LENS).to(dev), wr.dirty(v, Nq, wl, lens=wr.EDGE_LENS).to(dev), lens)
        outs = {}
        for ns in SPLITS:
            outs[ns] = dc.decode_c("window", *args, ns, wl)
            wr.check(*outs[ns], refs, (wr.EDGE_IDS[wr.EDGE_SHAPES.index(shape)], name, "splits", ns))
        for ns in SPLITS:
            assert dr.same_lse(outs[ns][1], outs[1][1]), (shape[:4], name, ns, "LSE of the split against split 1")
        o, lse = dc.decode_c("window", *args, 3, wl, 0.0, zero)               # zero slopes: the launch that slopes force must carry the window too
        wr.check(o, lse, refs, (shape[:4], name, "zero slopes"))
        po, pl = flash_attention_decode(*args, window=wl, return_lse=True, num_splits=3)
        assert torch.equal(po.view(torch.int16), outs[3][0].view(torch.int16)) and dr.same_lse(pl * LOG2E, outs[3][1]), (shape[:4], name, "operator")


@pytest.mark.parametrize("shape", [wr.SHAPES[0], wr.SHAPES[2], wr.SHAPES[4]], ids=[wr.IDS[0], wr.IDS[2], wr.IDS[4]])
def test_no_keywords_and_a_window_wider_than_the_cache_are_the_plain_call_bit_for_bit(shape):
    dev = dc.dev()
    H, Hkv, Nq, D, dt = shape
    q, k, v = wr.inputs(*shape)
    qd, kd_, vd_ = q.to(dev), wr.dirty(k, Nq, -1).to(dev), wr.dirty(v, Nq, -1).to(dev)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    for ns in (1, 3):
        want = dc.decode_c("plain", qd, kd_, vd_, lens, ns)
        assert torch.isfinite(want[0].float()).all()
        assert dc.same_bits(dc.decode_c("window", qd, kd_, vd_, lens, ns), want), (shape[:4], ns, "window_left -1, softcap 0, null slopes")
        assert dc.same_bits(dc.decode_c("window", qd, kd_, vd_, lens, ns, window_left=5000), want), (shape[:4], ns, "window_left 5000")
    # the same pair on an e4m3 cache with power-of-two descales
    k8, v8, kds, vds = _fp8_cache(k, v, Hkv, Nq, -1, dev)
    for ns in (1, 3):
        want = dc.decode_c("fp8", qd, k8, v8, lens, ns, kd=kds, vd=vds)
        assert torch.isfinite(want[0].float()).all()
        assert dc.same_bits(dc.decode_c("window", qd, k8, v8, lens, ns, kd=kds, vd=vds), want), (shape[:4], ns, "e4m3, no keywords")
        assert dc.same_bits(dc.decode_c("window", qd, k8, v8, lens, ns, window_left=5000, kd=kds, vd=vds), want), (shape[:4], ns, "e4m3, window_left 5000")


def _fp8_parts(k, v, Hkv):
    """CPU: e4m3 caches of k / 4 and v / 2 with descales 4 and 2 scaled per (sequence, head) by further powers of two, and the float values they mean."""
    B = k.shape[0]
    e = (torch.arange(B * Hkv).reshape(B, Hkv) % 3).float()
    kds, vds = 4.0 * 2.0 ** e, 2.0 * 2.0 ** -e
    k8 = (k.float() / kds[:, None, :, None]).to(E4M3)
    v8 = (v.float() / vds[:, None, :, None]).to(E4M3)
    return k8, v8, kds, vds, k8.float() * kds[:, None, :, None], v8.float() * vds[:, None, :, None]


def _dirty8(t8, Nq, wl):
    """0x7f (an e4m3 NaN code) in every byte at or beyond a length and below the lowest visible key"""
    raw = t8.view(torch.uint8).clone()
    return wr.dirty(raw, Nq, wl, fill=0x7F).view(E4M3)


def _fp8_cache(k, v, Hkv, Nq, wl, dev):
    k8, v8, kds, vds, _, _ = _fp8_parts(k, v, Hkv)
    return _dirty8(k8, Nq, wl).to(dev), _dirty8(v8, Nq, wl).to(dev), kds.to(dev), vds.to(dev)


def _paged(k, v, page, Nq, wl, g):
    """The clean [B, NMAX, Hkv, D] caches, made dirty, in pages (decode_calls.paged).  A page that holds only keys below its sequence's window is one the
    server freed: it stays NaN and the table names the NaN page."""
    return dc.paged(wr.dirty(k, Nq, wl), wr.dirty(v, Nq, wl), LENS, page, g, keep=lambda b, j: (j + 1) * page > wr.window_lo(LENS[b], Nq, wl))


@pytest.mark.parametrize("page", [64, 128])
@pytest.mark.parametrize("shape", [wr.SHAPES[0], wr.SHAPES[3]], ids=[wr.IDS[0], wr.IDS[3]])
def test_paged_with_freed_pages_is_bit_identical_to_contiguous(shape, page):
    dev = dc.dev()
    name = "all"
    q, k, v, lens, sl, wl, cap = _device_case(shape, name, dev)
    cq, ck, cv = wr.inputs(*shape)
    pk, pv, bt = _paged(ck, cv, page, shape[2], wl, torch.Generator(device="cpu").manual_seed(page))
    pk, pv, bt = pk.to(dev), pv.to(dev), bt.to(dev)
    for ns in (1, 3, 16):
        want = dc.decode_c("window", q, k, v, lens, ns, wl, cap, sl)
        got = dc.decode_c("window", q, pk, pv, lens, ns, wl, cap, sl, block_table=bt)
        assert dc.same_bits(got, want), (shape[:4], page, ns)
    o, lse = dc.decode_c("window", q, pk, pv, lens, 0, wl, cap, sl, block_table=bt)       # the plan's own split of the paged call
    wr.check(o, lse, wr.case_refs(shape, name), (shape[:4], "paged", page))
    # window only, where nothing but the select keeps the freed pages out
    q, k, v, lens, _, wl, _ = _device_case(shape, "window31", dev)
    pk, pv, bt = (t.to(dev) for t in _paged(ck, cv, page, shape[2], wl, torch.Generator(device="cpu").manual_seed(page + 1)))
    for ns in (1, 3):
        assert dc.same_bits(dc.decode_c("window", q, pk, pv, lens, ns, wl, block_table=bt), dc.decode_c("window", q, k, v, lens, ns, wl)), (shape[:4], page, ns, "window31")


@pytest.mark.parametrize("shape", [wr.SHAPES[0], wr.SHAPES[1], wr.SHAPES[3]], ids=[wr.IDS[0], wr.IDS[1], wr.IDS[3]])
def test_fp8_cache_against_float64_of_the_descaled_cache(shape):
    """window=100, softcap=8.0 and [B, H] slopes on an e4m3 cache with power-of-two descales: the cap acts on the DESCALED score."""
    dev = dc.dev()
    H, Hkv, Nq, D, dt = shape
    q, k, v = wr.inputs(*shape)
    wl, cap, sl = 100, 8.0, wr.slopes_of("BH", len(LENS), H)
    k8, v8, kds, vds, kf, vf = _fp8_parts(k, v, Hkv)
    assert torch.equal(kf.to(dt).float(), kf) and torch.equal(vf.to(dt).float(), vf), "the upcast, descaled cache is exact in q's dtype"
    refs = wr.seq_refs(q.float(), kf, vf, LENS, D ** -0.5, wl, cap, sl, dt)
    mo, ml = wr.margins(refs)
    assert mo >= 5 and ml >= 5, (mo, ml)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    args = (q.to(dev), _dirty8(k8, Nq, wl).to(dev), _dirty8(v8, Nq, wl).to(dev), lens)
    for ns in SPLITS:
        o, lse = dc.decode_c("window", *args, ns, wl, cap, sl.to(dev), kd=kds.to(dev), vd=vds.to(dev))
        wr.check(o, lse, refs, (shape[:4], "fp8", ns))
    # the operator reaches the same bits
    po, pl = flash_attention_decode(*args, window=wl, softcap=cap, alibi_slopes=sl.to(dev), k_descale=kds.to(dev), v_descale=vds.to(dev), return_lse=True,
                                    num_splits=3)
    o, lse = dc.decode_c("window", *args, 3, wl, cap, sl.to(dev), kd=kds.to(dev), vd=vds.to(dev))
    assert torch.equal(po.view(torch.int16), o.view(torch.int16)) and dr.same_lse(pl * LOG2E, lse)


@pytest.mark.parametrize("shape", [wr.SHAPES[0], wr.SHAPES[2]], ids=[wr.IDS[0], wr.IDS[2]])
def test_operator_gives_the_c_calls_bits(shape):
    dev = dc.dev()
    H, Hkv, Nq, D, dt = shape
    B = len(LENS)
    for name, window in (("window31", 31), ("window100", (100, 0)), ("softcap30", None), ("slopes_H", None), ("all", (100, None))):
        q, k, v, lens, sl, wl, cap = _device_case(shape, name, dev)
        qw = torch.full((B, Nq, H + 2, D), float("nan"), dtype=dt, device=dev)
        qw[:, :, :H] = q
        kw = torch.full((B, NMAX + 40, Hkv, D), float("nan"), dtype=dt, device=dev)       # a padded Nmax stride
        kw[:, :NMAX] = k
        assert not qw[:, :, :H].is_contiguous() and not kw[:, :NMAX].is_contiguous()
        for ns in (1, 3):
            o, lse = dc.decode_c("window", q, k, v, lens, ns, wl, cap, sl)
            po = flash_attention_decode(q, k, v, lens, num_splits=ns, window=window, softcap=cap, alibi_slopes=sl)
            assert torch.equal(po.view(torch.int16), o.view(torch.int16)), (shape[:4], name, ns)
            so, sl2 = flash_attention_decode(qw[:, :, :H], kw[:, :NMAX], v, lens, num_splits=ns, window=window, softcap=cap, alibi_slopes=sl, return_lse=True)
            assert torch.equal(so.view(torch.int16), o.view(torch.int16)), (shape[:4], name, ns, "strided q and cache view")
            assert sl2.shape == (B, H, Nq) and dr.same_lse(sl2 * LOG2E, lse), (shape[:4], name, ns, "return_lse: natural log")


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_fused_append_under_a_window_is_append_then_the_windowed_call(dt):
    dev = dc.dev()
    B, H, Hkv, Nq, D, N, wl = 4, 8, 2, 3, 128, 256, 40
    g = torch.Generator(device="cpu").manual_seed(23)
    q = (2 * torch.randn((B, Nq, H, D), generator=g)).to(dt).to(dev)
    k0, v0 = ((2 * torch.randn((B, N, Hkv, D), generator=g)).to(dt).to(dev) for _ in range(2))
    kn, vn = ((2 * torch.randn((B, Nq, Hkv, D), generator=g)).to(dt).to(dev) for _ in range(2))
    ang = torch.rand((N, D // 2), generator=g) * 6.28
    cos, sin = ang.cos().to(dev), ang.sin().to(dev)
    lens = torch.tensor([3, 77, 200, 256], dtype=torch.int32, device=dev)
    sl = wr.alibi_slopes(H).to(dev)
    ka, va = k0.clone(), v0.clone()
    q_rot = kvcache_append(ka, va, kn, vn, lens, rotary_cos=cos, rotary_sin=sin, q=q)
    want = flash_attention_decode(q_rot, ka, va, lens, window=wl, softcap=30.0, alibi_slopes=sl, return_lse=True, num_splits=2)
    plain = flash_attention_decode(q_rot, ka, va, lens, num_splits=2)
    assert not torch.equal(plain, want[0])
    kb, vb = k0.clone(), v0.clone()
    got = flash_attention_decode(q, kb, vb, lens, k=kn, v=vn, rotary_cos=cos, rotary_sin=sin, window=wl, softcap=30.0, alibi_slopes=sl, return_lse=True,
                                 num_splits=2)
    assert torch.equal(kb.view(torch.int16), ka.view(torch.int16)) and torch.equal(vb.view(torch.int16), va.view(torch.int16)), "the append is unaffected"
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("ns", [0, 3])
def test_graph_replay_follows_lengths_and_slopes_changed_in_place(ns):
    """The host reads neither cache_seqlens nor the slopes: one captured call with a window and slopes, replayed after both were overwritten in place,
    gives the eager result for the contents at that time (a fully valid cache, so that every permutation of the lengths is a legal call)."""
    dev = dc.dev()
    H, Hkv, Nq, D, dt, wl = 8, 2, 3, 128, F16, 100
    g = torch.Generator(device="cpu").manual_seed(78)
    B = len(LENS)
    q = (2 * torch.randn((B, Nq, H, D), generator=g)).to(dt).to(dev)
    k, v = ((2 * torch.randn((B, NMAX, Hkv, D), generator=g)).to(dt).to(dev) for _ in range(2))
    lens_a = torch.tensor(LENS, dtype=torch.int32, device=dev)
    lens_b = torch.tensor(LENS[3:] + LENS[:3], dtype=torch.int32, device=dev)
    sl_a, sl_b = wr.slopes_of("BH", B, H).to(dev), (wr.slopes_of("BH", B, H) * 3.0).flip(0).contiguous().to(dev)
    states = ((lens_a, sl_a), (lens_b, sl_b), (lens_a, sl_b), (lens_a, sl_a))
    want = [tuple(t.clone() for t in flash_attention_decode(q, k, v, x, window=wl, alibi_slopes=s, return_lse=True, num_splits=ns)) for x, s in states]
    assert not torch.equal(want[0][0], want[1][0]) and not torch.equal(want[0][0], want[2][0])
    lens, sl = lens_a.clone(), sl_a.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flash_attention_decode(q, k, v, lens, window=wl, alibi_slopes=sl, return_lse=True, num_splits=ns)           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            go, gl = flash_attention_decode(q, k, v, lens, window=wl, alibi_slopes=sl, return_lse=True, num_splits=ns)
    torch.cuda.current_stream().wait_stream(side)
    for (x, s), (wo, wlse) in zip(states, want):
        lens.copy_(x)
        sl.copy_(s)
        go.zero_()
        gl.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(go.view(torch.int16), wo.view(torch.int16)) and torch.equal(gl, wlse)
