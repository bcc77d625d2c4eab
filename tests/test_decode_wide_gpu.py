"""Decode attention at head dim 256 on the GPU: fa2_fwd_decode_wide and flash_attention_decode on D = 256 tensors.  tests/test_decode_gpu.py's layout (nine
lengths in a 1 024-slot cache; NaN at or beyond every length, below every window, in spare pages, in outputs and workspace) under the existing references and
bars (tests/decode_refs.py, tests/decode_window_refs.py), at 1, 2, 16, 17, 32, 33 and 64 rows per K / V head: one row tile, two, two row blocks, and the ragged
last tile of each.  No test feeds an out-of-range length or page id to the GPU."""
import functools

import pytest
import torch

import decode_calls as dc
import decode_refs as dr
import decode_window_refs as wr
from rocwmma_fattn.FlashAttn import flash_attention_decode, kvcache_append

pytestmark = pytest.mark.gpu

F16, BF16, E4M3 = torch.float16, torch.bfloat16, torch.float8_e4m3fn
LENS, NMAX, SPLITS, D = wr.LENS, wr.NMAX, wr.SPLITS, 256
LOG2E = 1.4426950408889634
ROWS = {1: (2, 2, 1), 2: (4, 2, 1), 16: (8, 2, 4), 17: (17, 1, 1), 32: (8, 1, 4), 33: (11, 1, 3), 64: (16, 1, 4)}      # rows -> (H, Hkv, Nq)


@functools.lru_cache(maxsize=None)
def _case(rows, dt):
    H, Hkv, Nq = ROWS[rows]
    g = torch.Generator(device="cpu").manual_seed(2560 + rows)
    q = torch.randn((len(LENS), Nq, H, D), generator=g).to(dt)
    k, v = (wr.dirty(torch.randn((len(LENS), NMAX, Hkv, D), generator=g).to(dt), Nq, -1) for _ in range(2))
    return q, k, v, dr.refs16(q, k, v, LENS, dc.code(dt))


def _lens(dev):
    return torch.tensor(LENS, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("rows", list(ROWS))
def test_lengths_rows_and_splits(rows, dt):
    dev = dc.dev()
    q, k, v, refs = _case(rows, dt)
    qd, kd, vd, lens = q.to(dev), k.to(dev), v.to(dev), _lens(dev)
    lses = {}
    for ns in SPLITS:
        o, lses[ns] = dc.decode_c("wide", qd, kd, vd, lens, ns)
        dr.check(o, lses[ns], refs, LENS, dc.code(dt), (rows, "splits", ns))
        assert dr.same_lse(lses[ns], lses[SPLITS[0]]), (rows, ns, "LSE of the split against the plan's")


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("rows", [2, 17, 64])
def test_e4m3_cache_with_power_of_two_descales(rows, dt):
    dev = dc.dev()
    H, Hkv, Nq = ROWS[rows]
    g = torch.Generator(device="cpu").manual_seed(2568 + rows)
    B = len(LENS)
    q = torch.randn((B, Nq, H, D), generator=g).to(dt)
    kds, vds = (2.0 ** -torch.randint(5, 8, (B, Hkv), generator=g).float() for _ in range(2))
    # x / descale as e4m3 (clamped first: torch's cast does not saturate), 0x7f — an e4m3 NaN — in every byte at or beyond a length.  V is N(0, 1) / 2:
    # refs_fp8 holds the oracle to float64 within FLOOR — half an f16 ulp of a value in [2, 4) already — and the largest of 17 * 256 N(0, 1) draws is past 2.
    k8, v8 = (wr.dirty((s * torch.randn((B, NMAX, Hkv, D), generator=g) / d[:, None, :, None]).clamp(-448.0, 448.0).to(E4M3).view(torch.uint8), Nq, -1,
                       fill=dc.NAN_BYTE).view(E4M3) for s, d in ((1.0, kds), (0.5, vds)))
    refs = dr.refs_fp8(q, k8, v8, kds, vds, LENS, dc.code(dt))
    for ns in (0, 3):
        o, lse = dc.decode_c("wide", q.to(dev), k8.to(dev), v8.to(dev), _lens(dev), ns, kd=kds.to(dev), vd=vds.to(dev))
        dr.check(o, lse, refs, LENS, dc.code(dt), (rows, "e4m3", ns))


@pytest.mark.parametrize("name,wl,cap,kind", [("window0", 0, 0.0, None), ("window31", 31, 0.0, None), ("all", 100, 30.0, "BH")])
@pytest.mark.parametrize("rows,dt", [(2, BF16), (33, F16)])
def test_window_softcap_and_slopes_against_float64(rows, dt, name, wl, cap, kind):
    dev = dc.dev()
    H, Hkv, Nq = ROWS[rows]
    q, k, v = wr.inputs(H, Hkv, Nq, D, dt)
    sl = wr.slopes_of(kind, len(LENS), H)
    refs = wr.seq_refs(q.float(), k.float(), v.float(), LENS, D ** -0.5, wl, cap, sl, dt)
    args = (q.to(dev), wr.dirty(k, Nq, wl).to(dev), wr.dirty(v, Nq, wl).to(dev), _lens(dev))      # NaN below the window too
    for ns in SPLITS:
        o, lse = dc.decode_c("wide", *args, ns, wl, cap, None if sl is None else sl.to(dev))
        wr.check(o, lse, refs, (rows, name, "splits", ns))


@pytest.mark.parametrize("rows,dt", [(2, F16), (33, BF16)])
def test_addressing_bit_equalities(rows, dt):
    """paged (64, 128) against contiguous at the same split; a strided q / cache view against the compact tensors; the operator against the C entry."""
    dev = dc.dev()
    H, Hkv, Nq = ROWS[rows]
    q, k, v, _ = _case(rows, dt)
    B = len(LENS)
    qd, kd, vd, lens = q.to(dev), k.to(dev), v.to(dev), _lens(dev)
    qw = torch.full((B, Nq, H + 2, D), float("nan"), dtype=dt, device=dev)
    qw[:, :, :H] = qd
    kw = torch.full((B, NMAX + 40, Hkv, D), float("nan"), dtype=dt, device=dev)       # a padded Nmax stride
    kw[:, :NMAX] = kd
    pools = {page: [t.to(dev) for t in dc.paged(k, v, LENS, page, torch.Generator(device="cpu").manual_seed(page))] for page in (64, 128)}
    for ns in (1, 3):
        want = dc.decode_c("wide", qd, kd, vd, lens, ns)
        for page, (pk, pv, bt) in pools.items():
            assert dc.same_bits(dc.decode_c("wide", qd, pk, pv, lens, ns, block_table=bt), want), (rows, page, ns)
        ow = torch.full((B, Nq, H + 2, D), float("nan"), dtype=dt, device=dev)
        assert dc.same_bits(dc.decode_c("wide", qw[:, :, :H], kw[:, :NMAX], vd, lens, ns, o=ow[:, :, :H]), want), (rows, ns, "strided views")
        assert torch.isnan(ow[:, :, H:]).all(), "the call wrote outside its view of o"
        po, pl = flash_attention_decode(qw[:, :, :H], kw[:, :NMAX], vd, lens, return_lse=True, num_splits=ns)
        assert torch.equal(po.view(torch.int16), want[0].view(torch.int16)) and dr.same_lse(pl * LOG2E, want[1]), (rows, ns, "flash_attention_decode")


def test_fused_append_is_append_then_decode():
    dev = dc.dev()
    B, H, Hkv, Nq, N, dt = 4, 8, 4, 3, 256, BF16
    g = torch.Generator(device="cpu").manual_seed(29)
    q = torch.randn((B, Nq, H, D), generator=g).to(dt).to(dev)
    k0, v0 = (torch.randn((B, N, Hkv, D), generator=g).to(dt).to(dev) for _ in range(2))
    kn, vn = (torch.randn((B, Nq, Hkv, D), generator=g).to(dt).to(dev) for _ in range(2))
    ang = torch.rand((N, D // 2), generator=g) * 6.28
    cos, sin = ang.cos().to(dev), ang.sin().to(dev)
    lens = torch.tensor([3, 77, 200, 256], dtype=torch.int32, device=dev)
    ka, va = k0.clone(), v0.clone()
    q_rot = kvcache_append(ka, va, kn, vn, lens, rotary_cos=cos, rotary_sin=sin, q=q)
    want = flash_attention_decode(q_rot, ka, va, lens, window=40, return_lse=True, num_splits=2)
    kb, vb = k0.clone(), v0.clone()
    got = flash_attention_decode(q, kb, vb, lens, k=kn, v=vn, rotary_cos=cos, rotary_sin=sin, window=40, return_lse=True, num_splits=2)
    assert torch.equal(kb.view(torch.int16), ka.view(torch.int16)) and torch.equal(vb.view(torch.int16), va.view(torch.int16))
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)) and torch.equal(got[1], want[1])


def test_graph_replay_follows_lengths_and_block_table_changed_in_place():
    """one captured paged call gives the eager result for the contents at replay time (every page valid, so that every state is a legal call)"""
    dev = dc.dev()
    H, Hkv, Nq, dt, page = 8, 2, 3, F16, 64
    g = torch.Generator(device="cpu").manual_seed(79)
    B, per = len(LENS), NMAX // page
    q = torch.randn((B, Nq, H, D), generator=g).to(dt).to(dev)
    pk, pv = (torch.randn((B * per, page, Hkv, D), generator=g).to(dt).to(dev) for _ in range(2))
    bt_a = torch.randperm(B * per, generator=g).to(torch.int32).reshape(B, per).to(dev)
    states = ((_lens(dev), bt_a), (torch.tensor(LENS[3:] + LENS[:3], dtype=torch.int32, device=dev), bt_a.flip(0).contiguous()), (_lens(dev), bt_a))
    want = [tuple(t.clone() for t in flash_attention_decode(q, pk, pv, x, block_table=t_, return_lse=True, num_splits=3)) for x, t_ in states]
    assert not torch.equal(want[0][0], want[1][0])
    lens, bt = states[0][0].clone(), bt_a.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flash_attention_decode(q, pk, pv, lens, block_table=bt, return_lse=True, num_splits=3)           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            go, gl = flash_attention_decode(q, pk, pv, lens, block_table=bt, return_lse=True, num_splits=3)
    torch.cuda.current_stream().wait_stream(side)
    for (x, t_), (wo, wlse) in zip(states, want):
        lens.copy_(x)
        bt.copy_(t_)
        go.zero_()
        gl.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(go.view(torch.int16), wo.view(torch.int16)) and torch.equal(gl, wlse)
