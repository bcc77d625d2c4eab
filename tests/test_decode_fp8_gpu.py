"""Decode attention on FP8 (e4m3) KV caches on the GPU: fa2_fwd_decode_fp8 and flash_attention_decode(k_descale=, v_descale=).

The batch is tests/test_decode_gpu.py's (nine sequences: a length of 0, lengths below Nq, both sides of the 32- and 64-key tile edges, a long one).
Every cache BYTE at or beyond a sequence's length is 0x7f, an e4m3 NaN; outputs and the workspace are pre-filled with NaN.

Reference under the same contract.  Cache values are clamp(randn / d, +-448) cast to e4m3 (clamped first: torch's cast does not saturate), the
descales d per (sequence, K / V head) powers of two from {2^-5, 2^-6, 2^-7}, so the dequantised cache is unit-scale like the 16-bit tests' data.
Every finite e4m3 value is a f16 and a bf16 value and a power of two commutes with every rounding, so the reference is the repository's oracle,
unchanged: fa2_oracle.fwd_c per sequence on the cache upcast to q's dtype and multiplied by k_descale (exact), its O multiplied by v_descale
(exact).  Bars: conftest's ATOL / RTOL / LSE_TOL against the oracle, 2 * FLOOR against float64 of the dequantised values (fwd_numpy).  Before
anything runs on the GPU, _case checks on the CPU that the oracle's own result on these inputs is within FLOOR of float64.
General (not power-of-two) descales are held to float64 only.  The references of a shape are computed once and shared.
No test feeds an out-of-range length or page id to the GPU."""
import functools

import numpy as np
import pytest
import torch

import decode_calls as dc
import decode_refs as dr
from oracle import fa2_oracle as fo
from rocwmma_fattn.FlashAttn import flash_attention_decode

pytestmark = pytest.mark.gpu

F16, BF16, E4M3 = torch.float16, torch.bfloat16, torch.float8_e4m3fn
LENS = (1, 63, 64, 65, 127, 129, 1000, 0, 2)
NMAX = 1024
SPLITS = (0, 1, 3, 16)
LOG2E = 1.4426950408889634
NAN_BYTE = 0x7F
# (H, Hkv, Nq, D, dtype): one row; 4 rows; 20 rows, a ragged second tile; 48 rows, the four-tile kernel; 64 rows
SHAPES = [(8, 8, 1, 128, F16), (8, 2, 1, 64, BF16), (10, 2, 4, 128, BF16), (16, 1, 3, 64, F16), (16, 1, 4, 128, F16)]
IDS = ["H%d_Hkv%d_Nq%d_D%d_%s" % (s[0], s[1], s[2], s[3], "f16" if s[4] == F16 else "bf16") for s in SHAPES]


def _quant(x, d):
    """x / d as e4m3, clamped into the format's range first (torch's cast does not saturate); d broadcasts against x."""
    return (x / d).clamp(-448.0, 448.0).to(E4M3)


def _poison(cache8):
    """every byte at or beyond a sequence's length: 0x7f"""
    raw = cache8.view(torch.uint8)
    for b, n in enumerate(LENS):
        raw[b, n:] = NAN_BYTE
    return cache8


_seq_inputs = dr.seq_inputs_fp8


@functools.lru_cache(maxsize=None)
def _case(H, Hkv, Nq, D, dt):
    """CPU tensors of one shape and, per sequence, the oracle's and the float64 results.  Computed once; the oracle is checked against float64 here."""
    g = torch.Generator(device="cpu").manual_seed(1000 * H + 100 * Hkv + 10 * Nq + D + 8)
    B = len(LENS)
    q = torch.randn((B, Nq, H, D), generator=g).to(dt)
    kd, vd = (2.0 ** -torch.randint(5, 8, (B, Hkv), generator=g).float() for _ in range(2))
    k8 = _poison(_quant(torch.randn((B, NMAX, Hkv, D), generator=g), kd[:, None, :, None]))
    v8 = _poison(_quant(torch.randn((B, NMAX, Hkv, D), generator=g), vd[:, None, :, None]))
    refs = dr.refs_fp8(q, k8, v8, kd, vd, LENS, dc.code(dt))
    return q, k8, v8, kd, vd, refs


def _check(o, lse2, refs, dt, tag, oracle=True):
    """o [B, Nq, H, D] and the log2 lse [B, H, Nq] (device) against the shared references; dead rows exactly 0 / -inf, every element written."""
    dr.check(o, lse2, refs, LENS, dc.code(dt), tag, oracle=oracle, verbose=True)


_same_lse = dr.same_lse


def _all_codes():
    """[4, 64] bytes: all 256 e4m3 codes, the two NaN codes (0x7f, 0xff) replaced by 0"""
    codes = torch.arange(256, dtype=torch.int16).to(torch.uint8)
    codes[codes == 0x7F] = 0
    codes[codes == 0xFF] = 0
    return codes.reshape(4, 64)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_every_v_code_exactly(dt):
    """B4 Hkv1 H1 D64, one key per sequence whose V row holds 64 of the 256 codes: a single key has weight exactly 1, so o is the V row converted —
    torch's e4m3fn -> q.dtype conversion bit for bit, for every code.  (One code is expected as a different bit pattern than torch's: 0x80, -0.  The
    f32 accumulator starts at +0 and +0 + 1 * (-0) is +0 under round-to-nearest, as in the 16-bit call on a V of -0; the value is the same.)"""
    dev = dc.dev()
    nmax = 64
    v8 = torch.full((4, nmax, 1, 64), NAN_BYTE, dtype=torch.uint8)
    v8[:, 0, 0] = _all_codes()
    k8 = torch.full((4, nmax, 1, 64), NAN_BYTE, dtype=torch.uint8)
    k8[:, 0] = 0x38                                                     # 1.0
    v8, k8 = v8.view(E4M3), k8.view(E4M3)
    q = torch.randn((4, 1, 1, 64), generator=torch.Generator(device="cpu").manual_seed(3)).to(dt)
    lens = torch.ones(4, dtype=torch.int32)
    o = flash_attention_decode(q.to(dev), k8.to(dev), v8.to(dev), lens.to(dev))
    want = v8[:, :1].to(dt)                                             # [4, 1, 1, 64] = o's shape (H = Hkv = 1)
    assert torch.isfinite(want.float()).all()
    want_bits = want.view(torch.int16).clone()
    want_bits[want_bits == -32768] = 0                                  # -0 -> +0 (see above)
    assert int((want.view(torch.int16) == -32768).sum()) == 1
    assert torch.equal(o.cpu().view(torch.int16), want_bits), (o.cpu().view(torch.int16) != want_bits).nonzero()[:8]


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_every_k_code_exactly(dt):
    """The same four rows as K, 64 query heads with q[h] = e_h and scale = 1: the one score of head h is k[h] exactly, so lse[b, h, 0] = float(k[b, 0, 0, h])
    within three f32 roundings (scale * log2e, the product, the operator's ln 2): 3 * 2^-24 = 1.8e-7 < 1e-6 relative."""
    dev = dc.dev()
    nmax = 64
    k8 = torch.full((4, nmax, 1, 64), NAN_BYTE, dtype=torch.uint8)
    k8[:, 0, 0] = _all_codes()
    v8 = torch.full((4, nmax, 1, 64), NAN_BYTE, dtype=torch.uint8)
    v8[:, 0] = 0x38
    v8, k8 = v8.view(E4M3), k8.view(E4M3)
    q = torch.eye(64).to(dt).reshape(1, 1, 64, 64).expand(4, 1, 64, 64).contiguous()
    lens = torch.ones(4, dtype=torch.int32)
    o, lse = flash_attention_decode(q.to(dev), k8.to(dev), v8.to(dev), lens.to(dev), scale=1.0, return_lse=True)
    want = k8[:, 0, 0].double()                                          # [4, 64] = lse[:, :, 0]
    got = lse[:, :, 0].double().cpu()
    assert torch.isfinite(got).all()
    assert bool(((got - want).abs() <= 1e-6 * want.abs() + 1e-30).all()), float((got - want).abs().max())
    assert torch.equal(o.float().cpu(), torch.ones(4, 1, 64, 64))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_lengths_shapes_and_splits(shape):
    dev = dc.dev()
    H, Hkv, Nq, D, dt = shape
    q, k8, v8, kd, vd, refs = _case(*shape)
    qd, kk, vv, kdd, vdd = (t.to(dev) for t in (q, k8, v8, kd, vd))
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    lse1 = None
    for ns in SPLITS:
        o, lse = dc.decode_c("fp8", qd, kk, vv, lens, ns, kd=kdd, vd=vdd)
        _check(o, lse, refs, dt, (shape[:4], "splits", ns))
        if ns == 1:
            lse1 = lse
        elif ns > 1:
            assert _same_lse(lse, lse1), (shape[:4], ns, "LSE of the split against split 1")
    # the operator: natural-log LSE, the same O bits as the C call with the plan's split
    po, pl = flash_attention_decode(qd, kk, vv, lens, return_lse=True, k_descale=kdd, v_descale=vdd)
    o0, l0 = dc.decode_c("fp8", qd, kk, vv, lens, 0, kd=kdd, vd=vdd)
    assert torch.equal(po.view(torch.int16), o0.view(torch.int16)) and _same_lse(pl * LOG2E, l0)


@pytest.mark.parametrize("which", ["both", "k_only", "v_only", "neither"])
def test_general_descales_against_float64(which):
    """Descales amax / 448 per (sequence, head) — not powers of two, so no same-contract oracle: float64 of the dequantised values only, 2 * FLOOR and
    LSE_TOL.  Where a descale is left out the cache is quantised at scale 1, so the dequantised values stay unit-scale and the absolute bar means
    what it means elsewhere."""
    dev = dc.dev()
    H, Hkv, Nq, D, dt = 8, 2, 3, 64, BF16
    G, B = H // Hkv, len(LENS)
    g = torch.Generator(device="cpu").manual_seed(41)
    q = torch.randn((B, Nq, H, D), generator=g).to(dt)
    xk, xv = (torch.randn((B, NMAX, Hkv, D), generator=g) for _ in range(2))

    def descale(x):
        d = torch.ones(B, Hkv)
        for b, n in enumerate(LENS):
            if n:
                d[b] = x[b, :n].abs().amax(dim=(0, 2)) / 448.0
        return d

    kd = descale(xk) if which in ("both", "k_only") else None
    vd = descale(xv) if which in ("both", "v_only") else None
    one = torch.ones(B, 1, Hkv, 1)
    k8 = _poison(_quant(xk, one if kd is None else kd[:, None, :, None]))
    v8 = _poison(_quant(xv, one if vd is None else vd[:, None, :, None]))
    refs = []
    for b, n in enumerate(LENS):
        if n == 0:
            refs.append(None)
            continue
        qs, ks, _, vs, keep, bias = _seq_inputs(q, k8, v8, kd, vd, b, n, Nq, G)
        o_true, lse_true = fo.fwd_numpy(qs.float().numpy(), ks.numpy(), vs.numpy(), False, bias=bias)
        refs.append((None, None, o_true, lse_true, ~keep.any(1)))
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    for ns in (0, 3):
        o, lse = flash_attention_decode(q.to(dev), k8.to(dev), v8.to(dev), lens, return_lse=True, num_splits=ns,
                                        k_descale=None if kd is None else kd.to(dev), v_descale=None if vd is None else vd.to(dev))
        _check(o, lse * LOG2E, refs, dt, (which, ns), oracle=False)


@pytest.mark.parametrize("page", [64, 128])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=[IDS[1], IDS[2]])
def test_paged_is_bit_identical_to_contiguous(shape, page):
    dev = dc.dev()
    q, k8, v8, kd, vd, refs = _case(*shape)
    pk, pv, bt = dc.paged(k8, v8, LENS, page, torch.Generator(device="cpu").manual_seed(page))
    qd, lens = q.to(dev), torch.tensor(LENS, dtype=torch.int32, device=dev)
    kk, vv, pkd, pvd, btd, kdd, vdd = (t.to(dev) for t in (k8, v8, pk, pv, bt, kd, vd))
    for ns in SPLITS[1:]:
        o, lse = dc.decode_c("fp8", qd, kk, vv, lens, ns, kd=kdd, vd=vdd)
        po, plse = dc.decode_c("fp8", qd, pkd, pvd, lens, ns, kd=kdd, vd=vdd, block_table=btd)
        assert torch.equal(po.view(torch.int16), o.view(torch.int16)) and torch.equal(plse, lse), (shape[:4], page, ns)
    po, plse = dc.decode_c("fp8", qd, pkd, pvd, lens, 0, kd=kdd, vd=vdd, block_table=btd)
    _check(po, plse, refs, shape[4], (shape[:4], "paged", page))
    oo = flash_attention_decode(qd, pkd, pvd, lens, block_table=btd, k_descale=kdd, v_descale=vdd)
    assert torch.equal(oo.view(torch.int16), po.view(torch.int16))


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]], ids=[IDS[1], IDS[4]])
def test_strided_views_are_bit_identical(shape):
    dev = dc.dev()
    H, Hkv, Nq, D, dt = shape
    q, k8, v8, kd, vd, _ = _case(*shape)
    B = q.shape[0]
    qd, kk, vv = q.to(dev), k8.to(dev), v8.to(dev)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    qw = torch.full((B, Nq, H + 2, D), float("nan"), dtype=dt, device=dev)
    qw[:, :, :H] = qd
    kw = torch.full((B, NMAX + 48, Hkv + 1, D), NAN_BYTE, dtype=torch.uint8, device=dev)       # a padded Nmax stride and a padded head stride
    kw[:, :NMAX, :Hkv] = kk.view(torch.uint8)
    kview = kw.view(E4M3)[:, :NMAX, :Hkv]
    dw = torch.full((B, 2 * Hkv + 1), float("nan"), device=dev)                                # strided descales: every other element of a wider row
    dk, dv = dw[:, 0:2 * Hkv:2], torch.full((B, 2 * Hkv + 1), float("nan"), device=dev)[:, 0:2 * Hkv:2]
    dk.copy_(kd)
    dv.copy_(vd)
    assert not kview.is_contiguous() and not dk.is_contiguous() and dk.stride() == dv.stride()
    for ns in (1, 3):
        o, lse = dc.decode_c("fp8", qd, kk, vv, lens, ns, kd=kd.to(dev), vd=vd.to(dev))
        ow = torch.full((B, Nq, H + 2, D), float("nan"), dtype=dt, device=dev)
        so, slse = dc.decode_c("fp8", qw[:, :, :H], kview, vv, lens, ns, kd=dk, vd=dv, o=ow[:, :, :H])
        assert torch.equal(so.view(torch.int16), o.view(torch.int16)) and torch.equal(slse, lse), (shape[:4], ns)
        assert torch.isnan(ow[:, :, H:]).all(), "the call wrote outside its view of o"
        po, pl = flash_attention_decode(qw[:, :, :H], kview, vv, lens, return_lse=True, num_splits=ns, k_descale=dk, v_descale=dv)
        assert torch.equal(po.view(torch.int16), o.view(torch.int16)), (shape[:4], ns, "flash_attention_decode")
        assert _same_lse(pl * LOG2E, lse)


@pytest.mark.parametrize("ns", [0, 3])
def test_graph_replay_follows_lengths_and_descales_changed_in_place(ns):
    """The host reads neither cache_seqlens nor the descales: one captured call, replayed after all three were overwritten in place, gives the eager
    result for the contents at that time (a fully valid cache here, so that every permutation of the lengths is a legal call)."""
    dev = dc.dev()
    H, Hkv, Nq, D, dt = 8, 2, 3, 128, F16
    B = len(LENS)
    g = torch.Generator(device="cpu").manual_seed(78)
    q = torch.randn((B, Nq, H, D), generator=g).to(dt).to(dev)
    k8, v8 = (_quant(torch.randn((B, NMAX, Hkv, D), generator=g), 2.0 ** -5).to(dev) for _ in range(2))
    sets = []
    for i in range(2):
        lens_i = torch.tensor(LENS[3 * i:] + LENS[:3 * i], dtype=torch.int32, device=dev)
        kd_i, vd_i = ((2.0 ** -5 * (1.0 + torch.rand((B, Hkv), generator=g))).to(dev) for _ in range(2))
        sets.append((lens_i, kd_i, vd_i))
    want = [tuple(t.clone() for t in flash_attention_decode(q, k8, v8, s[0], return_lse=True, num_splits=ns, k_descale=s[1], v_descale=s[2])) for s in sets]
    assert not torch.equal(want[0][0], want[1][0])
    lens, kd, vd = (t.clone() for t in sets[0])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flash_attention_decode(q, k8, v8, lens, return_lse=True, num_splits=ns, k_descale=kd, v_descale=vd)           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            go, gl = flash_attention_decode(q, k8, v8, lens, return_lse=True, num_splits=ns, k_descale=kd, v_descale=vd)
    torch.cuda.current_stream().wait_stream(side)
    for i in (0, 1, 0):
        lens.copy_(sets[i][0])
        kd.copy_(sets[i][1])
        vd.copy_(sets[i][2])
        go.zero_()
        gl.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(go.view(torch.int16), want[i][0].view(torch.int16)) and torch.equal(gl, want[i][1])
