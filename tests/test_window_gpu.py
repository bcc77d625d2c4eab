"""Sliding-window (local) attention on the GPU: fa2_fwd_window / fa2_bwd_window and flash_attention(window=..., q_offset=...).

The reference for a window is the repository's oracle given the band as a bias (fa2_oracle.fwd_c / bwd_c with bias = where(band, 0, -inf): the same
contract 0 arithmetic) and dense float64 (fwd_numpy / bwd_numpy with the same bias).  Tolerances are tests/conftest.py's: ATOL / RTOL / LSE_TOL against
the oracle, 2 * FLOOR against float64, GRAD_TOL for gradients."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import ATOL, FLOOR, GRAD_TOL, LSE_TOL, RTOL
from oracle import fa2_oracle as fo
from rocwmma_fattn import FlashAttn, _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    return torch.device("cuda", 0)


def _code(dt):
    return _fa2_lib.FA2_DTYPE_F16 if dt == torch.float16 else _fa2_lib.FA2_DTYPE_BF16


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _s3(t, bnhd=False):
    st = t.stride()
    return _fa2_lib.strides3(st[0], st[2], st[1]) if bnhd else _fa2_lib.strides3(st[0], st[1], st[2])


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _band(Nq, Nkv, left, right, off, causal=False):
    if causal:
        right = 0
    pos = np.arange(Nq)[:, None] + off
    j = np.arange(Nkv)[None, :]
    keep = np.ones((Nq, Nkv), dtype=bool)
    if left >= 0:
        keep &= j >= pos - left
    if right >= 0:
        keep &= j <= pos + right
    return keep


def _bias(*a, **kw):
    return np.where(_band(*a, **kw), 0.0, -np.inf).astype(np.float32)


def _fwd_window(q, k, v, left, right, off, flags=0, bnhd=False, o=None, lse=None):
    """fa2_fwd_window on BHND (or BNHD) tensors; K / V may have fewer heads."""
    lib = _fa2_lib.load()
    h_ax, n_ax = (2, 1) if bnhd else (1, 2)
    B, H, Nq, D = q.shape[0], q.shape[h_ax], q.shape[n_ax], q.shape[3]
    o = torch.full_like(q, float("nan")) if o is None else o
    lse = torch.full((B, H, Nq), float("nan"), dtype=torch.float32, device=q.device) if lse is None else lse
    _fa2_lib.check(lib.fa2_fwd_window(_code(q.dtype), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, k.shape[h_ax], Nq,
                                      k.shape[n_ax], D, _s3(q, bnhd), _s3(k, bnhd), _s3(v, bnhd), _s3(o, bnhd), _fa2_lib.strides2(H * Nq, Nq), D ** -0.5,
                                      flags, left, right, off, _stream()))
    torch.cuda.synchronize()
    return o, lse


def _bwd_window(q, k, v, o, do, lse, left, right, off, flags=0):
    lib = _fa2_lib.load()
    B, H, Nq, D = q.shape
    dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))      # NaN: every element must be written
    delta = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    _fa2_lib.check(lib.fa2_bwd_window(_code(q.dtype), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                                      dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), B, H, Nq, k.shape[2], D, *(_s3(t) for t in (q, k, v, o, do, dq, dk, dv)),
                                      _fa2_lib.strides2(H * Nq, Nq), D ** -0.5, flags, left, right, off, _stream()))
    torch.cuda.synchronize()
    return dq, dk, dv


def _rand(shape, dt, g):
    return torch.randn(shape, generator=g).to(dt)


def _check_forward(o, lse, q, k, v, bias, dt, tag):
    """o, lse (device) against the oracle and float64, both given the band as a bias; dead rows exactly 0 / -inf."""
    code = _code(dt)
    o_ref_bits, lse_ref = fo.fwd_c(_bits(q), _bits(k), _bits(v), code, False, bias=bias)
    o_ref = fo.bits_to_f32(o_ref_bits, code)
    o_true, lse_true = fo.fwd_numpy(q.float().numpy(), k.float().numpy(), v.float().numpy(), False, bias=bias)
    got, got_l = o.float().cpu().numpy(), lse.cpu().numpy()
    dead = ~np.isfinite(np.broadcast_to(bias, (1, 1) + bias.shape[-2:]).max(-1))[0, 0]
    err_o, err_t = np.abs(got - o_ref), np.abs(got - o_true)
    live_l = np.abs(got_l[..., ~dead] - lse_ref[..., ~dead]).max() if (~dead).any() else 0.0
    live_t = np.abs(got_l[..., ~dead] - lse_true[..., ~dead]).max() if (~dead).any() else 0.0
    print("%s: O vs oracle %.3g, vs float64 %.3g; LSE vs oracle %.3g, vs float64 %.3g; dead rows %d" % (tag, err_o.max(), err_t.max(), live_l, live_t, dead.sum()))
    assert np.isfinite(got).all(), tag
    assert np.all(err_o <= ATOL[code] + RTOL[code] * np.abs(o_ref)), (tag, "oracle O", float(err_o.max()))
    assert err_t.max() <= 2 * FLOOR[code], (tag, "float64 O", float(err_t.max()))
    assert live_l <= LSE_TOL and live_t <= LSE_TOL, (tag, "LSE", live_l, live_t)
    if dead.any():
        assert np.all(got[:, :, dead] == 0.0) and np.all(np.isneginf(got_l[:, :, dead])), (tag, "dead rows")
        assert np.all(np.isneginf(lse_ref[:, :, dead])) and np.all(o_ref[:, :, dead] == 0.0)


# (Nq, Nkv, D, left, right, q_offset)
FWD_SHAPES = [
    (1024, 1024, 64, 128, 0, 0), (1000, 1000, 128, 255, 0, 0), (777, 777, 64, 64, 64, 0), (512, 512, 128, 0, 0, 0),
    (129, 1153, 128, 256, 0, 1024),      # chunked prefill
    (1, 2049, 64, 512, 0, 2048),         # decode
    (640, 384, 64, 100, 0, 0),           # 156 dead rows
    (300, 300, 256, -1, 17, 0), (512, 512, 80, 63, -1, 0),
    (320, 320, 40, 96, 96, 0), (320, 320, 192, 96, 96, 0), (320, 320, 512, 96, 96, 0),      # the remaining kernel families
]


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "N%dx%d_D%d_w%d_%d_off%d" % s)
def test_forward_against_oracle_and_float64(shape, dt):
    Nq, Nkv, D, left, right, off = shape
    dev = _dev()
    B, H = (2, 2) if Nq * Nkv <= 600 * 600 else (1, 3)
    g = torch.Generator(device="cpu").manual_seed(Nq + 3 * Nkv + D + left)
    q, k, v = _rand((B, H, Nq, D), dt, g), _rand((B, H, Nkv, D), dt, g), _rand((B, H, Nkv, D), dt, g)
    bias = _bias(Nq, Nkv, left, right, off)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    for rows in (128, 256):
        with _fa2_lib.options(rows=rows):
            pl = _fa2_lib.window_plan(qd, kd, False, left, right, off)
            assert pl.kernel == _fa2_lib.FA2_KERNEL_HIP_WINDOW and pl.contract == 0 and pl.rows == (128 if D > 256 else rows)
            o, lse = _fwd_window(qd, kd, vd, left, right, off)
        _check_forward(o, lse, q, k, v, bias, dt, "rows %d" % rows)
        if (left, right, off) == (0, 0, 0):      # each row sees itself only: O is V's row, exactly
            assert torch.equal(o.cpu(), v)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_forward_bnhd_strides(dt):
    dev = _dev()
    B, H, Nq, Nkv, D, left, right, off = 2, 4, 333, 400, 128, 50, 20, 60
    g = torch.Generator(device="cpu").manual_seed(5)
    q, k, v = _rand((B, Nq, H, D), dt, g), _rand((B, Nkv, H, D), dt, g), _rand((B, Nkv, H, D), dt, g)
    o, lse = _fwd_window(q.to(dev), k.to(dev), v.to(dev), left, right, off, bnhd=True)
    _check_forward(o.transpose(1, 2), lse, *(t.transpose(1, 2).contiguous() for t in (q, k, v)), _bias(Nq, Nkv, left, right, off), dt, "bnhd")


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_equivalences_are_bit_for_bit(D, dt):
    """No window = fa2_fwd_gqa; the causal flag alone at offset 0 = today's causal call; window_right = 0 = the causal flag."""
    dev = _dev()
    lib = _fa2_lib.load()
    B, H, Hkv, N = 1, 4, 2, 1500
    g = torch.Generator(device="cpu").manual_seed(D)
    q, k, v = _rand((B, H, N, D), dt, g).to(dev), _rand((B, Hkv, N, D), dt, g).to(dev), _rand((B, Hkv, N, D), dt, g).to(dev)

    def gqa(causal):
        o, lse = torch.empty_like(q), torch.empty((B, H, N), dtype=torch.float32, device=dev)
        _fa2_lib.check(lib.fa2_fwd_gqa(_code(dt), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, Hkv, N, N, D, _s3(q), _s3(k), _s3(v),
                                       _s3(o), _fa2_lib.strides2(H * N, N), D ** -0.5, int(causal), None, 0, _stream()))
        torch.cuda.synchronize()
        return o, lse

    def same(a, b):
        return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert same(_fwd_window(q, k, v, -1, -1, 0), gqa(False))
    assert same(_fwd_window(q, k, v, N, N - 1, 0), gqa(False))                       # a window that masks nothing
    assert same(_fwd_window(q, k, v, -1, -1, 0, flags=1), gqa(True))
    assert same(_fwd_window(q, k, v, -1, 5, 0, flags=1), gqa(True))                  # the flag means window_right = 0
    assert same(_fwd_window(q, k, v, 200, 0, 0), _fwd_window(q, k, v, 200, -1, 0, flags=1))
    assert same(_fwd_window(q, k, v, 200, 0, 77), _fwd_window(q, k, v, 200, 33, 77, flags=1))
    assert not same(_fwd_window(q, k, v, 200, 0, 0), gqa(True))


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_grouped_kv_is_bit_identical_to_expanded_kv(D, dt):
    dev = _dev()
    B, H, Nq, Nkv, left, right, off = 2, 8, 400, 700, 130, 10, 300
    g = torch.Generator(device="cpu").manual_seed(D + 1)
    q = _rand((B, H, Nq, D), dt, g).to(dev)
    for Hkv in (1, H // 4):
        k, v = _rand((B, Hkv, Nkv, D), dt, g).to(dev), _rand((B, Hkv, Nkv, D), dt, g).to(dev)
        ke, ve = (t.repeat_interleave(H // Hkv, dim=1).contiguous() for t in (k, v))
        a, b = _fwd_window(q, k, v, left, right, off), _fwd_window(q, ke, ve, left, right, off)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), Hkv
        assert torch.isfinite(a[0]).all()


# self-attention shapes of FWD_SHAPES and the dead-row shape: the fused pass (D <= 64), wave pairs (<= 128), separate passes (<= 256), slabs (> 256)
BWD_SHAPES = [s for s in FWD_SHAPES if s[0] == s[1]] + [(640, 384, 64, 100, 0, 0), (640, 384, 128, 100, 0, 0), (400, 300, 256, 60, 5, 0), (333, 200, 512, 40, 0, 20)]


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: "N%dx%d_D%d_w%d_%d_off%d" % s)
def test_backward_against_oracle_and_float64(shape, dt):
    Nq, Nkv, D, left, right, off = shape
    dev = _dev()
    code = _code(dt)
    B, H = (2, 2) if Nq * Nkv <= 600 * 600 else (1, 2)
    g = torch.Generator(device="cpu").manual_seed(Nq + Nkv + D + left + 1)
    q, k, v, do = (_rand((B, H, n, D), dt, g) for n in (Nq, Nkv, Nkv, Nq))
    keep = _band(Nq, Nkv, left, right, off)
    bias = np.where(keep, 0.0, -np.inf).astype(np.float32)
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    o, lse = _fwd_window(qd, kd, vd, left, right, off, flags=_fa2_lib.FA2_FLAG_EXACT_SCALE)
    dq, dk, dv = _bwd_window(qd, kd, vd, o, dod, lse, left, right, off)
    o_bits, lse_ref = fo.fwd_c(_bits(q), _bits(k), _bits(v), code, False, bias=bias)
    want = fo.bwd_c(_bits(q), _bits(k), _bits(v), o_bits, _bits(do), lse_ref, code, False, bias=bias)
    truth = fo.bwd_numpy(q.float().numpy(), k.float().numpy(), v.float().numpy(), do.float().numpy(), False, bias=bias)
    dead_rows, dead_keys = ~keep.any(1), ~keep.any(0)
    for name, got_t, w_bits, t64 in zip(("dq", "dk", "dv"), (dq, dk, dv), want, truth):
        got, w = got_t.float().cpu().numpy(), fo.bits_to_f32(w_bits, code)
        e_o, e_t, ref_t = np.abs(got - w).max(), np.abs(got - t64).max(), np.abs(w - t64).max()
        print("%s: vs oracle %.3g (max |g| %.3g), vs float64 %.3g (oracle's own %.3g)" % (name, e_o, np.abs(w).max(), e_t, ref_t))
        assert np.isfinite(got).all(), name                       # (pre-filled with NaN: every element was written)
        assert e_o <= GRAD_TOL[code] * max(1.0, np.abs(w).max()), (name, "oracle", float(e_o))
        assert e_t <= max(2 * ref_t, GRAD_TOL[code] * max(1.0, np.abs(t64).max())), (name, "float64", float(e_t))
        dead = dead_rows if name == "dq" else dead_keys
        if dead.any():
            assert np.all(got[:, :, dead] == 0.0), (name, "rows / keys nobody sees")
    if shape == (640, 384, 64, 100, 0, 0):
        assert dead_rows.sum() == 156


def _sdpa_f32(q, k, v, keep, g):
    ke, ve = (t.repeat_interleave(g, dim=1) for t in (k, v))
    s = (q.float() @ ke.float().transpose(-1, -2)) * q.shape[-1] ** -0.5
    s = s.masked_fill(~keep, float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.where(keep.any(-1, keepdim=True), p, torch.zeros_like(p))
    return p @ ve.float()


@pytest.mark.parametrize("frontend", ["py", "compiled"])
@pytest.mark.parametrize("Hkv", [4, 1])
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_operator_matches_the_masked_path_and_sdpa(dt, Hkv, frontend, monkeypatch):
    dev = _dev()
    if frontend == "py":
        monkeypatch.setattr(FlashAttn, "_FRONTEND", [None])
    else:
        assert FlashAttn._frontend() is not None and hasattr(FlashAttn._frontend(), "forward_window")
    code = _code(dt)
    B, H, Nq, Nkv, D = 2, 4, 300, 420, 64
    for window, off, causal in (((100, 0), 120, False), (63, 0, False), ((80, None), 120, True), ((None, 0), 0, False)):
        left, right, _ = _fa2_lib.parse_window(window, off)
        keep = torch.from_numpy(_band(Nq, Nkv, left, right, off, causal)).to(dev)
        g = torch.Generator(device="cpu").manual_seed(Nq + Hkv)
        q, k, v, do = (_rand((B, h, n, D), dt, g).to(dev) for h, n in ((H, Nq), (Hkv, Nkv), (Hkv, Nkv), (H, Nq)))
        outs = []
        for use_window in (True, False):
            qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
            o = flash_attention(qq, kk, vv, causal=causal, window=window, q_offset=off) if use_window else flash_attention(qq, kk, vv, mask=keep)
            o.backward(do)
            outs.append((o.detach(), qq.grad, kk.grad, vv.grad))
        qq, kk, vv = (t.clone().float().requires_grad_(True) for t in (q, k, v))
        ref = _sdpa_f32(qq, kk, vv, keep, H // Hkv)
        ref.backward(do.float())
        torch.cuda.synchronize()
        with torch.no_grad():
            o_ng = flash_attention(q, k, v, causal=causal, window=window, q_offset=off)
        assert torch.equal(o_ng, outs[0][0])                       # the forward alone is the same kernel
        tol_o, tol_g = 2 * FLOOR[code], GRAD_TOL[code]
        for name, a, b, r in zip(("o", "dq", "dk", "dv"), outs[0], outs[1], (ref.detach(), qq.grad, kk.grad, vv.grad)):
            tol = tol_o if name == "o" else tol_g * max(1.0, r.abs().max().item())
            assert torch.isfinite(a).all(), name
            assert (a.float() - b.float()).abs().max().item() <= tol, (name, "masked path", window, off, causal)
            assert (a.float() - r).abs().max().item() <= tol, (name, "sdpa", window, off, causal)
    # mask + window = the mask AND the band (the masked path runs)
    m = torch.rand((B, 1, Nq, Nkv), device=dev) > 0.3
    m[..., 0] = True
    keep = torch.from_numpy(_band(Nq, Nkv, 100, 0, 120)).to(dev)
    a = flash_attention(q, k, v, mask=m, window=(100, 0), q_offset=120)
    b = flash_attention(q, k, v, mask=m & keep)
    assert torch.equal(a, b)
    fm = torch.randn((Nq, Nkv), device=dev).to(dt)
    a = flash_attention(q, k, v, mask=fm, window=(100, 0), q_offset=120)
    b = flash_attention(q, k, v, mask=fm.masked_fill(~keep, float("-inf")))
    assert torch.equal(a, b)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_window_edges_mid_tile_read_and_write_nothing_outside(D, dt):
    """Q, K, V, O and the gradients sit between NaN sentinels in one allocation, K and V at its very end; the window's range starts and ends
    mid-tile.  Results meet the oracle (a NaN read from outside would show), the sentinels are intact."""
    dev = _dev()
    B, H, Nq, Nkv, left, right, off, pad = 1, 2, 200, 333, 70, 30, 90, 64
    g = torch.Generator(device="cpu").manual_seed(D)
    q, k, v, do = (_rand((B, H, n, D), dt, g) for n in (Nq, Nkv, Nkv, Nq))
    sizes = [Nq, Nq, Nq, Nkv, Nkv, Nq, Nkv, Nkv]                   # o, dq, q, dk, dv, do, then K and V last
    total = sum(B * H * n * D for n in sizes) + pad * len(sizes)
    buf = torch.full((total,), float("nan"), dtype=dt, device=dev)
    views, at = [], pad
    for n in sizes:
        views.append(buf[at:at + B * H * n * D].view(B, H, n, D))
        at += B * H * n * D + pad
    at -= pad
    assert at == total                                             # V ends with the allocation
    o, dq, qd, dk, dv, dod, kd, vd = views
    qd.copy_(q), kd.copy_(k), vd.copy_(v), dod.copy_(do)
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device=dev)
    _fwd_window(qd, kd, vd, left, right, off, o=o, lse=lse)
    bias = _bias(Nq, Nkv, left, right, off)
    _check_forward(o, lse, q, k, v, bias, dt, "sentinels")
    lib = _fa2_lib.load()
    delta = torch.empty_like(lse)
    _fa2_lib.check(lib.fa2_bwd_window(_code(dt), qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), dod.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                                      dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), B, H, Nq, Nkv, D, *(_s3(t) for t in (qd, kd, vd, o, dod, dq, dk, dv)),
                                      _fa2_lib.strides2(H * Nq, Nq), D ** -0.5, 0, left, right, off, _stream()))
    torch.cuda.synchronize()
    code = _code(dt)
    o_bits, lse_ref = fo.fwd_c(_bits(q), _bits(k), _bits(v), code, False, bias=bias)
    want = fo.bwd_c(_bits(q), _bits(k), _bits(v), o_bits, _bits(do), lse_ref, code, False, bias=bias)
    for name, got_t, w_bits in zip(("dq", "dk", "dv"), (dq, dk, dv), want):
        got, w = got_t.float().cpu().numpy(), fo.bits_to_f32(w_bits, code)
        assert np.isfinite(got).all() and np.abs(got - w).max() <= GRAD_TOL[code] * max(1.0, np.abs(w).max()), name
    at = 0
    for n in sizes:
        assert torch.isnan(buf[at:at + pad]).all(), "sentinel overwritten"
        at += pad + B * H * n * D
    for t, src in ((qd, q), (kd, k), (vd, v), (dod, do)):
        assert torch.equal(t.cpu(), src)
