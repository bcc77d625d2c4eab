"""GPU tests of attention dropout (fa2_fwd_dropout / fa2_bwd_dropout and their packed twins, flash_attention(dropout_p=...)).
The reference is dense float64 attention (tools/fuzz_features.py: ref64), with the keep mask taken from the library's host function (dropout_keep_mask): the oracle is
not involved.  Bars, scaled by magnitude because 1 / (1 - p) enlarges O:
    max|O - O_true| <= max(2 * err_emu, FLOOR[dt] * max(1, max|O_true|)),   gradients likewise with GRAD_TOL[dt],
err_emu = the error against float64 of a same-contract torch emulation (f32 scores and sums, P rounded to the I/O dtype, one final rounding).
The LSE is that of the undropped probabilities: LSE_TOL against float64 and against the same call without dropout."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from conftest import FLOOR, GRAD_TOL, LSE_TOL
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import dropout_keep_mask, flash_attention, flash_attention_varlen, flash_attn_wmma

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
LN2 = math.log(2.0)


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("these tests need a ROCm device")
    return torch.device("cuda")


def _code(dt):
    return 0 if dt == torch.float16 else 1


def _rand(shape, dt, g, mul=1.0):
    return (torch.randn(shape, generator=g) * mul).to(dt)


# the band, float64 truth, the same-contract emulation and the bar rule: one copy, in tools/fuzz_features.py (the randomised sweep uses them too)
_spec = importlib.util.spec_from_file_location("_fuzz_features", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "tools", "fuzz_features.py"))
_ff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ff)
_band, _ref64, _emu = _ff.band, _ff.ref64, _ff.emu


def _check(name, got, true, emu, tol, tag):
    err, err_emu, bar = _ff.error_and_bar(got, true, emu, tol)
    print("%s %s: err %.3g, emulation %.3g, bar %.3g (max |true| %.3g)" % (tag, name, err, err_emu, bar, true.abs().max().item()))
    assert err <= bar, (tag, name, err, bar)


def _dense_case(dt, B, H, Hkv, Nq, Nkv, D, causal, p, seed, window=None, q_offset=0, bnhd=False, gseed=0):
    dev = _dev()
    g = torch.Generator().manual_seed(1000 + gseed)
    q, k, v, do = _rand((B, H, Nq, D), dt, g), _rand((B, Hkv, Nkv, D), dt, g), _rand((B, Hkv, Nkv, D), dt, g), _rand((B, H, Nq, D), dt, g)
    scale = D ** -0.5
    left, right, off = _fa2_lib.parse_window(window if window is not None else (-1, -1), q_offset)
    band = _band(Nq, Nkv, left, right, off, causal)
    keep = dropout_keep_mask(seed, p, B, H, Nq, Nkv)

    def put(t):
        t = t.to(dev)
        return (t.transpose(1, 2).contiguous() if bnhd else t).requires_grad_(True)
    qd, kd, vd = put(q), put(k), put(v)
    o = flash_attention(qd, kd, vd, causal=causal, BNHD_fmt=bnhd, window=window, q_offset=q_offset, dropout_p=p, dropout_seed=seed)
    dod = do.to(dev).transpose(1, 2).contiguous() if bnhd else do.to(dev)
    o.backward(dod)
    unp = (lambda t: t.transpose(1, 2)) if bnhd else (lambda t: t)
    got = [unp(t).detach().cpu() for t in (o, qd.grad, kd.grad, vd.grad)]
    code, grp = _code(dt), H // Hkv
    tag = "%s B%d H%d/%d %dx%d D%d causal=%d p=%g win=%s off=%d bnhd=%d" % (str(dt)[6:], B, H, Hkv, Nq, Nkv, D, causal, p, window, q_offset, bnhd)
    for b in range(B):
        ke, ve = k[b].repeat_interleave(grp, 0), v[b].repeat_interleave(grp, 0)
        true = _ref64(q[b], ke, ve, do[b], keep[b], band, scale, p)
        emu = _emu(q[b], ke, ve, do[b], keep[b], band, scale, p, dt)
        fold = lambda t: t.unflatten(0, (Hkv, grp)).sum(1)      # noqa: E731 - dK / dV of a group
        _check("O", got[0][b], true[0], emu[0], FLOOR[code], tag)
        _check("dQ", got[1][b], true[2], emu[1], GRAD_TOL[code], tag)
        _check("dK", got[2][b], fold(true[3]), fold(emu[2]), GRAD_TOL[code], tag)
        _check("dV", got[3][b], fold(true[4]), fold(emu[3]), GRAD_TOL[code], tag)
        dead = ~band.any(-1)
        if dead.any():
            assert (got[0][b][:, dead] == 0).all() and (got[1][b][:, dead] == 0).all(), (tag, "rows that see no key")
    return tag


# ---- 1. the device's mask, read back from O, equals the host's bit for bit
def _readback_inputs(B, H, Nq, D, dev):
    Nkv = 4 * D
    j = torch.arange(Nkv)
    V = torch.zeros(Nkv, D, dtype=torch.float16)
    V[j, j % D] = (2.0 ** (j // D)).to(torch.float16)
    q = torch.randn(B, H, Nq, D, generator=torch.Generator().manual_seed(3)).to(torch.float16)
    k = torch.zeros(B, H, Nkv, D, dtype=torch.float16)
    v = V.expand(B, H, Nkv, D).contiguous()
    return q.to(dev), k.to(dev), v.to(dev), Nkv


def _decode(o, Nkv, D):
    """O [..., Nq, D] of the readback inputs at p = 0.5 -> keep [..., Nq, Nkv]: O[i, c] = (2 / Nkv) * sum_g keep[i, g * D + c] * 2^g, every step exact."""
    n = o.double() * (Nkv / 2.0)
    assert (n == n.round()).all() and (n >= 0).all() and (n <= 15).all()
    n = n.round().long()
    return torch.cat([((n >> gI) & 1).bool() for gI in range(4)], dim=-1)


@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("rows", [128, 256])
@pytest.mark.parametrize("bnhd", [False, True])
def test_mask_readback_forward(D, rows, bnhd):
    dev = _dev()
    B, H, Nq, seed = 2, 3, 200, 2 ** 40 + 12345
    q, k, v, Nkv = _readback_inputs(B, H, Nq, D, dev)
    if bnhd:
        q, k, v = (t.transpose(1, 2).contiguous() for t in (q, k, v))
    with _fa2_lib.options(rows=rows):
        o = flash_attention(q, k, v, BNHD_fmt=bnhd, dropout_p=0.5, dropout_seed=seed)
    o = (o.transpose(1, 2) if bnhd else o).cpu()
    want = dropout_keep_mask(seed, 0.5, B, H, Nq, Nkv)
    got = _decode(o, Nkv, D)
    bad = (got != want).sum().item()
    print("readback D%d rows %d bnhd %d: %d of %d mask elements differ; keep rate %.4f" % (D, rows, bnhd, bad, want.numel(), got.float().mean().item()))
    assert bad == 0


@pytest.mark.parametrize("D", [64, 256])
def test_mask_readback_packed(D):
    dev = _dev()
    H, seed, lens = 2, 77, [70, 1, 130]
    Nkv = 4 * D
    q, k, v, _ = _readback_inputs(1, H, sum(lens), D, dev)
    qp = q[0].transpose(0, 1).contiguous()                                                  # [total_q, H, D]
    kp = torch.zeros(len(lens) * Nkv, H, D, dtype=torch.float16, device=dev)
    vp = v[0].transpose(0, 1).repeat(len(lens), 1, 1).contiguous()                        # every sequence: the same 4 D keys
    cu_q = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev)
    cu_k = torch.arange(len(lens) + 1, dtype=torch.int32, device=dev) * Nkv
    o = flash_attention_varlen(qp, kp, vp, cu_q, cu_k, max(lens), Nkv, dropout_p=0.5, dropout_seed=seed).cpu()
    want = dropout_keep_mask(seed, 0.5, len(lens), H, max(lens), Nkv)                         # b = the sequence, rows counted inside it
    r0 = 0
    for s, n in enumerate(lens):
        got = _decode(o[r0:r0 + n].transpose(0, 1), Nkv, D)
        assert (got == want[s, :, :n]).all(), ("sequence", s)
        r0 += n


# ---- 2. forward and gradients against float64
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [40, 64, 128, 256, 512])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_forward_and_gradients_against_float64(dt, D, causal, p):
    _dense_case(dt, 1, 4, 4, 200, 333, D, causal, p, seed=2 ** 33 + 7 * D + causal, gseed=D)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
def test_window_offset_grouped_and_layouts(dt, D):
    _dense_case(dt, 2, 4, 4, 200, 333, D, False, 0.1, seed=11, window=(60, 40), q_offset=100, gseed=1)
    _dense_case(dt, 1, 4, 4, 300, 333, D, True, 0.5, seed=12, window=(100, None), q_offset=33, gseed=2)
    _dense_case(dt, 1, 8, 2, 200, 333, D, True, 0.1, seed=13, gseed=3)                      # grouped k / v: the mask is keyed by the query head
    _dense_case(dt, 2, 8, 2, 200, 333, D, False, 0.5, seed=14, bnhd=True, gseed=4)
    _dense_case(dt, 1, 2, 1, 260, 200, D, True, 0.1, seed=15, window=(50, 0), gseed=5)      # rows past the keys' end under a window: dead rows


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [64, 128, 256, 512])
def test_short_key_ranges(dt, D):
    """Nkv <= 64: one wrong mask element in the dQ or the dK / dV pass moves a gradient far beyond the bar."""
    for i, (Nq, Nkv) in enumerate(((100, 64), (64, 33), (300, 17), (33, 8))):
        _dense_case(dt, 1, 2, 2, Nq, Nkv, D, False, 0.5, seed=900 + i, gseed=10 + i)
    _dense_case(dt, 1, 2, 2, 48, 48, D, True, 0.5, seed=950, gseed=20)


# ---- 3. packed batches
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D,H,Hkv", [(64, 4, 4), (128, 4, 2), (256, 2, 2)])
@pytest.mark.parametrize("causal,bottom_right", [(False, False), (True, True)])
def test_packed_against_float64(dt, D, H, Hkv, causal, bottom_right):
    dev = _dev()
    lq, lk = [0, 1, 77, 200, 130, 64], [5, 1, 77, 150, 0, 300]
    p, seed, scale, code, grp = 0.1 if D == 64 else 0.5, 2 ** 35 + D, D ** -0.5, _code(dt), H // Hkv
    g = torch.Generator().manual_seed(D)
    q, do = _rand((sum(lq), H, D), dt, g), _rand((sum(lq), H, D), dt, g)
    k, v = _rand((sum(lk), Hkv, D), dt, g), _rand((sum(lk), Hkv, D), dt, g)
    cu_q = torch.tensor([0] + list(np.cumsum(lq)), dtype=torch.int32, device=dev)
    cu_k = torch.tensor([0] + list(np.cumsum(lk)), dtype=torch.int32, device=dev)
    qd, kd, vd = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    o = flash_attention_varlen(qd, kd, vd, cu_q, cu_k, max(lq), max(lk), causal=causal, bottom_right=bottom_right, dropout_p=p, dropout_seed=seed)
    o.backward(do.to(dev))
    got_o, got_dq, got_dk, got_dv = (t.detach().cpu() for t in (o, qd.grad, kd.grad, vd.grad))
    keep = dropout_keep_mask(seed, p, len(lq), H, max(lq), max(lk))
    q0 = k0 = 0
    for s, (nq, nk) in enumerate(zip(lq, lk)):
        tag = "%s D%d packed seq %d (%d x %d) causal=%d" % (str(dt)[6:], D, s, nq, nk, causal)
        sq, sk = slice(q0, q0 + nq), slice(k0, k0 + nk)
        q0, k0 = q0 + nq, k0 + nk
        if nq == 0 or nk == 0:
            assert (got_o[sq] == 0).all() and (got_dq[sq] == 0).all() and (got_dk[sk] == 0).all() and (got_dv[sk] == 0).all(), tag
            continue
        band = _band(nq, nk, -1, -1, nk - nq if bottom_right else 0, causal)
        hm = lambda t: t.transpose(0, 1)                           # noqa: E731 - [n, H, D] -> [H, n, D]
        ke, ve = hm(k[sk]).repeat_interleave(grp, 0), hm(v[sk]).repeat_interleave(grp, 0)
        args = (hm(q[sq]), ke, ve, hm(do[sq]), keep[s, :, :nq, :nk], band, scale, p)
        true, emu = _ref64(*args), _emu(*args, dt)
        fold = lambda t: t.unflatten(0, (Hkv, grp)).sum(1)         # noqa: E731
        _check("O", hm(got_o[sq]), true[0], emu[0], FLOOR[code], tag)
        _check("dQ", hm(got_dq[sq]), true[2], emu[1], GRAD_TOL[code], tag)
        _check("dK", hm(got_dk[sk]), fold(true[3]), fold(emu[2]), GRAD_TOL[code], tag)
        _check("dV", hm(got_dv[sk]), fold(true[4]), fold(emu[3]), GRAD_TOL[code], tag)


# ---- 4. determinism, p = 0, the LSE
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
def test_determinism_p0_and_lse(dt, D):
    dev = _dev()
    B, H, Nq, Nkv, p = 2, 4, 300, 500, 0.3
    g = torch.Generator().manual_seed(D + 1)
    q, k, v, do = (_rand((B, H, n, D), dt, g).to(dev) for n in (Nq, Nkv, Nkv, Nq))

    def run(**kw):
        qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
        o = flash_attention(qq, kk, vv, causal=True, **kw)
        o.backward(do)
        return [t.detach() for t in (o, qq.grad, kk.grad, vv.grad)]
    a, b2, c = run(dropout_p=p, dropout_seed=5), run(dropout_p=p, dropout_seed=5), run(dropout_p=p, dropout_seed=6)
    assert all(torch.equal(x, y) for x, y in zip(a, b2)), "same seed: bit-identical O, dQ, dK, dV"
    assert not torch.equal(a[0], c[0]), "another seed: another mask"
    plain, p0 = run(), run(dropout_p=0.0)
    assert all(torch.equal(x, y) for x, y in zip(plain, p0)), "dropout_p = 0.0 is the call without the argument"
    # the LSE is the undropped call's: against the plain forward's and against float64 (log2 units)
    scale, flags = D ** -0.5, _fa2_lib.FA2_FLAG_CAUSAL | _fa2_lib.FA2_FLAG_EXACT_SCALE
    L_drop = flash_attn_wmma.forward_py(q, k, v, 64, 128, flags, scale, False, window=(-1, -1, 0), dropout=(p, 5))[5][:, :, :Nq]
    L_zero = flash_attn_wmma.forward_py(q, k, v, 64, 128, flags, scale, False, window=(-1, -1, 0), dropout=(0.0, 5))[5][:, :, :Nq]
    L_plain = flash_attn_wmma.forward_py(q, k, v, 64, 128, flags, scale, False)[5][:, :, :Nq]
    S = (q.double().cpu() @ k.double().cpu().transpose(-1, -2)) * scale
    S = S.masked_fill(~_band(Nq, Nkv, -1, -1, 0, True), float("-inf"))
    L_true = torch.logsumexp(S, -1) / LN2
    e0, e1, e2 = ((L_drop.cpu().double() - t.cpu().double()).abs().max().item() for t in (L_zero, L_plain, L_true))
    print("LSE of the dropout call vs p = 0 (same kernels) %.3g, vs the plain call %.3g, vs float64 %.3g (bar %.3g)" % (e0, e1, e2, LSE_TOL))
    assert e0 <= LSE_TOL and e1 <= LSE_TOL and e2 <= LSE_TOL


# ---- 5. dropout_seed=None follows torch.manual_seed
def test_default_seed_reproduces_under_manual_seed():
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    q, k, v = (_rand((1, 2, 130, 64), torch.float16, g).to(dev) for _ in range(3))
    torch.manual_seed(4321)
    a = flash_attention(q, k, v, dropout_p=0.2)
    b2 = flash_attention(q, k, v, dropout_p=0.2)
    torch.manual_seed(4321)
    c = flash_attention(q, k, v, dropout_p=0.2)
    assert torch.equal(a, c) and not torch.equal(a, b2)
    # dropout applies without grad mode, too (as scaled_dot_product_attention)
    with torch.no_grad():
        torch.manual_seed(4321)
        assert torch.equal(flash_attention(q, k, v, dropout_p=0.2), a)
    assert not torch.equal(a, flash_attention(q, k, v))
