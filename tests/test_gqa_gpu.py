"""Grouped-query / multi-query attention on the GPU (fa2_fwd_gqa / fa2_bwd_gqa and the operator): the forward is bit-identical to the MHA call on
K / V expanded with repeat_interleave, in every forward kernel family; the backward's dK / dV (summed over each group in-kernel) meet the float64 bars
of tests/conftest.py and are never further from float64 than the MHA call on expanded K / V with its gradients summed over the group in float64."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from conftest import ATOL, FLOOR, GRAD_TOL, LSE_TOL, LSE_TOL_P16_BF16, LSE_TRUTH_TOL, RTOL
from oracle import fa2_oracle as fo
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import FlashAttentionFunction, _frontend, flash_attention, flash_attn_wmma

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    return torch.device("cuda", 0)


def _s3(t, bnhd):
    st = t.stride()
    return _fa2_lib.strides3(st[0], st[2], st[1]) if bnhd else _fa2_lib.strides3(st[0], st[1], st[2])


def _rand(shape, dt, g, bnhd, scale=1.0):
    B, H, N, D = shape
    t = (torch.randn((B, N, H, D) if bnhd else (B, H, N, D), generator=g) * scale).to(dt)
    return t.to(_dev())


def _expand(t, g, bnhd):
    return t.repeat_interleave(g, dim=2 if bnhd else 1).contiguous() if g > 1 else t


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _code(dt):
    return _fa2_lib.FA2_DTYPE_F16 if dt == torch.float16 else _fa2_lib.FA2_DTYPE_BF16


def _fwd(q, k, v, B, H, Hkv, Nq, Nkv, D, causal, bnhd, gqa, ws=True, flags=0):
    """One forward through the C-ABI: fa2_fwd_gqa (gqa) or fa2_fwd_ws, with the workspace the library asks for (ws)."""
    lib = _fa2_lib.load()
    dt = _code(q.dtype)
    o = torch.empty_like(q)
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    need = lib.fa2_fwd_workspace_bytes(dt, B, H, Nq, Nkv, D, int(causal)) if ws else 0
    w = torch.empty(max(need, 16), dtype=torch.uint8, device=q.device)
    s2 = _fa2_lib.strides2(H * Nq, Nq)
    args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr())
    strides = (_s3(q, bnhd), _s3(k, bnhd), _s3(v, bnhd), _s3(o, bnhd), s2)
    if gqa:
        rc = lib.fa2_fwd_gqa(dt, *args, B, H, Hkv, Nq, Nkv, D, *strides, D ** -0.5, int(causal) | flags, w.data_ptr() if need else None, need, _stream())
    else:
        rc = lib.fa2_fwd_ws(dt, *args, B, H, Nq, Nkv, D, *strides, D ** -0.5, int(causal), w.data_ptr() if need else None, need, _stream())
    _fa2_lib.check(rc)
    torch.cuda.synchronize()
    return o, lse


def _dense(q, k, v, causal, bnhd):
    """float64 attention of (expanded) BHND / BNHD tensors."""
    if bnhd:
        q, k, v = (t.transpose(1, 2) for t in (q, k, v))
    s = (q.double() @ k.double().transpose(-1, -2)) * q.shape[-1] ** -0.5
    if causal:
        nq, nk = s.shape[-2:]
        s = s.masked_fill(torch.ones(nq, nk, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    o = torch.softmax(s, -1) @ v.double()
    return o.transpose(1, 2) if bnhd else o


HEADS = [(8, 8), (8, 2), (12, 4), (32, 8), (16, 1)]


def _bhnd(t, bnhd):
    return t.transpose(1, 2) if bnhd else t


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _check_heads_vs_oracle_and_truth(o, lse, q, k, v, g, causal, bnhd, plan):
    """Sampled Q heads (first and last of the first and last batch) against the same-contract C oracle and float64 truth, each on the K / V head the
    group maps it to, under the tests/conftest.py bars (O: oracle ATOL / RTOL, truth FLOOR; LSE: oracle LSE_TOL, truth LSE_TRUTH_TOL)."""
    dt = _code(q.dtype)
    qb, kb, vb, ob = (_bhnd(t, bnhd) for t in (q, k, v, o))
    B, H, Nq, D = qb.shape
    for b, h in {(0, 0), (0, H - 1), (B - 1, 0), (B - 1, H - 1)}:
        contract = plan.contract if b * H + h < plan.heads_main else plan.contract_tail
        flags = (fo.PRESCALE_Q if contract & _fa2_lib.FA2_CONTRACT_PRESCALE_Q else 0) | (fo.LSUM_P16 if contract & _fa2_lib.FA2_CONTRACT_LSUM_P16 else 0)
        if dt == 0 and flags & fo.PRESCALE_Q:
            flags |= fo.PRESCALE_FUSED
        qs, ks, vs = qb[b:b + 1, h:h + 1], kb[b:b + 1, h // g:h // g + 1], vb[b:b + 1, h // g:h // g + 1]
        o_ref_bits, lse_ref = fo.fwd_c(_bits(qs), _bits(ks), _bits(vs), dt, causal, flags=flags)
        got = ob[b, h].float().cpu().numpy()
        o_ref = fo.bits_to_f32(o_ref_bits, dt)[0, 0]
        assert np.all(np.abs(got - o_ref) <= ATOL[dt] + RTOL[dt] * np.abs(o_ref)), ("oracle O", b, h, float(np.abs(got - o_ref).max()))
        lse_tol = LSE_TOL_P16_BF16 if (dt == 1 and flags & fo.LSUM_P16) else LSE_TOL
        got_l = lse[b, h].cpu().numpy()
        assert np.abs(got_l - lse_ref[0, 0]).max() <= lse_tol, ("oracle LSE", b, h)
        s = (qs.double() @ ks.double().transpose(-1, -2)) * D ** -0.5
        if causal:
            s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool, device=s.device).triu(1), float("-inf"))
        want = torch.softmax(s, -1) @ vs.double()
        # against truth: conftest's max(2 * the reference's error, floor), with the same-contract oracle in the reference's role
        o_ref_err = (torch.from_numpy(o_ref).to(want.device).double() - want[0, 0]).abs().max().item()
        assert (ob[b, h].double() - want[0, 0]).abs().max().item() <= max(2 * o_ref_err, FLOOR[dt]), ("truth O", b, h, o_ref_err)
        lse_true = torch.logsumexp(s, -1)[0, 0] / math.log(2.0)
        l_ref_err = (torch.from_numpy(lse_ref[0, 0]).to(want.device).double() - lse_true).abs().max().item()
        assert (lse[b, h].double() - lse_true).abs().max().item() <= max(2 * l_ref_err, LSE_TRUTH_TOL[dt]), ("truth LSE", b, h, l_ref_err)

# (B, Nq, Nkv, D, causal, bnhd, dtype): the HIP 256 / 128 and trimmed kernels (D 40, 80, 160, 512), the short kernel (Nkv 77), the hand-scheduled
# D64 / D128 bodies (long non-causal sweeps, causal from 1792 keys), the hand-scheduled D = 256 kernel (D 192, 256), ragged Nq / Nkv
FWD_CASES = [
    (1, 300, 333, 40, False, False, torch.float16), (1, 257, 200, 80, True, True, torch.bfloat16), (1, 200, 320, 160, False, False, torch.bfloat16),
    (1, 130, 100, 512, True, False, torch.float16), (2, 1000, 77, 64, False, True, torch.float16), (2, 1000, 77, 128, False, False, torch.bfloat16),
    (1, 1024, 1024, 64, True, False, torch.float16), (1, 1024, 1024, 128, False, True, torch.float16), (1, 1024, 2048, 128, True, False, torch.bfloat16),
    (1, 512, 1024, 192, False, False, torch.float16), (1, 512, 1024, 256, False, True, torch.bfloat16), (1, 1100, 2048, 256, True, False, torch.float16),
]


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "B%d_N%dx%d_D%d_%s_%s_%s" % (c[0], c[1], c[2], c[3], "c" if c[4] else "nc",
                                                                                     "bnhd" if c[5] else "bhnd", str(c[6])[6:]))
def test_forward_is_bit_identical_to_the_expanded_mha_call(case):
    B, Nq, Nkv, D, causal, bnhd, dt = case
    g = torch.Generator(device="cpu").manual_seed(Nq * 7 + D)
    for H, Hkv in HEADS:
        if H * Nq * Nkv > 32 * 1024 * 1100 and (H, Hkv) != (8, 2):
            continue                                 # (the longest sweeps: one grouping is enough)
        q = _rand((B, H, Nq, D), dt, g, bnhd)
        k = _rand((B, Hkv, Nkv, D), dt, g, bnhd)
        v = _rand((B, Hkv, Nkv, D), dt, g, bnhd)
        o, lse = _fwd(q, k, v, B, H, Hkv, Nq, Nkv, D, causal, bnhd, gqa=True)
        ke, ve = _expand(k, H // Hkv, bnhd), _expand(v, H // Hkv, bnhd)
        o_m, lse_m = _fwd(q, ke, ve, B, H, Hkv, Nq, Nkv, D, causal, bnhd, gqa=False)
        assert torch.equal(o, o_m) and torch.equal(lse, lse_m), (H, Hkv)
        # the same kernels: the grouped plan is the MHA plan
        qm = q if not bnhd else q.transpose(1, 2)
        assert _fa2_lib.gqa_plan(qm, k if not bnhd else k.transpose(1, 2), causal).as_dict() == \
            _fa2_lib.fwd_plan(qm, ke if not bnhd else ke.transpose(1, 2), causal).as_dict()
        need = _fa2_lib.load().fa2_fwd_workspace_bytes(_code(dt), B, H, Nq, Nkv, D, int(causal))      # (the workspace _fwd handed over)
        _check_heads_vs_oracle_and_truth(o, lse, q, k, v, H // Hkv, causal, bnhd,
                                         _fa2_lib.gqa_plan(qm, k if not bnhd else k.transpose(1, 2), causal, workspace_bytes=need))


@pytest.mark.parametrize("shape", [(2, 10, 2, 4096, 4096, 64), (1, 32, 8, 1, 8192, 128), (1, 32, 1, 1, 8192, 128), (1, 16, 4, 2048, 4096, 128)],
                         ids=["tail_split_d64", "decode_hkv8", "decode_mqa", "underfilled_d128"])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_forward_split_plans_are_bit_identical(shape, dt):
    """The tail split (B2 H10 N4096 D64) and the decode split (B1 H32 Nq1 Nkv8192) with the workspace: the grouped call is the MHA call bit for bit."""
    B, H, Hkv, Nq, Nkv, D = shape
    g = torch.Generator(device="cpu").manual_seed(5)
    for bnhd in (False, True):
        q = _rand((B, H, Nq, D), dt, g, bnhd)
        k = _rand((B, Hkv, Nkv, D), dt, g, bnhd)
        v = _rand((B, Hkv, Nkv, D), dt, g, bnhd)
        o, lse = _fwd(q, k, v, B, H, Hkv, Nq, Nkv, D, False, bnhd, gqa=True)
        o_m, lse_m = _fwd(q, _expand(k, H // Hkv, bnhd), _expand(v, H // Hkv, bnhd), B, H, Hkv, Nq, Nkv, D, False, bnhd, gqa=False)
        assert torch.equal(o, o_m) and torch.equal(lse, lse_m)
    need = _fa2_lib.load().fa2_fwd_gqa_workspace_bytes(_code(dt), B, H, Hkv, Nq, Nkv, D, 0)
    assert need == _fa2_lib.load().fa2_fwd_workspace_bytes(_code(dt), B, H, Nq, Nkv, D, 0)


def _grad_err_bars(q, k, v, do, causal, bnhd, g):
    """(float64 truth of dQ, dK, dV; the errors of the MHA call on expanded K / V, its dK / dV summed over each group in float64)."""
    h_ax = 2 if bnhd else 1
    q64, k64, v64 = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    o64 = _dense(q64, k64.repeat_interleave(g, dim=h_ax), v64.repeat_interleave(g, dim=h_ax), causal, bnhd)
    o64.backward(do.double())
    truth = (q64.grad, k64.grad, v64.grad)
    qe = q.detach().clone().requires_grad_(True)
    ke = _expand(k.detach(), g, bnhd).requires_grad_(True)
    ve = _expand(v.detach(), g, bnhd).requires_grad_(True)
    FlashAttentionFunction.apply(qe, ke, ve, None, causal, None, bnhd).backward(do)

    def group_sum(t):
        t = t.double()
        if bnhd:
            B, N, H, D = t.shape
            return t.view(B, N, H // g, g, D).sum(3)
        B, H, N, D = t.shape
        return t.view(B, H // g, g, N, D).sum(2)
    mha = (qe.grad.double(), group_sum(ke.grad), group_sum(ve.grad))
    return truth, [(m - t).abs().max().item() for m, t in zip(mha, truth)]


def _check_grads(got, truth, mha_err, dt, what):
    for name, x, t, e in zip("qkv", got, truth, mha_err):
        assert x is not None and torch.isfinite(x).all(), (what, name)
        err = (x.double() - t).abs().max().item()
        bar = max(2 * e, GRAD_TOL[_code(dt)] * max(1.0, t.abs().max().item()))
        assert err <= bar, (what, name, err, bar, e)


# (B, H, Hkv, Nq, Nkv, D, causal, bnhd, dtype): D 64 fused pass, D 96 wave pairs, D 128 (hand-scheduled dQ + wave pairs), D 160 / 256 / 512 slabs,
# causal ragged, cross-attention over 77 keys (the split over the virtual sweep), MQA
BWD_CASES = [
    (2, 8, 2, 384, 384, 64, False, False, torch.float16), (1, 12, 4, 333, 250, 64, True, True, torch.bfloat16),
    (1, 8, 2, 320, 320, 96, False, True, torch.float16), (1, 12, 4, 300, 300, 96, True, False, torch.bfloat16),
    (1, 8, 2, 512, 512, 128, False, False, torch.float16), (1, 32, 8, 256, 256, 128, True, False, torch.bfloat16),
    (1, 8, 2, 320, 256, 128, False, True, torch.bfloat16), (1, 16, 1, 256, 300, 128, True, True, torch.float16),
    (1, 8, 2, 200, 160, 160, False, False, torch.float16), (1, 12, 4, 150, 150, 256, True, True, torch.bfloat16),
    (1, 8, 2, 130, 100, 512, False, False, torch.float16), (1, 16, 1, 96, 96, 512, True, False, torch.bfloat16),
    (2, 10, 2, 4096, 77, 64, False, False, torch.float16), (2, 10, 2, 4096, 77, 64, False, True, torch.bfloat16),
    (1, 16, 1, 1000, 1000, 64, False, False, torch.float16), (1, 8, 8, 256, 256, 64, True, False, torch.float16),
]


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: "H%d_Hkv%d_N%dx%d_D%d_%s_%s_%s" % (c[1], c[2], c[3], c[4], c[5], "c" if c[6] else "nc",
                                                                                          "bnhd" if c[7] else "bhnd", str(c[8])[6:]))
def test_backward_against_float64_and_the_expanded_mha_call(case):
    B, H, Hkv, Nq, Nkv, D, causal, bnhd, dt = case
    g = torch.Generator(device="cpu").manual_seed(H * 31 + D + Nq)
    q = _rand((B, H, Nq, D), dt, g, bnhd, 0.5).requires_grad_(True)
    k = _rand((B, Hkv, Nkv, D), dt, g, bnhd, 0.5).requires_grad_(True)
    v = _rand((B, Hkv, Nkv, D), dt, g, bnhd, 0.5).requires_grad_(True)
    do = _rand((B, H, Nq, D), dt, g, bnhd)
    o = FlashAttentionFunction.apply(q, k, v, None, causal, None, bnhd)
    o.backward(do)
    assert k.grad.shape == k.shape and v.grad.shape == v.shape
    truth, mha_err = _grad_err_bars(q, k, v, do, causal, bnhd, H // Hkv)
    _check_grads((q.grad, k.grad, v.grad), truth, mha_err, dt, case)


def _bwd_c(q, k, v, o, do, lse, H, Hkv, causal, ws, bnhd=False):
    """fa2_bwd_gqa (the in-kernel group sum) on BHND / BNHD tensors, with (ws) or without the workspace."""
    lib = _fa2_lib.load()
    B, _, Nq, D = _bhnd(q, bnhd).shape
    Nkv = _bhnd(k, bnhd).shape[2]
    dt = _code(q.dtype)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    need = lib.fa2_bwd_gqa_workspace_bytes(dt, B, H, Hkv, Nq, Nkv, D, int(causal)) if ws else 0
    w = torch.empty(max(need, 16), dtype=torch.uint8, device=q.device)
    s = lambda t: _s3(t, bnhd)  # noqa: E731
    rc = lib.fa2_bwd_gqa(dt, q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                         dv.data_ptr(), delta.data_ptr(), B, H, Hkv, Nq, Nkv, D, s(q), s(k), s(v), s(o), s(do), s(dq), s(dk), s(dv),
                         _fa2_lib.strides2(lse.stride(0), lse.stride(1)), D ** -0.5, int(causal), w.data_ptr() if need else None, need, _stream())
    _fa2_lib.check(rc)
    torch.cuda.synchronize()
    return dq, dk, dv, need


def _oracle_grad_bars(q, k, v, o, do, lse, causal, bnhd, g):
    """float64 truth of dQ, dK, dV, the same-contract C oracle's gradients (on expanded K / V, dK / dV summed over each group in float64) and the
    oracle's own error against truth — the role the reference's error plays in the tests/conftest.py gradient bar."""
    h_ax = 2 if bnhd else 1
    q64, k64, v64 = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    _dense(q64, k64.repeat_interleave(g, dim=h_ax), v64.repeat_interleave(g, dim=h_ax), causal, bnhd).backward(do.double())
    truth = tuple(_bhnd(t.grad, bnhd) for t in (q64, k64, v64))
    dt = _code(q.dtype)
    qb, ob, gb = (_bhnd(t, bnhd) for t in (q, o, do))
    kb, vb = (_bhnd(_expand(t.detach(), g, bnhd), bnhd) for t in (k, v))
    want = fo.bwd_c(_bits(qb), _bits(kb), _bits(vb), _bits(ob), _bits(gb), lse.cpu().numpy(), dt, causal)
    dq_o, dk_o, dv_o = (torch.from_numpy(fo.bits_to_f32(w, dt).astype(np.float64)).to(q.device) for w in want)
    B, H, Nkv, D = dk_o.shape
    orc = (dq_o, dk_o.view(B, H // g, g, Nkv, D).sum(2), dv_o.view(B, H // g, g, Nkv, D).sum(2))
    return truth, orc, [(x - t).abs().max().item() for x, t in zip(orc, truth)]


def _check_vs_oracle(got, truth, orc, orc_err, dt, g, what):
    """conftest's gradient bars: against truth max(2 * the oracle's error, GRAD_TOL * max(1, max|g_true|)); against the oracle GRAD_TOL *
    max(1, max|g_oracle|), plus, for dK / dV, the oracle's own g roundings of its per-head gradients before the group sum (half an ulp each)."""
    for i, (name, x, t, w, e) in enumerate(zip("qkv", got, truth, orc, orc_err)):
        x = _bhnd(x, False).double()
        assert torch.isfinite(x).all(), (what, name)
        err_t = (x - t).abs().max().item()
        bar_t = max(2 * e, GRAD_TOL[dt] * max(1.0, t.abs().max().item()))
        assert err_t <= bar_t, (what, name, "truth", err_t, bar_t)
        err_o = (x - w).abs().max().item()
        bar_o = GRAD_TOL[dt] * max(1.0, w.abs().max().item()) * (1.0 + (g / 4.0 if i else 0.0))
        assert err_o <= bar_o, (what, name, "oracle", err_o, bar_o)


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: "H%d_Hkv%d_N%dx%d_D%d_%s_%s_%s" % (c[1], c[2], c[3], c[4], c[5], "c" if c[6] else "nc",
                                                                                          "bnhd" if c[7] else "bhnd", str(c[8])[6:]))
def test_in_kernel_group_sum_against_the_oracle_and_float64(case):
    """fa2_bwd_gqa — the dK / dV passes that sweep every member head of a group (D 64 fused, D 96 / 128 wave pairs with the hand-scheduled dQ pass
    at 128, D 160 / 256 / 512 slabs, causal ragged, the split over the virtual sweep at 77 keys, MQA) — against the C oracle on expanded K / V."""
    B, H, Hkv, Nq, Nkv, D, causal, bnhd, dt = case
    g = torch.Generator(device="cpu").manual_seed(H * 17 + D + Nkv)
    q = _rand((B, H, Nq, D), dt, g, bnhd, 0.5)
    k = _rand((B, Hkv, Nkv, D), dt, g, bnhd, 0.5)
    v = _rand((B, Hkv, Nkv, D), dt, g, bnhd, 0.5)
    do = _rand((B, H, Nq, D), dt, g, bnhd)
    o, lse = _fwd(q, k, v, B, H, Hkv, Nq, Nkv, D, causal, bnhd, gqa=True, flags=_fa2_lib.FA2_FLAG_EXACT_SCALE)
    got = _bwd_c(q, k, v, o, do, lse, H, Hkv, causal, ws=not causal, bnhd=bnhd)
    truth, orc, orc_err = _oracle_grad_bars(q, k, v, o, do, lse, causal, bnhd, H // Hkv)
    _check_vs_oracle([_bhnd(x, bnhd) for x in got[:3]], truth, orc, orc_err, _code(dt), H // Hkv, case)


@pytest.mark.parametrize("shape", [(2, 10, 2, 4096, 77, 64), (1, 8, 1, 2048, 256, 64), (1, 16, 4, 1024, 1024, 64)], ids=["cross77", "mqa", "gqa"])
def test_backward_with_and_without_the_workspace(shape):
    """The split of the fused dK / dV pass over the virtual sweep of g x (Q tiles) changes the f32 summation order only."""
    B, H, Hkv, Nq, Nkv, D = shape
    dt = torch.float16
    g = torch.Generator(device="cpu").manual_seed(11)
    q = _rand((B, H, Nq, D), dt, g, False, 0.5)
    k = _rand((B, Hkv, Nkv, D), dt, g, False, 0.5)
    v = _rand((B, Hkv, Nkv, D), dt, g, False, 0.5)
    do = _rand((B, H, Nq, D), dt, g, False)
    o, lse = _fwd(q, k, v, B, H, Hkv, Nq, Nkv, D, False, False, gqa=True, ws=False, flags=_fa2_lib.FA2_FLAG_EXACT_SCALE)
    a = _bwd_c(q, k, v, o, do, lse, H, Hkv, False, ws=False)
    b = _bwd_c(q, k, v, o, do, lse, H, Hkv, False, ws=True)
    if shape[4] == 77:
        assert b[3] > 0                              # the cross-attention shape does split
    truth, orc, orc_err = _oracle_grad_bars(q, k, v, o, do, lse, False, False, H // Hkv)
    _check_vs_oracle(a[:3], truth, orc, orc_err, _code(dt), H // Hkv, ("plain", shape))
    _check_vs_oracle(b[:3], truth, orc, orc_err, _code(dt), H // Hkv, ("split", shape))


def test_operator_front_ends_agree_and_route_grouped_shapes():
    """Compiled and Python front ends: identical outputs and gradients for grouped shapes; flash_attention and FlashAttentionFunction.apply agree."""
    from rocwmma_fattn import FlashAttn as fa
    dev = _dev()
    fe = _frontend()
    # the compiled front end is compared whenever build.py produced it (it is optional: without it both entries ARE the Python path)
    assert fe is not None or not os.path.exists(os.path.join(os.path.dirname(fa.__file__), "_fa2_frontend.so"))
    g = torch.Generator(device="cpu").manual_seed(3)
    for (B, H, Hkv, N, Nkv, D), dt, causal, bnhd in ((((2, 8, 2, 200, 150, 64)), torch.float16, False, False),
                                                     (((1, 12, 4, 256, 256, 128)), torch.bfloat16, True, True),
                                                     (((1, 16, 1, 100, 333, 40)), torch.float16, False, False)):
        q = _rand((B, H, N, D), dt, g, bnhd)
        k = _rand((B, Hkv, Nkv, D), dt, g, bnhd)
        v = _rand((B, Hkv, Nkv, D), dt, g, bnhd)
        do = _rand((B, H, N, D), dt, g, bnhd)
        py = flash_attn_wmma.forward_py(q, k, v, 64, 128, causal, D ** -0.5, bnhd)
        if fe is not None:
            c = fe.forward(q, k, v, 64, 128, causal, D ** -0.5, bnhd)
            for x, y in zip(c, py):
                assert torch.equal(x, y)
            _, qb, kb, vb, ob, L = flash_attn_wmma.forward_py(q, k, v, 64, 128, int(causal) | _fa2_lib.FA2_FLAG_EXACT_SCALE, D ** -0.5, bnhd)
            n_ax = 1 if bnhd else 2
            cg = fe.backward(qb, kb, vb, ob, do, L, q.shape[n_ax], k.shape[n_ax], D, 128, 128, causal, D ** -0.5, bnhd)
            pg = flash_attn_wmma.backward_py(qb, kb, vb, ob, do, L, q.shape[n_ax], k.shape[n_ax], D, 128, 128, causal, D ** -0.5, bnhd)
            for x, y in zip(cg, pg):
                assert x.shape == y.shape and torch.equal(x, y)
        pyx = flash_attn_wmma.forward_py(q, k, v, 64, 128, int(causal) | _fa2_lib.FA2_FLAG_EXACT_SCALE, D ** -0.5, bnhd)    # (what a differentiated call runs)
        grads = []
        for use in ("apply", "flash_attention"):
            qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
            o = FlashAttentionFunction.apply(qq, kk, vv, None, causal, None, bnhd) if use == "apply" else flash_attention(qq, kk, vv, causal=causal, BNHD_fmt=bnhd)
            o.backward(do)
            assert torch.equal(o.detach(), pyx[0])
            grads.append((qq.grad, kk.grad, vv.grad))
        _, qb, kb, vb, ob, L = pyx
        n_ax = 1 if bnhd else 2
        pyg = flash_attn_wmma.backward_py(qb, kb, vb, ob, do, L, q.shape[n_ax], k.shape[n_ax], D, 128, 128, causal, D ** -0.5, bnhd)
        for a, b in zip(grads[0], grads[1]):
            assert torch.equal(a, b)
        for a, b in zip(grads[0], pyg):
            assert torch.equal(a, b)
    assert dev.type == "cuda"


def test_masked_grouped_calls_expand_on_the_host():
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(4)
    B, H, Hkv, N, Nkv, D = 2, 8, 2, 130, 77, 64
    q = _rand((B, H, N, D), torch.float16, g, False, 0.5).requires_grad_(True)
    k = _rand((B, Hkv, Nkv, D), torch.float16, g, False, 0.5).requires_grad_(True)
    v = _rand((B, Hkv, Nkv, D), torch.float16, g, False, 0.5).requires_grad_(True)
    mask = (torch.rand((B, 1, 1, Nkv), generator=g) > 0.2).to(dev)
    do = _rand((B, H, N, D), torch.float16, g, False)
    o = flash_attention(q, k, v, mask=mask)
    o.backward(do)
    ke, ve = _expand(k.detach(), 4, False), _expand(v.detach(), 4, False)
    assert torch.equal(o.detach(), flash_attention(q.detach(), ke, ve, mask=mask))
    q64, k64, v64 = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    s = (q64 @ k64.repeat_interleave(4, 1).transpose(-1, -2)) * D ** -0.5
    o64 = torch.softmax(s.masked_fill(~mask, float("-inf")), -1) @ v64.repeat_interleave(4, 1)
    o64.backward(do.double())
    for x, t in zip((q.grad, k.grad, v.grad), (q64.grad, k64.grad, v64.grad)):
        assert (x.double() - t).abs().max().item() <= 2 * GRAD_TOL[0] * max(1.0, t.abs().max().item())


def test_a_head_count_that_does_not_divide_raises():
    dev = _dev()
    q = torch.randn((1, 8, 64, 64), device=dev, dtype=torch.float16)
    k = torch.randn((1, 3, 64, 64), device=dev, dtype=torch.float16)
    with pytest.raises(RuntimeError, match=r"\(3\).*\(8\)"):
        FlashAttentionFunction.apply(q, k, k, None, False)
    with pytest.raises(RuntimeError, match=r"\(3\).*\(8\)"):
        flash_attn_wmma.forward_py(q, k, k, 64, 128, False, 0.125, False)
    with pytest.raises(RuntimeError, match=r"\(3\).*\(8\)"):
        FlashAttentionFunction.apply(q.requires_grad_(True), k, k, None, False)
    with pytest.raises(RuntimeError, match=r"\(3\).*\(8\)"):
        flash_attention(q, k, k, mask=torch.ones((64, 64), dtype=torch.bool, device=dev))
