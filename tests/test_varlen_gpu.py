"""Packed, variable-length attention on the GPU: fa2_fwd_varlen / fa2_bwd_varlen and flash_attention_varlen.

The reference is the repository's oracle run PER SEQUENCE on that sequence's slice, the band given as a -inf bias (fa2_oracle.fwd_c / bwd_c: the same
contract 0 arithmetic; fwd_numpy / bwd_numpy: dense float64), as tests/test_window_gpu.py does for one window.  Zero-length slices are checked
directly.  Tolerances are tests/conftest.py's: ATOL / RTOL / LSE_TOL against the oracle, 2 * FLOOR against float64, the two GRAD_TOL rules of
tests/test_window_gpu.py for gradients.  Where the windowed kernel serves a sequence on its own, the packed result must equal it bit for bit: it is
the same instruction stream on the same data."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import ATOL, FLOOR, GRAD_TOL, LSE_TOL, RTOL
from oracle import fa2_oracle as fo
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention, flash_attention_varlen

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
CAUSAL, EXACT, BR = _fa2_lib.FA2_FLAG_CAUSAL, _fa2_lib.FA2_FLAG_EXACT_SCALE, _fa2_lib.FA2_FLAG_BOTTOM_RIGHT

# (q lengths, k lengths): 1, 63, 64, 65, 257, 1000 and a zero-length sequence on the q side and on the k side; the second set has Nq_s != Nkv_s,
# sequences with fewer keys than queries (1000 / 257, 300 / 100, 64 / 1) and an empty sequence on each side
LENSETS = {
    "self": ((1, 63, 64, 65, 257, 1000, 0, 300), (1, 63, 64, 65, 257, 1000, 0, 300)),
    "cross": ((65, 0, 1000, 257, 64, 1, 63, 300), (1000, 64, 257, 0, 1, 65, 63, 100)),
}
# (flags, window_left, window_right): plain, causal top-left, causal bottom-right, window (left, 0), a two-sided window
VARIANTS = {"plain": (0, -1, -1), "causal": (CAUSAL, -1, -1), "causal_br": (CAUSAL | BR, -1, -1), "left": (0, 100, 0), "band_br": (BR, 70, 30)}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    return torch.device("cuda", 0)


def _code(dt):
    return _fa2_lib.FA2_DTYPE_F16 if dt == torch.float16 else _fa2_lib.FA2_DTYPE_BF16


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _s2(t):
    return _fa2_lib.strides2(t.stride(1), t.stride(0))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _cu(lens, dev=None):
    t = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    return t if dev is None else t.to(dev)


def _rand(shape, dt, g):
    return torch.randn(shape, generator=g).to(dt)


def _keep(Nq, Nkv, flags, left, right):
    """The [Nq, Nkv] visibility matrix of one sequence (the contract of include/fa2_gfx950.h)."""
    off = Nkv - Nq if flags & BR else 0
    if flags & CAUSAL:
        right = 0
    pos = np.arange(Nq)[:, None] + off
    j = np.arange(Nkv)[None, :]
    keep = np.ones((Nq, Nkv), dtype=bool)
    if left >= 0:
        keep &= j >= pos - left
    if right >= 0:
        keep &= j <= pos + right
    return keep


def _fwd_varlen(q, k, v, cu_q, cu_k, max_q, max_k, flags, left, right, o=None, lse=None, B=None):
    """fa2_fwd_varlen on packed tensors; outputs pre-filled with NaN (every element below cu[B] must be written)."""
    lib = _fa2_lib.load()
    H, D = q.shape[1], q.shape[2]
    o = torch.full_like(q, float("nan")) if o is None else o
    lse = torch.full((H, q.shape[0]), float("nan"), dtype=torch.float32, device=q.device) if lse is None else lse
    _fa2_lib.check(lib.fa2_fwd_varlen(_code(q.dtype), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), cu_q.numel() - 1 if B is None else B,
                                      H, k.shape[1], max_q, max_k, D, cu_q.data_ptr(), cu_k.data_ptr(), _s2(q), _s2(k), _s2(v), _s2(o), lse.stride(0), D ** -0.5,
                                      flags, left, right, _stream()))
    torch.cuda.synchronize()
    return o, lse


def _bwd_varlen(q, k, v, o, do, lse, cu_q, cu_k, max_q, max_k, flags, left, right, B=None):
    lib = _fa2_lib.load()
    H, D = q.shape[1], q.shape[2]
    dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
    delta = torch.empty_like(lse)
    _fa2_lib.check(lib.fa2_bwd_varlen(_code(q.dtype), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                                      dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), cu_q.numel() - 1 if B is None else B, H, max_q, max_k, D, cu_q.data_ptr(),
                                      cu_k.data_ptr(), *(_s2(t) for t in (q, k, v, o, do, dq, dk, dv)), lse.stride(0), D ** -0.5, flags, left, right, _stream()))
    torch.cuda.synchronize()
    return dq, dk, dv


def _seq(t, cu, s, g=1):
    """Sequence s of a packed CPU tensor as the oracle's [1, H, N, D] (grouped K / V expanded)."""
    x = t[int(cu[s]):int(cu[s + 1])].transpose(0, 1)
    return x.repeat_interleave(g, dim=0).unsqueeze(0).contiguous() if g > 1 else x.unsqueeze(0).contiguous()


def _check_forward(o, lse, q, k, v, lq, lk, flags, left, right, dt, tag):
    """Packed o / lse (device) against the oracle and float64, sequence by sequence; dead rows exactly 0 / -inf, everything below cu[B] finite."""
    code = _code(dt)
    cq, ck = np.concatenate([[0], np.cumsum(lq)]), np.concatenate([[0], np.cumsum(lk)])
    g = q.shape[1] // k.shape[1]
    got_o, got_l = o.float().cpu(), lse.cpu()
    assert torch.isfinite(got_o).all(), (tag, "O not finite")
    assert not torch.isnan(got_l).any(), (tag, "LSE not written")
    worst = [0.0, 0.0, 0.0, 0.0]
    for s, (nq, nk) in enumerate(zip(lq, lk)):
        if nq == 0:
            continue
        go = got_o[cq[s]:cq[s + 1]].transpose(0, 1).unsqueeze(0).numpy()
        gl = got_l[:, cq[s]:cq[s + 1]].unsqueeze(0).numpy()
        if nk == 0:
            assert np.all(go == 0.0) and np.all(np.isneginf(gl)), (tag, s, "a sequence without keys")
            continue
        keep = _keep(nq, nk, flags, left, right)
        bias = np.where(keep, 0.0, -np.inf).astype(np.float32)
        qs, ks, vs = _seq(q, cq, s), _seq(k, ck, s, g), _seq(v, ck, s, g)
        o_ref_bits, lse_ref = fo.fwd_c(_bits(qs), _bits(ks), _bits(vs), code, False, bias=bias)
        o_ref = fo.bits_to_f32(o_ref_bits, code)
        o_true, lse_true = fo.fwd_numpy(qs.float().numpy(), ks.float().numpy(), vs.float().numpy(), False, bias=bias)
        dead = ~keep.any(1)
        err_o, err_t = np.abs(go - o_ref), np.abs(go - o_true)
        live_l = np.abs(gl[..., ~dead] - lse_ref[..., ~dead]).max() if (~dead).any() else 0.0
        live_t = np.abs(gl[..., ~dead] - lse_true[..., ~dead]).max() if (~dead).any() else 0.0
        worst = [max(a, float(b)) for a, b in zip(worst, (err_o.max(), err_t.max(), live_l, live_t))]
        assert np.all(err_o <= ATOL[code] + RTOL[code] * np.abs(o_ref)), (tag, s, nq, nk, "oracle O", float(err_o.max()))
        assert err_t.max() <= 2 * FLOOR[code], (tag, s, nq, nk, "float64 O", float(err_t.max()))
        assert live_l <= LSE_TOL and live_t <= LSE_TOL, (tag, s, nq, nk, "LSE", live_l, live_t)
        if dead.any():
            assert np.all(go[:, :, dead] == 0.0) and np.all(np.isneginf(gl[:, :, dead])), (tag, s, "dead rows")
    print("%s: O vs oracle %.3g, vs float64 %.3g; LSE vs oracle %.3g, vs float64 %.3g" % ((tag,) + tuple(worst)))


def _window_twin(q, k, v, cq, ck, s, flags, left, right):
    """fa2_fwd_window on sequence s alone (BNHD strides, B = 1, q_offset = off_s) -> (o [N, H, D], lse [H, N]), or None where that call is refused
    (a negative offset) or would not run the windowed kernel (a band that masks nothing for these lengths: the plain kernels serve it)."""
    lib = _fa2_lib.load()
    nq, nk = int(cq[s + 1] - cq[s]), int(ck[s + 1] - ck[s])
    off = nk - nq if flags & BR else 0
    if nq == 0 or nk == 0 or off < 0:
        return None
    H, Hkv, D = q.shape[1], k.shape[1], q.shape[2]
    qs, ks, vs = q[int(cq[s]):int(cq[s + 1])], k[int(ck[s]):int(ck[s + 1])], v[int(ck[s]):int(ck[s + 1])]

    def s3(t):
        return _fa2_lib.strides3(t.stride(0) * t.shape[0], t.stride(1), t.stride(0))
    plan = _fa2_lib.FwdPlan()
    _fa2_lib.check(lib.fa2_fwd_window_plan(_code(q.dtype), 1, H, Hkv, nq, nk, D, s3(qs), s3(ks), D ** -0.5, flags & CAUSAL, left, right, off, 0, ctypes.byref(plan)))
    if plan.kernel != _fa2_lib.FA2_KERNEL_HIP_WINDOW:
        return None
    o = torch.full_like(qs, float("nan"))
    lse = torch.full((H, nq), float("nan"), dtype=torch.float32, device=q.device)
    _fa2_lib.check(lib.fa2_fwd_window(_code(q.dtype), qs.data_ptr(), ks.data_ptr(), vs.data_ptr(), o.data_ptr(), lse.data_ptr(), 1, H, Hkv, nq, nk, D, s3(qs), s3(ks),
                                      s3(vs), s3(o), _fa2_lib.strides2(H * nq, nq), D ** -0.5, flags & CAUSAL, left, right, off, _stream()))
    torch.cuda.synchronize()
    return o, lse


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [40, 64, 80, 128, 192, 256, 512])
def test_forward_against_oracle_and_float64(D, dt):
    """Every masking variant on both length sets, both `rows` options: per-sequence oracle and float64, NaN-prefilled outputs finite below cu[B], dead
    rows exactly 0 / -inf — and each sequence bit-identical to the windowed kernel on that sequence alone wherever that kernel serves it."""
    dev = _dev()
    H = 2
    twins = 0
    for (lname, (lq, lk)), (vname, (flags, left, right)) in [(a, b) for a in LENSETS.items() for b in VARIANTS.items()]:
        g = torch.Generator(device="cpu").manual_seed(D + len(vname) + 7 * len(lname))
        q, k, v = _rand((sum(lq), H, D), dt, g), _rand((sum(lk), H, D), dt, g), _rand((sum(lk), H, D), dt, g)
        qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
        cq, ck = _cu(lq, dev), _cu(lk, dev)
        results = []
        for rows in (128, 256):
            with _fa2_lib.options(rows=rows):
                pl = _fa2_lib.varlen_plan(qd, kd, max(lq), max(lk), len(lq), flags, left, right)
                assert pl.kernel == _fa2_lib.FA2_KERNEL_HIP_VARLEN and pl.contract == 0 and pl.rows == (128 if D > 256 else rows)
                o, lse = _fwd_varlen(qd, kd, vd, cq, ck, max(lq), max(lk), flags, left, right)
                for s in range(len(lq)):
                    twin = _window_twin(qd, kd, vd, cq.cpu().numpy(), ck.cpu().numpy(), s, flags, left, right)
                    if twin is not None:
                        a, b = int(cq[s]), int(cq[s + 1])
                        assert torch.equal(o[a:b], twin[0]) and torch.equal(lse[:, a:b], twin[1]), (lname, vname, rows, s, "not the windowed kernel's bits")
                        twins += 1
            results.append((o, lse))
        _check_forward(results[0][0], results[0][1], q, k, v, lq, lk, flags, left, right, dt, "%s %s rows 128" % (lname, vname))
        if D <= 256:           # (above 256 both options run the 128-row kernel: the same launch twice)
            _check_forward(results[1][0], results[1][1], q, k, v, lq, lk, flags, left, right, dt, "%s %s rows 256" % (lname, vname))
        else:
            assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert twins >= 20         # (14 sequence / variant pairs per `rows` option have a windowed twin: the others reduce to plain or causal calls there,
                               #  have an empty side or a negative offset)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_grouped_kv_is_bit_identical_to_expanded_kv(D, dt):
    dev = _dev()
    H = 8
    lq, lk = LENSETS["cross"]
    g = torch.Generator(device="cpu").manual_seed(D + 2)
    q = _rand((sum(lq), H, D), dt, g).to(dev)
    cq, ck = _cu(lq, dev), _cu(lk, dev)
    for Hkv in (H, H // 4, 1):
        k, v = _rand((sum(lk), Hkv, D), dt, g).to(dev), _rand((sum(lk), Hkv, D), dt, g).to(dev)
        ke, ve = (t.repeat_interleave(H // Hkv, dim=1).contiguous() for t in (k, v))
        for flags, left, right in (VARIANTS["causal_br"], VARIANTS["band_br"], VARIANTS["plain"]):
            a = _fwd_varlen(q, k, v, cq, ck, max(lq), max(lk), flags, left, right)
            b = _fwd_varlen(q, ke, ve, cq, ck, max(lq), max(lk), flags, left, right)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (Hkv, flags)
            assert torch.isfinite(a[0]).all()
    # grouped results against the oracle once (Hkv = 2)
    qc = q.cpu()
    k, v = _rand((sum(lk), 2, D), dt, g), _rand((sum(lk), 2, D), dt, g)
    flags, left, right = VARIANTS["causal_br"]
    o, lse = _fwd_varlen(q, k.to(dev), v.to(dev), cq, ck, max(lq), max(lk), flags, left, right)
    _check_forward(o, lse, qc, k, v, lq, lk, flags, left, right, dt, "grouped")


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_equal_lengths_are_the_batched_windowed_call_bit_for_bit(D, dt):
    """B sequences of one length: the packed call equals fa2_fwd_window on the same memory read as [B, N, H, D]."""
    dev = _dev()
    lib = _fa2_lib.load()
    B, H, Hkv, N = 3, 4, 2, 700
    g = torch.Generator(device="cpu").manual_seed(D + 3)
    q, k, v = _rand((B * N, H, D), dt, g).to(dev), _rand((B * N, Hkv, D), dt, g).to(dev), _rand((B * N, Hkv, D), dt, g).to(dev)
    cu = _cu([N] * B, dev)
    for rows in (128, 256):
        for flags, left, right in ((0, 100, 0), (CAUSAL, 200, -1), (0, 64, 64)):
            with _fa2_lib.options(rows=rows):
                o, lse = _fwd_varlen(q, k, v, cu, cu, N, N, flags, left, right)
                q4, k4, v4 = q.view(B, N, H, D), k.view(B, N, Hkv, D), v.view(B, N, Hkv, D)
                o4 = torch.full_like(q4, float("nan"))
                lse4 = torch.full((B, H, N), float("nan"), dtype=torch.float32, device=dev)

                def s3(t):
                    return _fa2_lib.strides3(t.stride(0), t.stride(2), t.stride(1))
                _fa2_lib.check(lib.fa2_fwd_window(_code(dt), q4.data_ptr(), k4.data_ptr(), v4.data_ptr(), o4.data_ptr(), lse4.data_ptr(), B, H, Hkv, N, N, D, s3(q4),
                                                  s3(k4), s3(v4), s3(o4), _fa2_lib.strides2(H * N, N), D ** -0.5, flags, left, right, 0, _stream()))
                torch.cuda.synchronize()
            assert torch.equal(o.view(B, N, H, D), o4), (rows, flags, left, right)
            assert torch.equal(lse.view(H, B, N).transpose(0, 1), lse4), (rows, flags, left, right)


def _backward_reference(q, k, v, do, lq, lk, flags, left, right, code):
    """Per sequence: (oracle dq, dk, dv as f32; float64 dq, dk, dv; dead rows; dead keys), None for a sequence with an empty side."""
    cq, ck = np.concatenate([[0], np.cumsum(lq)]), np.concatenate([[0], np.cumsum(lk)])
    out = []
    for s, (nq, nk) in enumerate(zip(lq, lk)):
        if nq == 0 or nk == 0:
            out.append(None)
            continue
        keep = _keep(nq, nk, flags, left, right)
        bias = np.where(keep, 0.0, -np.inf).astype(np.float32)
        qs, ks, vs, gs = _seq(q, cq, s), _seq(k, ck, s), _seq(v, ck, s), _seq(do, cq, s)
        o_bits, lse_ref = fo.fwd_c(_bits(qs), _bits(ks), _bits(vs), code, False, bias=bias)
        want = [fo.bits_to_f32(b, code) for b in fo.bwd_c(_bits(qs), _bits(ks), _bits(vs), o_bits, _bits(gs), lse_ref, code, False, bias=bias)]
        truth = fo.bwd_numpy(qs.float().numpy(), ks.float().numpy(), vs.float().numpy(), gs.float().numpy(), False, bias=bias)
        out.append((want, truth, ~keep.any(1), ~keep.any(0)))
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128, 256, 512])       # the fused pass, the wave-pair pass, the separate passes, the slab pass
def test_backward_against_oracle_and_float64(D, dt):
    dev = _dev()
    code = _code(dt)
    H = 2
    for (lname, (lq, lk)), (vname, (flags, left, right)) in [(a, b) for a in LENSETS.items() for b in VARIANTS.items()]:
        g = torch.Generator(device="cpu").manual_seed(D + len(vname) + 5 * len(lname))
        q, k, v, do = (_rand((n, H, D), dt, g) for n in (sum(lq), sum(lk), sum(lk), sum(lq)))
        qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
        cq, ck = _cu(lq, dev), _cu(lk, dev)
        o, lse = _fwd_varlen(qd, kd, vd, cq, ck, max(lq), max(lk), flags | EXACT, left, right)
        grads = _bwd_varlen(qd, kd, vd, o, dod, lse, cq, ck, max(lq), max(lk), flags, left, right)
        refs = _backward_reference(q, k, v, do, lq, lk, flags, left, right, code)
        cqn, ckn = cq.cpu().numpy(), ck.cpu().numpy()
        worst = {}
        for name, got_t, idx in zip(("dq", "dk", "dv"), grads, (0, 1, 2)):
            assert torch.isfinite(got_t).all(), (lname, vname, name, "pre-filled with NaN: every element must be written")
            cu = cqn if name == "dq" else ckn
            for s, ref in enumerate(refs):
                got = got_t[int(cu[s]):int(cu[s + 1])].float().cpu().transpose(0, 1).unsqueeze(0).numpy()
                if ref is None:          # no queries: dK / dV of its keys are zero; no keys: dQ of its rows is zero
                    assert np.all(got == 0.0), (lname, vname, name, s, "a sequence with an empty side")
                    continue
                w, t64 = ref[0][idx], ref[1][idx]
                e_o, e_t, ref_t = np.abs(got - w).max(), np.abs(got - t64).max(), np.abs(w - t64).max()
                worst[name] = max(worst.get(name, (0.0, 0.0)), (float(e_o), float(e_t)))
                assert e_o <= GRAD_TOL[code] * max(1.0, np.abs(w).max()), (lname, vname, name, s, "oracle", float(e_o))
                assert e_t <= max(2 * ref_t, GRAD_TOL[code] * max(1.0, np.abs(t64).max())), (lname, vname, name, s, "float64", float(e_t))
                dead = ref[2] if name == "dq" else ref[3]
                if dead.any():
                    assert np.all(got[:, :, dead] == 0.0), (lname, vname, name, s, "rows / keys nobody sees")
        print("%s %s: (vs oracle, vs float64) %s" % (lname, vname, worst))


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_a_neighbours_nan_stays_out(D, dt):
    """(i) One sequence's K and V are NaN: every other sequence's O / LSE / dQ / dK / dV is bit-identical to the clean run."""
    dev = _dev()
    H = 2
    lq, lk = (130, 65, 300, 64, 200), (100, 65, 257, 1, 333)
    poisoned = 2
    cq, ck = _cu(lq, dev), _cu(lk, dev)
    g = torch.Generator(device="cpu").manual_seed(D + 4)
    q, k, v, do = (_rand((n, H, D), dt, g).to(dev) for n in (sum(lq), sum(lk), sum(lk), sum(lq)))
    kp, vp = k.clone(), v.clone()
    kp[int(ck[poisoned]):int(ck[poisoned + 1])] = float("nan")
    vp[int(ck[poisoned]):int(ck[poisoned + 1])] = float("nan")
    for flags, left, right in (VARIANTS["plain"], VARIANTS["causal_br"], VARIANTS["band_br"]):
        runs = []
        for kk, vv in ((k, v), (kp, vp)):
            o, lse = _fwd_varlen(q, kk, vv, cq, ck, max(lq), max(lk), flags, left, right)
            runs.append((o, lse) + _bwd_varlen(q, kk, vv, o, do, lse, cq, ck, max(lq), max(lk), flags, left, right))
        for s in range(len(lq)):
            if s == poisoned:
                continue
            a, b, c, d = int(cq[s]), int(cq[s + 1]), int(ck[s]), int(ck[s + 1])
            clean, dirty = runs
            assert torch.equal(clean[0][a:b], dirty[0][a:b]) and torch.equal(clean[1][:, a:b], dirty[1][:, a:b]), (flags, s, "forward")
            assert torch.equal(clean[2][a:b], dirty[2][a:b]), (flags, s, "dq")
            assert torch.equal(clean[3][c:d], dirty[3][c:d]) and torch.equal(clean[4][c:d], dirty[4][c:d]), (flags, s, "dk / dv")
            assert torch.isfinite(dirty[0][a:b]).all() and torch.isfinite(dirty[2][a:b]).all() and torch.isfinite(dirty[3][c:d]).all()


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128, 256, 512])
def test_rows_beyond_the_last_boundary_are_neither_read_nor_written(D, dt):
    """(ii) B = 1 on buffers that hold two sequences: the second sequence's rows of o, lse, dq, dk, dv stay the NaN they were filled with, and nothing
    is read from it (its q / k / v / dout are NaN; the first sequence's results are those of the two-sequence call)."""
    dev = _dev()
    H = 2
    lq, lk = (200, 190), (333, 100)
    cq, ck = _cu(lq, dev), _cu(lk, dev)
    g = torch.Generator(device="cpu").manual_seed(D + 5)
    q, k, v, do = (_rand((n, H, D), dt, g).to(dev) for n in (sum(lq), sum(lk), sum(lk), sum(lq)))
    for flags, left, right in (VARIANTS["plain"], VARIANTS["band_br"]):
        o2, lse2 = _fwd_varlen(q, k, v, cq, ck, max(lq), max(lk), flags, left, right)
        g2 = _bwd_varlen(q, k, v, o2, do, lse2, cq, ck, max(lq), max(lk), flags, left, right)
        qn, kn, vn, don = q.clone(), k.clone(), v.clone(), do.clone()
        qn[lq[0]:], don[lq[0]:], kn[lk[0]:], vn[lk[0]:] = float("nan"), float("nan"), float("nan"), float("nan")
        o1, lse1 = _fwd_varlen(qn, kn, vn, cq[:2].contiguous(), ck[:2].contiguous(), max(lq), max(lk), flags, left, right, B=1)
        on = o1.clone()
        on[lq[0]:] = 0             # (a stand-in for the forward's output there: the backward must not read it either)
        g1 = _bwd_varlen(qn, kn, vn, on, don, lse1, cq[:2].contiguous(), ck[:2].contiguous(), max(lq), max(lk), flags, left, right, B=1)
        assert torch.equal(o1[:lq[0]], o2[:lq[0]]) and torch.equal(lse1[:, :lq[0]], lse2[:, :lq[0]])
        assert torch.isnan(o1[lq[0]:]).all() and torch.isnan(lse1[:, lq[0]:]).all()
        for a, b, n in zip(g1, g2, (lq[0], lk[0], lk[0])):
            assert torch.equal(a[:n], b[:n]) and torch.isfinite(a[:n]).all()
            assert torch.isnan(a[n:]).all()


def _dense_f32(q, k, v, keep, g):
    ke, ve = (t.repeat_interleave(g, dim=1) for t in (k, v))
    s = (q.float() @ ke.float().transpose(-1, -2)) * q.shape[-1] ** -0.5
    s = s.masked_fill(~keep, float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.where(keep.any(-1, keepdim=True), p, torch.zeros_like(p))
    return p @ ve.float()


@pytest.mark.parametrize("Hkv", [4, 1])
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_operator_matches_the_masked_path_and_a_dense_reference(dt, Hkv):
    """flash_attention_varlen with grouped K / V through autograd, against flash_attention(mask=...) on the padded batch and an f32 dense reference
    (the pattern of test_operator_matches_the_masked_path_and_sdpa); the no-grad forward is bit-identical to the differentiated call's."""
    dev = _dev()
    code = _code(dt)
    H, D = 4, 64
    lq, lk = (150, 0, 300, 64, 33), (200, 64, 120, 0, 33)
    B, mq, mk = len(lq), max(lq), max(lk)
    cq, ck = _cu(lq, dev), _cu(lk, dev)
    for kw in (dict(), dict(causal=True), dict(causal=True, bottom_right=True), dict(window=(40, 0)), dict(window=(30, 20), bottom_right=True)):
        left, right, _ = _fa2_lib.parse_window(kw.get("window"), 0)
        flags = (CAUSAL if kw.get("causal") else 0) | (BR if kw.get("bottom_right") else 0)
        g = torch.Generator(device="cpu").manual_seed(Hkv + len(kw))
        q, k, v, do = (_rand((n, h, D), dt, g).to(dev) for n, h in ((sum(lq), H), (sum(lk), Hkv), (sum(lk), Hkv), (sum(lq), H)))
        # the padded batch [B, H, max, D] and its keep-mask [B, 1, mq, mk]: the band of each sequence over its own keys
        qp, kp, vp, dop = (torch.zeros((B, h, n, D), dtype=dt, device=dev) for h, n in ((H, mq), (Hkv, mk), (Hkv, mk), (H, mq)))
        keep = torch.zeros((B, 1, mq, mk), dtype=torch.bool, device=dev)
        for s in range(B):
            a, b, c, d = int(cq[s]), int(cq[s + 1]), int(ck[s]), int(ck[s + 1])
            qp[s, :, :lq[s]], dop[s, :, :lq[s]] = q[a:b].transpose(0, 1), do[a:b].transpose(0, 1)
            kp[s, :, :lk[s]], vp[s, :, :lk[s]] = k[c:d].transpose(0, 1), v[c:d].transpose(0, 1)
            keep[s, 0, :lq[s], :lk[s]] = torch.from_numpy(_keep(lq[s], lk[s], flags, left, right)).to(dev)

        def unpad(t, lens, cu):
            return torch.cat([t[s, :, :lens[s]].transpose(0, 1) for s in range(B)], 0)
        qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
        o = flash_attention_varlen(qq, kk, vv, cq, ck, mq, mk, **kw)
        o.backward(do)
        mine = (o.detach(), qq.grad, kk.grad, vv.grad)
        qm, km, vm = (t.clone().requires_grad_(True) for t in (qp, kp, vp))
        om = flash_attention(qm, km, vm, mask=keep)
        om.backward(dop)
        masked = (unpad(om.detach(), lq, cq), unpad(qm.grad, lq, cq), unpad(km.grad, lk, ck), unpad(vm.grad, lk, ck))
        qf, kf, vf = (t.clone().float().requires_grad_(True) for t in (qp, kp, vp))
        ref = _dense_f32(qf, kf, vf, keep, H // Hkv)
        ref.backward(dop.float())
        dense = (unpad(ref.detach(), lq, cq), unpad(qf.grad, lq, cq), unpad(kf.grad, lk, ck), unpad(vf.grad, lk, ck))
        torch.cuda.synchronize()
        with torch.no_grad():
            o_ng = flash_attention_varlen(q, k, v, cq, ck, mq, mk, **kw)
            o_sync = flash_attention_varlen(q, k, v, cq, ck, **kw)                  # the maxima computed from the tensors
        assert torch.equal(o_ng, mine[0]) and torch.equal(o_sync, mine[0]), kw
        tol_o, tol_g = 2 * FLOOR[code], GRAD_TOL[code]
        for name, a, b, r in zip(("o", "dq", "dk", "dv"), mine, masked, dense):
            tol = tol_o if name == "o" else tol_g * max(1.0, r.abs().max().item())
            assert a.shape == r.shape and torch.isfinite(a).all(), (name, kw)
            assert (a.float() - b.float()).abs().max().item() <= tol, (name, "masked path", kw, (a.float() - b.float()).abs().max().item())
            assert (a.float() - r).abs().max().item() <= tol, (name, "dense", kw, (a.float() - r).abs().max().item())


def test_operator_pads_odd_head_dims_and_takes_strided_inputs():
    dev = _dev()
    lq = (70, 0, 130)
    cu = _cu(lq, dev)
    g = torch.Generator(device="cpu").manual_seed(11)
    qkv = _rand((sum(lq), 3, 4, 64), torch.float16, g).to(dev)                         # a fused QKV projection: strided views
    q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]
    a = flash_attention_varlen(q, k, v, cu, cu, causal=True)
    b = flash_attention_varlen(q.contiguous(), k.contiguous(), v.contiguous(), cu, cu, 130, 130, causal=True)
    assert torch.equal(a, b)
    q36 = _rand((sum(lq), 2, 36), torch.float16, g).to(dev).requires_grad_(True)       # D = 36: padded to 40 by the operator
    o = flash_attention_varlen(q36, q36.detach(), q36.detach(), cu, cu)
    assert o.shape == q36.shape
    o.sum().backward()
    assert q36.grad.shape == q36.shape and torch.isfinite(q36.grad).all()
    ref = torch.cat([torch.nn.functional.scaled_dot_product_attention(*(3 * [q36.detach()[int(cu[s]):int(cu[s + 1])].transpose(0, 1).float()])).transpose(0, 1)
                     for s in range(len(lq)) if lq[s]], 0)
    assert (o.float() - ref).abs().max().item() <= 2 * FLOOR[0]
