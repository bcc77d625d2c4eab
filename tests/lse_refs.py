"""References shared by tests/test_lse_gpu.py and tests/test_merge_gpu.py (a helper module like far_layouts.py, not a test file).

truth64: dense float64 autograd of the contract with the LSE as a second output — loss = (O * dO).sum() + (lse_live * u).sum(), lse in natural-log
units, u the caller's weights; every route of flash_attention goes through the same few lines: scaled scores, soft-capping, ALiBi, an additive bias,
a keep mask (bool mask and band) as -inf, dropout applied to the probabilities (the LSE is that of the undropped ones).
emulate: the same contract as the kernels run it — f32 scores and sums, P rounded to the I/O dtype, dS (1 - t^2) rounded to the I/O dtype, outputs
rounded once — with the dQ pass's row term delta - u.
Bars: the project's rule (tools/fuzz_features.py: error_and_bar; FLOOR / GRAD_TOL / LSE_TOL of conftest.py); the LSE is compared in log2 units."""
import importlib.util
import math
import os

import torch

from conftest import FLOOR, GRAD_TOL, LSE_TOL

LN2 = math.log(2.0)
NAMES = ("O", "lse", "dQ", "dK", "dV")

_spec = importlib.util.spec_from_file_location("_fuzz_features", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "tools", "fuzz_features.py"))
ff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ff)


def code(dt):
    return 0 if dt == torch.float16 else 1


def _scores(q, k, scale, softcap, slopes, off, bias, allow):
    """-> (S with -inf where not allowed, d S / d x of the soft-capping, dead rows [H, Nq])."""
    S = (q @ k.transpose(-1, -2)) * scale
    fac = torch.ones_like(S)
    if softcap > 0:
        t = torch.tanh(S / softcap)
        S, fac = softcap * t, 1.0 - t * t
    if slopes is not None:
        dist = (torch.arange(q.shape[1], device=q.device).unsqueeze(1) + off - torch.arange(k.shape[1], device=q.device).unsqueeze(0)).abs()
        S = S - slopes.to(S.dtype).to(q.device)[:, None, None] * dist.to(S.dtype)
    if bias is not None:
        S = S + bias.to(S.dtype)
    S = S.masked_fill(~allow, float("-inf"))
    return S, fac, torch.isneginf(S).all(-1)


def truth64(q, k, v, do, u, allow, scale, softcap=0.0, slopes=None, off=0, bias=None, keep=None, rs=1.0):
    """[H, Nq, D] q, do; [H, Nkv, D] k, v (grouped k / v already expanded); u [H, Nq] (None: no LSE term); allow: bool, broadcastable to [H, Nq, Nkv].
    -> dict O, lse (log2 units, -inf on dead rows), dQ, dK, dV."""
    q, k, v = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    S, _, dead = _scores(q, k, scale, softcap, slopes, off, None if bias is None else bias.double(), allow)
    Ssafe = S.masked_fill(dead.unsqueeze(-1), 0.0)
    lse = torch.logsumexp(Ssafe, -1)
    P = torch.exp(Ssafe - lse.unsqueeze(-1)).masked_fill(dead.unsqueeze(-1), 0.0)
    O = (P if keep is None else P * keep * rs) @ v
    loss = (O * do.double()).sum()
    if u is not None:
        loss = loss + (lse * u.double()).masked_fill(dead, 0.0).sum()
    loss.backward()
    return dict(O=O.detach(), lse=(lse.detach() / LN2).masked_fill(dead, float("-inf")), dQ=q.grad, dK=k.grad, dV=v.grad)


def emulate(q, k, v, do, u, allow, scale, dt, softcap=0.0, slopes=None, off=0, bias=None, keep=None, rs=1.0):
    qf, kf, vf, gf = q.float(), k.float(), v.float(), do.float()
    S, fac, dead = _scores(qf, kf, scale, softcap, slopes, off, None if bias is None else bias.float(), allow)
    m = S.max(-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    E = torch.exp(S - m)
    l = E.sum(-1, keepdim=True)
    l1 = torch.where(l > 0, l, torch.ones_like(l))
    rs = torch.tensor(rs, dtype=torch.float32).item()
    kf32 = torch.ones_like(S) if keep is None else keep.float()
    O = (((E.to(dt).float() * kf32) @ vf) / l1 * rs).to(dt)
    Pn = E / l1
    dV = (((Pn.to(dt).float() * kf32).transpose(-1, -2) @ gf) * rs).to(dt)
    dP = (gf @ vf.transpose(-1, -2)) * kf32 * rs
    delta = (gf * O.float()).sum(-1, keepdim=True)
    if u is not None:
        delta = delta - u.float().masked_fill(dead, 0.0).unsqueeze(-1)
    dX = (Pn * (dP - delta) * fac).to(dt).float()
    dQ = ((dX @ kf) * scale).to(dt)
    dK = ((dX.transpose(-1, -2) @ qf) * scale).to(dt)
    lse = ((m + torch.log(l)) / LN2).squeeze(-1).masked_fill(dead, float("-inf"))
    return dict(O=O.double(), lse=lse.double(), dQ=dQ.double(), dK=dK.double(), dV=dV.double())


def fold(t, hkv):
    return t.unflatten(0, (hkv, t.shape[0] // hkv)).sum(1)


def bars_of(true, emu, dt):
    """name -> (bar, err_emu): max(2 * err_emu, tol * max(1, max|true|)); the LSE (log2 units): max(LSE_TOL, 2 * err_emu)."""
    out = {}
    for n in NAMES:
        if n == "lse":
            live = ~torch.isinf(true["lse"])
            e = (emu["lse"][live] - true["lse"][live]).abs().max().item() if live.any() else 0.0
            out[n] = (max(LSE_TOL, 2 * e), e)
        else:
            _, e, bar = ff.error_and_bar(emu[n], true[n], emu[n], FLOOR[code(dt)] if n == "O" else GRAD_TOL[code(dt)])
            out[n] = (bar, e)
    return out


def check(tag, got, true, bars, names=NAMES):
    """got: name -> tensor (lse in log2 units).  Prints every figure before it asserts."""
    for n in names:
        bar, e_emu = bars[n]
        x, t = got[n].double(), true[n]
        if n == "lse":
            dead = torch.isinf(t)
            assert torch.isneginf(got[n][dead]).all(), (tag, "rows that see no key: lse = -inf exactly")
            x, t = x[~dead], t[~dead]
        assert torch.isfinite(x).all(), (tag, n, "non-finite")
        err = (x - t).abs().max().item() if x.numel() else 0.0
        print("%s %s: err %.3g, emulation %.3g, bar %.3g" % (tag, n, err, e_emu, bar))
        assert err <= bar, (tag, n, err, bar)


def check_not_vacuous(tag, true, without_u, bars):
    """The u term must move the float64 dQ and dK by at least 5 bars (dV does not depend on dlse)."""
    for n in ("dQ", "dK"):
        mg = (true[n] - without_u[n]).abs().max().item() / bars[n][0]
        print("%s %s: the LSE term moves it by %.1f bars" % (tag, n, mg))
        assert mg >= 5.0, (tag, n, mg)
    assert (true["dV"] - without_u["dV"]).abs().max().item() <= 1e-9 * max(1.0, true["dV"].abs().max().item())


def merge64(outs, lses):
    """float64 merge of parts: outs [..., D], lses [...] natural-log -> (out, lse); all -inf rows give zeros and -inf."""
    L = torch.stack([l.double() for l in lses])
    O = torch.stack([o.double() for o in outs])
    m = L.max(0).values
    dead = torch.isneginf(m)
    w = torch.exp(L - torch.where(dead, torch.zeros_like(m), m))
    s = w.sum(0)
    w = w / torch.where(dead, torch.ones_like(s), s)
    O = torch.where(w.unsqueeze(-1) > 0, O, torch.zeros_like(O))          # a part of weight 0 may hold anything
    return (w.unsqueeze(-1) * O).sum(0), torch.where(dead, m, m + torch.log(torch.where(dead, torch.ones_like(s), s)))


MERGE_EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}          # half an ulp at 1: one round-to-nearest of the I/O dtype


def merge_check(tag, dt, natural, outs, lses, dout, dlse, out, lse, dos, dls):
    """fa2_merge_fwd / fa2_merge_bwd against the float64 merge and its autograd.  Everything as [B, H, N, D] / [B, H, N] views: the parts, dO, dlse
    (the LSEs' unit, natural-log or log2), the merged out / lse and the parts' gradients.  Bars: one rounding of the I/O dtype at the largest
    magnitude for out and dO_k, LSE_TOL in log2 units for the LSE, 1e-4 relative for dlse_k (f32 dot products over D against float64).  Rows whose
    LSE is -inf in a part have weight 0 there: whatever that part's O holds is replaced by zeros on the way in (the kernel does not read it)."""
    nq, nparts = outs[0].shape[2], len(outs)
    unit = 1.0 if natural else LN2                                         # the LSEs' unit in natural-log units
    lin = [(l.double() * unit).requires_grad_(True) for l in lses]
    oin = [torch.where(torch.isneginf(l).unsqueeze(-1), torch.zeros_like(o), o).double().requires_grad_(True) for o, l in zip(outs, lses)]
    O64, L64 = merge64(oin, lin)
    dead = torch.isneginf(L64.detach())
    ((O64 * dout.double()).sum() + (L64.masked_fill(dead, 0.0) * (dlse.double() / unit)).masked_fill(dead, 0.0).sum()).backward()
    O64, L64 = O64.detach(), L64.detach()
    # forward: f32 accumulation of <= 16 weighted 16-bit values, rounded once
    lse2 = lse.double() * unit / LN2
    bar_o = 2 * MERGE_EPS[dt] * max(1.0, O64.abs().max().item())
    err_o = (out.double() - O64).abs().max().item()
    assert nq == 1 or dead[:, :, 0].all(), "row 0 of the case is dead"
    assert torch.isneginf(lse2[dead]).all() and (out[dead] == 0).all(), (tag, "dead rows: O = 0, lse = -inf")
    err_l = (lse2[~dead] - L64[~dead] / LN2).abs().max().item() if (~dead).any() else 0.0
    print("%s: O err %.3g (bar %.3g), lse err %.3g log2 units (bar %.3g)" % (tag, err_o, bar_o, err_l, LSE_TOL))
    assert err_o <= bar_o and err_l <= LSE_TOL, (tag, err_o, bar_o, err_l)
    if nparts == 1:
        assert torch.equal(out[~dead], outs[0][~dead]), "one part: its rows come back bit for bit"
    # backward: dO_k = w_k dO rounded once; dlse_k in the LSEs' unit
    for kx in range(nparts):
        want, wl = oin[kx].grad, lin[kx].grad * unit
        bar = 2 * MERGE_EPS[dt] * max(1.0, want.abs().max().item())
        err = (dos[kx].double() - want).abs().max().item()
        bar_l = 1e-4 * max(1.0, wl.abs().max().item())
        err_lk = (dls[kx].double() - wl).abs().max().item()
        assert torch.isfinite(dos[kx].float()).all() and torch.isfinite(dls[kx]).all(), (tag, kx, "non-finite gradient")
        assert err <= bar and err_lk <= bar_l, (tag, kx, err, bar, err_lk, bar_l)
        zero_w = torch.isneginf(lses[kx])
        assert (dls[kx][zero_w] == 0).all() and (dos[kx][zero_w] == 0).all(), (tag, kx, "zero-weight parts get zeros")
