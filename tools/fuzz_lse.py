"""Randomised float64 sweep of the score-modifier, LSE-gradient and merge calls (developer tool; the committed output lives under profiles/).

tools/fuzz_features.py draws window / packed / grouped / dropout calls; this tool draws what came after it, on that tool's draws, layouts, input builders
and bar rule.  Four families (--mode, draw_case's `force`):
    scoremod   flash_attention / flash_attention_varlen with softcap and / or alibi_slopes ([H], [B, H] / [num_sequences, H], a strided view of the
               latter; geometric, negative, zero and mixed-sign values), input amplitudes that saturate the cap or stay in its linear part
    lse        return_lse=True on every route (plain, causal, grouped, mask=, window / q_offset, dropout, softcap / ALiBi, BNHD, packed in both
               alignments), loss = (out * dO).sum() + (lse * u).sum() over live rows; u ~ N(0, 1), absent, or the only term; NaN on dead rows
    merge      fa2_merge_fwd / fa2_merge_bwd through the C-ABI (1 .. 16 parts, both LSE units, row-padded and head-sliced parts) and merge_attention
               (up to 40 parts, parts of different strides); LSE spreads of 0 / 40 / 300 log2 units, NaN / inf under every weight of exactly 0
    chain      the KV axis cut into 2 .. 6 chunks, one flash_attention(return_lse=True, q_offset = off - chunk start) per chunk, merge_attention, the
               gradient through the merge and every part, against float64 attention over the whole axis
The float64 truth (truth64, merge64) and the same-contract emulation (emulate, merge_emulate) live here; tests/lse_refs.py re-exports them to the
fixed-shape tests.  Bars: fuzz_features.error_and_bar with FLOOR / GRAD_TOL, the LSE max(LSE_TOL, 2 err_emu) in log2 units (every call of these
families is flagged FA2_FLAG_EXACT_SCALE: contract 0); merge calls: merge_check.  Dead rows give O = dQ = 0 and LSE = -inf exactly, everything is finite,
every fourth case runs twice and must repeat bit for bit.  Each scoremod case states, from float64 alone, by how many bars the modifiers move an
output, each lse case with a u the same for u: a case that moves nothing by QUIET_BARS bars is "quiet" — reported, and capped at a quarter of a slice.

The draw (draw_case, pure Python) is separate from the run (run_case); tests/test_fuzz_lse.py checks the draw's coverage and the checker's power on
the CPU.

    python tools/fuzz_lse.py --mode scoremod --cases 1000 --seed 1 [--bwd-every 2] [--long] [--out FILE]
"""
import argparse
import ctypes
import json
import math
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
for _p in (os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import fuzz_features as ff  # noqa: E402 - the draws, layouts, input builders, band, keep mask and the bar rule
import fuzz_parity as fzp  # noqa: E402
from rocwmma_fattn import _fa2_lib  # noqa: E402

LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
FLOOR, GRAD_TOL = ff.FLOOR, ff.GRAD_TOL                 # tests/conftest.py's, by dtype
LSE_TOL = 1e-3                                          # tests/conftest.py's (tests/lse_refs.py asserts they agree)
NAMES = ("O", "lse", "dQ", "dK", "dV")
MODES = ("scoremod", "lse", "merge", "chain")
SOFTCAPS = [0.0, 0.5, 1.0, 30.0, 50.0, 1e4]
SLOPE_SHAPES = [None, "H", "BH", "BH_view"]
SLOPE_VALUES = ["geometric", "negative", "zero", "mixed"]
MASK_KINDS = [("bool", "b1qk"), ("float", "1hqk"), ("bool", "b11k"), ("float", "b1qk"), ("bool", "1hqk"), ("float", "b11k")]
QUIET_BARS = 5.0                                        # the fixed-shape tests' non-vacuity threshold (lse_refs.check_not_vacuous)
QUIET_CAP = 0.25
ZERO_GAP = 200.0                                        # log2 units below the row's largest LSE: 2^-200 is exactly 0 in f32 (and no denormal)


# ---------------------------------------------------------------------------------------------------------------- the references
def _scores(q, k, scale, softcap, slopes, off, bias, allow, mut=()):
    """-> (S with -inf where not allowed, d S / d x of the soft-capping, dead rows [H, Nq]).  mut: names of deliberate errors (the CPU tests' mutants)."""
    S = (q @ k.transpose(-1, -2)) * scale
    fac = torch.ones_like(S)
    if "cap_after_mask" in mut:
        S = S.masked_fill(~allow, float("-inf"))
    if softcap > 0:
        t = torch.tanh(S / softcap)
        S, fac = softcap * t, 1.0 - t * t
    if "no_fac" in mut:
        fac = torch.ones_like(S)
    if slopes is not None:
        dist = (torch.arange(q.shape[1], device=q.device).unsqueeze(1) + off - torch.arange(k.shape[1], device=q.device).unsqueeze(0)).abs()
        S = S - slopes.to(S.dtype).to(q.device)[:, None, None] * dist.to(S.dtype)
    if bias is not None:
        S = S + bias.to(S.dtype)
    if "cap_after_mask" not in mut:
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


def emulate(q, k, v, do, u, allow, scale, dt, softcap=0.0, slopes=None, off=0, bias=None, keep=None, rs=1.0, mut=()):
    qf, kf, vf, gf = q.float(), k.float(), v.float(), do.float()
    S, fac, dead = _scores(qf, kf, scale, softcap, slopes, off, None if bias is None else bias.float(), allow, mut)
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
        delta = delta - (u.float() if "dlse_dead" in mut else u.float().masked_fill(dead, 0.0)).unsqueeze(-1)
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
            _, e, bar = ff.error_and_bar(emu[n], true[n], emu[n], FLOOR[dt] if n == "O" else GRAD_TOL[dt])
            out[n] = (bar, e)
    return out


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


def merge_emulate(outs, lses, dout, dlse, natural, dt, mut=()):
    """The merge kernels' arithmetic in torch (csrc/merge_hip.cpp): differences of LSEs in their own unit, f32 weights 2^((lse_k - m) * unit), parts of
    weight exactly 0 not read, out rounded once; the backward's weights 2^((lse_k - lse) * unit).  [..., N, D] parts, [..., N] LSEs in their own unit
    -> (out, lse, dO parts, dlse parts)."""
    in_unit = LOG2E if (natural or "natural_weights" in mut) else 1.0
    out_unit, dot_unit = (LN2, 1.0) if natural else (1.0, LN2)
    n = len(outs)
    ls = torch.stack([lses[(k + 1) % n if "next_lse" in mut else k].float() for k in range(n)])
    xs = torch.stack([o.float() for o in outs])
    m = ls.max(0).values
    dead = torch.isneginf(m)
    w = torch.exp2((ls - torch.where(dead, torch.zeros_like(m), m)) * in_unit)
    xs0 = torch.where((w != 0).unsqueeze(-1), xs, torch.zeros_like(xs))
    s = w.sum(0)
    s1 = torch.where(dead, torch.ones_like(s), s)
    out = ((w.unsqueeze(-1) * xs0).sum(0) / s1.unsqueeze(-1)).to(dt)
    lse = torch.where(dead, m, m + torch.log2(s1) * out_unit)
    wb = torch.exp2((ls - torch.where(dead, torch.zeros_like(lse), lse)) * in_unit)
    wb = torch.where(dead.unsqueeze(0), torch.zeros_like(wb), wb)
    xb = torch.where((wb != 0).unsqueeze(-1), xs, torch.zeros_like(xs))
    g = dout.float()
    d = (g.unsqueeze(0) * xb).sum(-1)
    dot_o = (wb * d).sum(0)
    gl = torch.zeros_like(m) if dlse is None else torch.where(dead, torch.zeros_like(m), dlse.float())
    dterm = torch.zeros_like(d) if "no_dot_term" in mut else dot_unit * (d - dot_o)
    dls = wb * (gl + dterm)
    dos = (wb.unsqueeze(-1) * g.unsqueeze(0)).to(dt)
    return out, lse, list(dos), list(dls)


# ---------------------------------------------------------------------------------------------------------------- the draw (pure Python)
_SPLIT_NKV = {}


def kv_split_nkv(H, Nq):
    """The smallest Nkv for which fa2_bwd_workspace_bytes reports a KV-split dQ pass for B1, H heads, D 64 (bf16, non-causal), read from the library."""
    if (H, Nq) not in _SPLIT_NKV:
        lib = _fa2_lib.load()
        n = next(n for n in range(64, 1 << 16, 64) if lib.fa2_bwd_workspace_bytes(1, 1, H, Nq, n, 64, 0) > 0)
        while n > 1 and lib.fa2_bwd_workspace_bytes(1, 1, H, Nq, n - 1, 64, 0) > 0:
            n -= 1
        _SPLIT_NKV[(H, Nq)] = n
    return _SPLIT_NKV[(H, Nq)]


def _nmax(D, long):
    return (300 if D > 256 else 700) if not long else (300 if D > 256 else 700 if D > 128 else 1500)


def _draw_len(rng, D, long):
    nmax = _nmax(D, long)
    return rng.choice([n for n in fzp.EDGE_LENGTHS if n <= nmax]) if rng.random() < 0.4 else rng.randint(1, nmax)


def _dense_base(i, rng, long):
    D = rng.choice(fzp.HEAD_DIMS)
    Nq, Nkv = _draw_len(rng, D, long), _draw_len(rng, D, long)
    if rng.random() < 0.3:
        Nkv = Nq
    H, Hkv = ff._draw_heads(rng)
    return dict(i=i, mode="dense", long=long, dtype=rng.choice(["float16", "bfloat16"]), D=D, B=rng.randint(1, 2), H=H, Hkv=Hkv, Nq=Nq, Nkv=Nkv,
                causal=rng.random() < 0.4, window=ff._draw_window(rng, Nkv), q_offset=rng.choice([0, max(Nkv - Nq, 0), rng.randint(0, Nkv + 70)]),
                p=0.0, seed=0, bnhd=rng.random() < 0.5, layouts=[ff._draw_layout(rng, ["contig", "bnhd_view", "rowpad", "headslice"]) for _ in range(3)],
                scale_mul=ff._draw_scale_mul(rng), dist="randn", rows=rng.choice([0, 128, 256]), bwd=False, twice=i % 4 == 0)


def _packed_base(i, rng, long):
    D = rng.choice(fzp.HEAD_DIMS)
    nseq = rng.randint(1, 5)
    one = lambda: rng.choice(ff.PACKED_LENGTHS) if rng.random() < 0.4 else rng.randint(0, 200 if D > 256 else 400)  # noqa: E731
    lens_q = [one() for _ in range(nseq)]
    lens_k = list(lens_q) if rng.random() < 0.5 else [one() for _ in range(nseq)]
    if sum(lens_q) == 0:
        lens_q[0] = lens_k[0] = 65
    H, Hkv = ff._draw_heads(rng)
    causal, bottom_right = rng.choice([(False, False), (True, False), (True, True), (False, True)])
    return dict(i=i, mode="packed", long=long, dtype=rng.choice(["float16", "bfloat16"]), D=D, H=H, Hkv=Hkv, lens_q=lens_q, lens_k=lens_k, causal=causal,
                bottom_right=bottom_right, window=ff._draw_window(rng, max(lens_k)), p=0.0, seed=0, max_kind=rng.choice(["exact", "round64", "none"]),
                layouts=[ff._draw_layout(rng, ["contig", "rowpad", "headslice"]) for _ in range(3)], surplus=rng.randint(1, 70) if rng.random() < 0.25 else 0,
                scale_mul=ff._draw_scale_mul(rng), dist="randn", rows=rng.choice([0, 128, 256]), bwd=False, twice=i % 4 == 0)


def _draw_modifiers(rng, d, force=True):
    """softcap, the slopes' shape / values / multiplier and the input amplitude.  force: at least one modifier is on."""
    cap = rng.choice(SOFTCAPS)
    shape = rng.choice(SLOPE_SHAPES)
    if force and cap == 0.0 and shape is None:
        shape = rng.choice(SLOPE_SHAPES[1:])
    if force and shape is None and cap > 50.0 and rng.random() < 0.7:          # a cap of 1e4 alone moves nothing: mostly drawn with slopes
        shape = rng.choice(SLOPE_SHAPES[1:])
    values = rng.choice(SLOPE_VALUES)
    if force and cap == 0.0 and values == "zero" and rng.random() < 0.7:       # zero slopes alone likewise
        values = rng.choice(["geometric", "negative", "mixed"])
    amp = 1.0
    if 0.0 < cap <= 50.0:      # saturated (|x| ~ amp^2 |scale_mul| = 4 softcap) or in the linear part
        amp = math.sqrt(4.0 * cap / abs(d["scale_mul"])) if rng.random() < 0.6 else min(1.0, math.sqrt(0.25 * cap / abs(d["scale_mul"])))
    d.update(softcap=cap, slopes=shape, slope_values=values, slope_mul=rng.choice([1.0, 8.0]), amp=amp)


def saturated(d):
    return d["softcap"] > 0 and d["amp"] ** 2 * abs(d["scale_mul"]) >= 3.0 * d["softcap"]


def _draw_scoremod(i, rng, long):
    d = _packed_base(i, rng, long) if rng.random() < 0.4 else _dense_base(i, rng, long)
    _draw_modifiers(rng, d)
    d.update(fam="scoremod", u="none", mask=None)
    return d


def _draw_lse(i, rng, long):
    kind = {5: "short", 11: "asm128"}.get(i % 24)           # the routes a random draw reaches rarely, at fixed places of the sequence
    if i % 36 == 17 and not long:                            # (the KV-split needs a long sweep: two cases in a slice of 72)
        kind = "split"
    packed = kind is None and rng.random() < 0.4
    d = _packed_base(i, rng, long) if packed else _dense_base(i, rng, long)
    d.update(fam="lse", softcap=0.0, slopes=None, slope_values="geometric", slope_mul=1.0, amp=2.0, mask=None, kind=kind,
             u=rng.choice(["randn", "randn", "randn", "randn", "none", "only"]), dist=rng.choice(["rand", "randn"]))
    if packed:
        route, feats = "packed", rng.sample(["window", "dropout", "smod"], rng.randint(0, 2))
        if "dropout" in feats and "smod" in feats:
            feats.remove(rng.choice(["dropout", "smod"]))
    else:
        route = rng.choice(["plain", "mask", "mask", "window", "dropout", "smod"]) if kind is None else "plain"
        feats = [route] if route in ("window", "dropout", "smod") else []
    if route == "plain":
        d["window"], d["q_offset"] = None, 0
    elif route == "packed" and "window" not in feats:
        d["window"] = None
    elif "window" in feats and d["window"] is None:
        d["window"] = [ff._window_edge(rng, 64), ff._window_edge(rng, 64)]
    if "dropout" in feats:
        d["p"], d["seed"] = ff._draw_dropout(rng, always=True)
    if "smod" in feats:
        _draw_modifiers(rng, d)
        d["amp"] = max(d["amp"], 1.0)
    if route == "mask":
        d["mask"] = list(rng.choice(MASK_KINDS)) + [rng.random() < 0.5]
        d["D"] = d["D"] if d["D"] <= 256 else rng.choice([64, 72, 128, 200, 256])          # (a masked call with gradients: head dims up to 256)
        d["Nq"], d["Nkv"] = min(d["Nq"], 513), min(d["Nkv"], 513)
    if kind == "short":
        d.update(Nkv=rng.choice([1, 31, 64, 77, 127, 128]), D=rng.choice([64, 64, 40, 128]), u="randn")
    elif kind == "asm128":
        d.update(D=128, Nq=rng.choice([256, 512]), causal=False, u="randn", rows=0, H=rng.choice([2, 4]), layouts=[["contig", 0]] * 3, bnhd=False)
        d.update(Nkv=d["Nq"], Hkv=d["H"], scale_mul=1.0)
    elif kind == "split":
        H, Nq = rng.choice([1, 2]), rng.choice([64, 200, 256])
        d.update(D=64, B=1, H=H, Hkv=H, Nq=Nq, Nkv=kv_split_nkv(H, Nq), causal=False, u="randn", dtype="bfloat16", rows=0, layouts=[["contig", 0]] * 3)
    return d


def _draw_merge(i, rng, long):
    via = "op" if i % 4 == 3 else "abi"
    nparts = rng.choice([1, 2, 3, 5, 16, 16, rng.randint(1, 16)]) if via == "abi" else rng.choice([rng.randint(17, 40), rng.randint(33, 40), rng.randint(2, 16), rng.randint(2, 16)])
    D = 8 * rng.randint(1, 64)
    layout = rng.choice(["bhnd", "bnhd", "packed"])
    strides = rng.choice(["contig", "rowpad", "headslice"])
    return dict(i=i, fam="merge", mode="merge", via=via, nparts=nparts, D=D, Nq=rng.choice(fzp.EDGE_LENGTHS[:15] + [rng.randint(1, 300)]),
                B=1 if layout == "packed" else rng.randint(1, 2), H=rng.choice(ff.HEAD_COUNTS[:5]), layout=layout, strides=strides,
                par=8 * rng.randint(1, 4) if strides == "rowpad" else rng.randint(1, 3), mixed_strides=via == "op" and nparts <= 16 and rng.random() < 0.6,
                natural=via == "op" or rng.random() < 0.5, spread=rng.choice([0, 40, 300]), dtype=rng.choice(["float16", "bfloat16"]),
                dlse=rng.random() < 0.7, dead_frac=rng.choice([0.0, 0.1, 0.3]), bwd=False, twice=i % 4 == 0)


def _draw_chain(i, rng, long):
    D = rng.choice([64, 128, 64, 128, 40, 72, 200, 256, 320])
    Nq = _draw_len(rng, D, False)
    Nkv = max(_draw_len(rng, D, False), rng.randint(130, 300))
    ncut = min(rng.randint(1, 5), Nkv - 1)
    pick = lambda: rng.randrange(64, Nkv, 64) if rng.random() < 0.3 and Nkv > 64 else rng.randint(1, Nkv - 1)  # noqa: E731
    cuts = sorted({pick() for _ in range(ncut)})
    H, Hkv = ff._draw_heads(rng, [1, 2, 4, 6])
    left = rng.choice([-1, -1, 0, 31, 63, 64, 65, rng.randint(0, Nkv)])
    window = None if left < 0 and rng.random() < 0.5 else [left, rng.choice([-1, 0, 1, 63, rng.randint(0, Nkv)])]
    d = dict(i=i, fam="chain", mode="dense", long=long, dtype=rng.choice(["float16", "bfloat16"]), D=D, B=rng.randint(1, 2), H=H, Hkv=Hkv, Nq=Nq, Nkv=Nkv,
             causal=rng.random() < 0.5, window=window, q_offset=cuts[-1] + rng.choice([0, 1, rng.randint(0, Nkv - cuts[-1] + 40)]), cuts=cuts, p=0.0, seed=0,
             bnhd=False, layouts=[["contig", 0]] * 3, scale_mul=1.0, dist="randn", rows=0, mask=None, u="randn", bwd=False, twice=i % 4 == 0)
    _draw_modifiers(rng, d, force=False)
    d["amp"] = max(d["amp"], 1.0) * (2.0 if d["softcap"] == 0.0 else 1.0)
    return d


def draw_case(i, rng, force):
    """Case i of a family as a dict that describes the call completely; force: one of MODES, or (mode, long).  Pure Python."""
    mode, long = force if isinstance(force, (tuple, list)) else (force, False)
    return {"scoremod": _draw_scoremod, "lse": _draw_lse, "merge": _draw_merge, "chain": _draw_chain}[mode](i, rng, long)


def draw_sweep(seed, counts, bwd_every=2):
    """The cases of a sweep: counts = [(force, n), ...] drawn in that order from one generator; every bwd_every-th case of a family runs the backward."""
    rng = random.Random(seed)
    out = []
    for force, n in counts:
        for j in range(n):
            d = draw_case(j, rng, force)
            d["bwd"] = bwd_every > 0 and (j % bwd_every == 0 or d.get("kind") is not None) and not (d["fam"] == "merge" and d["nparts"] > 16)
            out.append(d)
    return out


# tests/test_fuzz_lse_gpu.py: one slice per family; tests/test_fuzz_lse.py proves on the CPU that these seeds and counts reach every coverage item
SLICES = {"scoremod": (1, [("scoremod", 56)]), "lse": (9, [("lse", 72)]), "merge": (1, [("merge", 48)]), "chain": (1, [("chain", 16)])}


def parts_of(d):
    """The chunks [c0, c1) of a chain case."""
    edges = [0] + list(d["cuts"]) + [d["Nkv"]]
    return list(zip(edges[:-1], edges[1:]))


def _edge_in_tile(d):
    if d["mode"] != "dense" or d["window"] is None or d["q_offset"] <= 0:
        return False
    _, nk, l, r, off = ff.units_of(d)[0]
    return bool((l >= 0 and 0 < off - l < nk and (off - l) % 64) or (r >= 0 and off + r + 1 < nk and (off + r + 1) % 64))


def _chain_dead_part(d):
    """A chunk no row of which sees a key of it."""
    nq, nk, l, r, off = ff.units_of(d)[0]
    for c0, c1 in parts_of(d):
        lo = 0 if l < 0 else off - l                       # the first key row 0 sees; the last key the last row sees
        hi = nk - 1 if r < 0 else nq - 1 + off + r
        if lo >= c1 or hi < c0:
            return True
    return False


def bwd_plan(d, has_dlse):
    """(dq_kernel, dkv_kernel) fa2_bwd_lse_plan reports for a dense case on the plain route, and whether fa2_bwd_workspace_bytes asks for the KV-split's
    workspace; None for the other routes (their entry points have no plan query)."""
    if d["mode"] != "dense" or d["window"] is not None or d["q_offset"] or d["p"] > 0 or d["softcap"] > 0 or d["slopes"] is not None or d["mask"] is not None:
        return None
    lib, a, code = _fa2_lib.load(), _fa2_lib.BwdPlan(), 0 if d["dtype"] == "float16" else 1
    flags = _fa2_lib.FA2_FLAG_CAUSAL if d["causal"] else 0
    _fa2_lib.check(lib.fa2_bwd_lse_plan(code, d["B"], d["H"], d["Hkv"], d["Nq"], d["Nkv"], d["D"], None, None, None, None, None, ff.scale_of(d), flags, 0, None,
                                        int(has_dlse), ctypes.byref(a)))
    split = d["H"] == d["Hkv"] and lib.fa2_bwd_workspace_bytes(code, d["B"], d["H"], d["Nq"], d["Nkv"], d["D"], flags) > 0
    return a.dq_kernel, a.dkv_kernel, bool(split)


def coverage(descs):
    """What a list of drawn cases reaches, as counts by name (every slice of tests/test_fuzz_lse_gpu.py must have each of its family's >= 1).  The
    plan items ask the library which kernels the drawn call runs (host functions: no GPU)."""
    c = {}

    def hit(name, cond=True):
        c[name] = c.get(name, 0) + int(bool(cond))
    for d in descs:
        fam = d["fam"]
        if fam == "merge":
            lanes = d["D"] // 8
            hit("merge with D / 8 not a power of two", lanes & (lanes - 1))
            hit("merge with 16 parts", d["nparts"] == 16)
            hit("merge with more than 32 parts", d["nparts"] > 32)
            hit("merge with a finite-LSE part of weight exactly 0", d["spread"] == 300 and d["nparts"] > 1)
            hit("merge with strided parts", d["strides"] != "contig" and d["via"] == "abi")
            hit("merge with parts of different strides (operator)", d["mixed_strides"])
            hit("merge in log2 units with a dlse and a backward", not d["natural"] and d["dlse"] and d["bwd"])
            hit("merge with a null dlse and a backward", not d["dlse"] and d["bwd"])
            continue
        if fam == "chain":
            hit("chain with a cut inside a tile", any(x % 64 for x in d["cuts"]))
            hit("chain with an all-dead part", _chain_dead_part(d))
            hit("chain with softcap or ALiBi", d["softcap"] > 0 or d["slopes"] is not None)
            hit("chain with grouped heads", d["H"] != d["Hkv"])
            continue
        packed, units, smod = d["mode"] == "packed", ff.units_of(d), d["softcap"] > 0 or d["slopes"] is not None
        g, hasu, bwd = d["H"] // d["Hkv"], d["u"] != "none", d["bwd"]
        ragged = any(u[0] % 64 for u in units)
        left_open = d["window"] is None or d["window"][0] < 0
        if fam == "scoremod":
            for f in (64, 128, 256, 512):
                hit("family %d with a modifier and a backward" % f, ff.family(d["D"]) == f and bwd)
            hit("off-family head dim with a modifier and a backward", ff.family(d["D"]) != d["D"] and bwd)
            for r in (128, 256):
                hit("rows %d with a modifier" % r, d["rows"] == r)
            hit("group >= 4 with per-batch slopes", g >= 4 and d["slopes"] in ("BH", "BH_view") and not packed)
            hit("packed per-sequence slopes", packed and d["slopes"] in ("BH", "BH_view") and len(units) > 1)
            neg = d["slopes"] is not None and d["slope_values"] in ("negative", "mixed") and left_open and ragged and bwd
            hit("negative slopes, unbounded left, ragged last Q tile, dense", neg and not packed)
            hit("negative slopes, unbounded left, ragged last Q tile, packed", neg and packed)
            hit("negative slopes at head dim 512's family with a backward", neg and d["D"] > 256)
            hit("a saturated cap", saturated(d))
            hit("a cap in its linear part", d["softcap"] > 0 and not saturated(d))
            hit("window edge inside a tile with q_offset > 0 under ALiBi", _edge_in_tile(d) and d["slopes"] is not None)
            hit("dead rows with a modifier", ff.has_dead_rows(d))
            hit("strided [B, H] slopes", d["slopes"] == "BH_view")
            hit("scale other than D^-0.5 with a modifier", d["scale_mul"] != 1.0)
            hit("row-padded or head-sliced input with a modifier", any(l[0] in ("rowpad", "headslice") for l in d["layouts"]))
            hit("zero-length sequence with a modifier", packed and any((u[0] == 0) != (u[1] == 0) for u in units))
            continue
        for f in (64, 128, 256, 512):
            hit("family %d with a u and a backward" % f, ff.family(d["D"]) == f and bwd and hasu)
        hit("off-family head dim with a u and a backward", ff.family(d["D"]) != d["D"] and bwd and hasu)
        for r in (128, 256):
            hit("rows %d with a u" % r, d["rows"] == r and hasu and bwd)
        hit("dead rows with a NaN u", ff.has_dead_rows(d) and hasu and bwd)
        hit("packed + window + u", packed and d["window"] is not None and hasu and bwd)
        hit("packed + dropout + u", packed and d["p"] > 0 and hasu and bwd)
        hit("packed + modifier + u", packed and smod and hasu and bwd)
        hit("packed bottom-right + u", packed and d["bottom_right"] and hasu and bwd)
        for dtk, shp in MASK_KINDS[:3]:
            hit("mask %s %s with a u" % (dtk, shp), d["mask"] is not None and d["mask"][1] == shp and hasu and bwd)
        hit("float mask with a u", d["mask"] is not None and d["mask"][0] == "float" and hasu and bwd)
        hit("fully masked rows with a u", d["mask"] is not None and d["mask"][2] and d["mask"][1] != "b11k" and hasu and bwd)
        hit("dO = None", d["u"] == "only" and bwd)
        hit("no dlse", d["u"] == "none" and bwd)
        hit("dense dropout + u", not packed and d["p"] > 0 and hasu and bwd)
        hit("dense modifier + u", not packed and smod and hasu and bwd)
        hit("dense window + u", not packed and d["window"] is not None and hasu and bwd)
        hit("grouped heads + u", g > 1 and hasu and bwd)
        hit("BNHD + u", not packed and d["bnhd"] and hasu and bwd)
        hit("scale other than D^-0.5 with a u", d["scale_mul"] != 1.0 and hasu and bwd)
        hit("row-padded or head-sliced input with a u", any(l[0] in ("rowpad", "headslice") for l in d["layouts"]) and hasu and bwd)
        plan = bwd_plan(d, True) if bwd and hasu else None
        plain = bwd_plan(d, False) if plan is not None else None
        hit("plan: the short dQ kernel takes a dlse", plan is not None and plan[0] == _fa2_lib.FA2_BWD_KERNEL_SHORT)
        hit("plan: D = 128 falls back from the hand-scheduled passes", plan is not None and d["D"] == 128 and plain[0] == _fa2_lib.FA2_BWD_KERNEL_ASM and
            plan[0] == _fa2_lib.FA2_BWD_KERNEL_HIP)
        hit("plan: the slabs above D = 256 take a dlse", bwd and hasu and d["D"] > 256)
        hit("plan: KV-split parts take a dlse", plan is not None and plan[2])
    return c


def shrink(desc, nmax):
    """The same call with every length capped at nmax (tests/test_fuzz_lse.py: the checker on the CPU)."""
    if desc["fam"] == "merge":
        return dict(desc, Nq=min(desc["Nq"], nmax))
    d = ff.shrink(desc, nmax)
    if desc["fam"] == "chain":
        cuts = sorted({min(x, d["Nkv"] - 1) for x in desc["cuts"] if min(x, d["Nkv"] - 1) >= 1}) or [d["Nkv"] // 2]
        d.update(cuts=cuts, q_offset=max(d["q_offset"], cuts[-1]))
    return d


# ---------------------------------------------------------------------------------------------------------------- tensors of a case
def slope_tensor(d, nb, dev):
    """The alibi_slopes argument of a case (None, [H], [nb, H] or a strided [nb, H] view), float32 on dev."""
    if d["slopes"] is None:
        return None
    H = d["H"]
    base = torch.tensor([2.0 ** (-8.0 * (i + 1) / H) for i in range(H)], dtype=torch.float32) * d["slope_mul"]
    sign = {"geometric": torch.ones(H), "negative": -torch.ones(H), "zero": torch.zeros(H),
            "mixed": torch.tensor([1.0 if (i * 7 + d["i"]) % 3 else -1.0 for i in range(H)])}[d["slope_values"]]
    a = base * sign
    if d["slopes"] == "H":
        return a.to(dev)
    full = torch.stack([a * (1.0 + 0.5 * b) * (-1.0 if d["slope_values"] == "mixed" and b % 2 else 1.0) for b in range(nb)])
    if d["slopes"] == "BH_view":
        wide = torch.full((nb, 2 * H), float("nan"))
        wide[:, ::2] = full
        return wide.to(dev)[:, ::2]
    return full.to(dev)


def _mask_tensor(d, gen):
    """The mask= argument of a dense lse case: bool (True = attend) or float (added to the scores), in one of the broadcast shapes."""
    if d["mask"] is None:
        return None
    kind, shp, dead_rows = d["mask"]
    B, H, Nq, Nkv = d["B"], d["H"], d["Nq"], d["Nkv"]
    shape = {"b1qk": (B, 1, Nq, Nkv), "1hqk": (1, H, Nq, Nkv), "b11k": (B, 1, 1, Nkv)}[shp]
    r = torch.rand(shape, generator=gen, device=gen.device)
    if kind == "bool":
        m = r < 0.7
        if shp == "b11k":
            m[..., 0] = True
        if dead_rows and shp != "b11k":
            m[:, :, Nq // 2] = False
        return m
    m = torch.randn(shape, generator=gen, device=gen.device)
    m = m.masked_fill(r < 0.1, float("-inf"))
    if shp == "b11k":
        m[..., 0] = 0.5
    if dead_rows and shp != "b11k":
        m[:, :, Nq // 2] = float("-inf")
    return m


def build_case(d, gen):
    """The tensors of a scoremod / lse / chain case on gen's device: fuzz_features.build_inputs' q, k, v, do (scaled by the case's amplitude), the slopes,
    the mask, u (NaN on rows that see no key and on the surplus rows) and per unit the float64 truth's arguments."""
    dev, H, g = gen.device, d["H"], d["H"] // d["Hkv"]
    inp = ff.build_inputs(d, gen)
    for n in ("q", "k", "v"):
        inp[n].mul_(d["amp"])
    units = ff.units_of(d)
    inp["slopes"] = slope_tensor(d, len(units), dev)
    inp["mask"] = _mask_tensor(d, gen)
    nrow = inp["q"].shape[0] if d["mode"] == "packed" else d["Nq"]
    u = torch.randn((H, nrow) if d["mode"] == "packed" else (d["B"], H, nrow), generator=gen, device=dev)
    if d["mode"] == "packed":
        u[:, inp["total_q"]:] = float("nan")
    inp["refs"] = []
    for b, (un, (nq, nk, left, right, off)) in enumerate(zip(inp["units"], units)):
        ub = u[:, un["q0"]:un["q0"] + nq] if d["mode"] == "packed" else u[b]
        if nq == 0 or nk == 0:
            ub.fill_(float("nan"))
            inp["refs"].append(None)
            continue
        allow, bias, keep, rs = ff.band(nq, nk, left, right, off, False, dev), None, None, 1.0
        if inp["mask"] is not None:
            mb = inp["mask"][b if inp["mask"].shape[0] > 1 else 0]
            if mb.dtype == torch.bool:
                allow = allow & mb
            else:
                bias, allow = mb, allow & ~torch.isneginf(mb)
        dead = ~allow.any(-1)
        ub[dead.expand(H, nq)] = float("nan")
        if d["p"] > 0:
            keep, rs = ff.keep_unit(d["seed"], d["p"], H, b, nq, nk).to(dev), 1.0 / (1.0 - ff.p_eff(d["p"]))
        sl = None if inp["slopes"] is None else inp["slopes"] if inp["slopes"].dim() == 1 else inp["slopes"][b]
        inp["refs"].append(dict(q=un["q"], ke=un["k"].repeat_interleave(g, 0), ve=un["v"].repeat_interleave(g, 0), allow=allow,
                                do=torch.zeros_like(un["do"]) if d["u"] == "only" else un["do"], u=None if d["u"] == "none" else ub,
                                kw=dict(softcap=d["softcap"], slopes=sl, off=off, bias=bias, keep=keep, rs=rs)))
    inp["u"] = u
    return inp


def _folded(r, hkv):
    r["dK"], r["dV"] = fold(r["dK"], hkv), fold(r["dV"], hkv)
    return r


def unit_truth(d, ref, u="own", **kw):
    """float64 truth of one unit; u: "own" or None (the same call without the LSE term); kw replaces the modifiers (softcap=0.0, slopes=None)."""
    uu = None if u is None or ref["u"] is None else torch.nan_to_num(ref["u"], nan=0.0)       # (NaN only on dead rows, which the loss masks)
    return _folded(truth64(ref["q"], ref["ke"], ref["ve"], ref["do"], uu, ref["allow"], ff.scale_of(d), **dict(ref["kw"], **kw)), d["Hkv"])


def unit_emulation(d, ref, mut=(), u="own", **kw):
    return _folded(emulate(ref["q"], ref["ke"], ref["ve"], ref["do"], ref["u"] if u == "own" else u, ref["allow"], ff.scale_of(d),
                           getattr(torch, d["dtype"]), mut=mut, **dict(ref["kw"], **kw)), d["Hkv"])


def references(d, inp):
    """Per unit (None for one without queries or keys): true, emu, bars and the case's margin — by how many bars the modifiers (scoremod) or u (lse, chain)
    move the float64 outputs, the largest over the outputs and units."""
    dt, out, margin = getattr(torch, d["dtype"]), [], None
    names = NAMES if d["bwd"] else ("O", "lse")
    for ref in inp["refs"]:
        if ref is None:
            out.append(None)
            continue
        true, emu = unit_truth(d, ref), unit_emulation(d, ref)
        bars = bars_of(true, emu, dt)
        other = None
        if d["fam"] == "scoremod":
            other = unit_truth(d, ref, softcap=0.0, slopes=None)
        elif d["u"] != "none" and d["bwd"]:
            other, names_m = unit_truth(d, ref, u=None), ("dQ", "dK")
        if other is not None:
            for n in (names if d["fam"] == "scoremod" else names_m):
                a, b = true[n], other[n]
                if n == "lse":
                    live = ~torch.isinf(a) & ~torch.isinf(b)
                    a, b = a[live], b[live]
                if a.numel():
                    margin = max(margin or 0.0, (a - b).abs().max().item() / bars[n][0])
        out.append(dict(true=true, emu=emu, bars=bars))
    return out, margin


def emulated_outputs(d, inp, mutate=None):
    """The emulation's outputs in the shape of the operator's, per unit — "the kernel's output" of the CPU tests.  mutate(b, ref) -> None or
    dict(mut=, u=, slopes=, off=, ...): what a wrong kernel would compute with."""
    dt, got = getattr(torch, d["dtype"]), []
    for b, (ref, (nq, nk, *_)) in enumerate(zip(inp["refs"], ff.units_of(d))):
        if ref is None:
            z = lambda n, h: torch.zeros(h, n, d["D"], dtype=dt)             # noqa: E731
            got.append(dict(O=z(nq, d["H"]), lse=torch.full((d["H"], nq), float("-inf")), dQ=z(nq, d["H"]), dK=z(nk, d["Hkv"]), dV=z(nk, d["Hkv"])))
            continue
        m = dict(mutate(b, ref) or {}) if mutate is not None else {}
        e = unit_emulation(d, ref, mut=m.pop("mut", ()), u=m.pop("u", "own"), **m)
        got.append({n: (e[n].float() if n == "lse" else e[n].to(dt)) for n in NAMES})
    return got


def check_units(d, refs, got):
    """The checks of one case on the outputs `got` (per unit: O, lse in log2 units and, with a backward, dQ, dK, dV): -> (fails, figures)."""
    fails, fig = [], dict(o_ratio=0.0, grad_ratio=0.0, lse_ratio=0.0)
    names = NAMES if d["bwd"] else ("O", "lse")
    for b, (r, g, (nq, nk, *_)) in enumerate(zip(refs, got, ff.units_of(d))):
        tag = "unit %d (%d x %d)" % (b, nq, nk)
        bad = [n for n in names if not torch.isfinite(g[n].float().masked_fill(torch.isneginf(g[n].float()), 0.0) if n == "lse" else g[n].float()).all()]
        if bad:
            fails.append("%s: %s non-finite" % (tag, ", ".join(bad)))
            continue
        if r is None:
            if any((g[n] != 0).any() for n in names if n != "lse") or not torch.isneginf(g["lse"]).all():
                fails.append("%s: an empty side must give zeros and LSE = -inf" % tag)
            continue
        true, bars = r["true"], r["bars"]
        dead = torch.isinf(true["lse"])
        if dead.any() and ((g["O"][dead] != 0).any() or not torch.isneginf(g["lse"][dead]).all() or (d["bwd"] and (g["dQ"][dead] != 0).any())):
            fails.append("%s: rows that see no key must give O = dQ = 0 and LSE = -inf" % tag)
        for n in names:
            x, t = g[n].double(), true[n]
            if n == "lse":
                if torch.isinf(x[~dead]).any():
                    fails.append("%s: LSE infinite on a live row" % tag)
                    continue
                x, t = x[~dead], t[~dead]
            err = (x - t).abs().max().item() if x.numel() else 0.0
            key = "o_ratio" if n == "O" else "lse_ratio" if n == "lse" else "grad_ratio"
            fig[key] = max(fig[key], err / bars[n][0])
            if not err <= bars[n][0]:
                fails.append("%s: %s err %.3e > %.3e (emulation %.3e)" % (tag, n, err, bars[n][0], bars[n][1]))
    return fails, fig


# ---------------------------------------------------------------------------------------------------------------- running a case on the device
def _loss(out, lse, do, u, kind, nlive=None):
    """(out * dO).sum() + (lse * u).sum() over live rows (lse in natural-log units, as the operator returns it); kind: the case's u."""
    live = ~torch.isinf(lse.detach())
    if nlive is not None:
        live[..., nlive:] = False
    terms = []
    if kind != "only":
        terms.append((out.float() * do.float()).sum())
    if kind != "none":
        terms.append((lse * u).masked_fill(~live, 0.0).sum())
    return sum(terms)


def _call_dense(d, inp):
    from rocwmma_fattn.FlashAttn import flash_attention
    bnhd, B = d["bnhd"], d["B"]
    kw = dict(causal=d["causal"], scale=ff.scale_of(d), BNHD_fmt=bnhd, window=None if d["window"] is None else tuple(d["window"]), q_offset=d["q_offset"],
              dropout_p=float(d["p"]), dropout_seed=d["seed"] if d["p"] > 0 else None, softcap=d["softcap"], alibi_slopes=inp["slopes"], mask=inp["mask"])
    qo, ko, vo, doo = (ff._bhnd(inp[n], bnhd) for n in ("q", "k", "v", "do"))
    with torch.no_grad():
        o, lse = flash_attention(qo, ko, vo, return_lse=True, **kw)
    same, grads = True, [None] * 3
    if d["fam"] == "scoremod":      # the operator without return_lse (its own autograd node): the same bits
        same = torch.equal(o, flash_attention(qo, ko, vo, **kw))
    if d["bwd"]:
        qg, kg, vg = (t.detach().requires_grad_(True) for t in (qo, ko, vo))
        if d["fam"] == "scoremod":
            og = flash_attention(qg, kg, vg, **kw)
            og.backward(doo)
        else:
            og, lg = flash_attention(qg, kg, vg, return_lse=True, **kw)
            same = same and torch.equal(lg.detach(), lse)
            _loss(og, lg, doo, inp["u"], d["u"]).backward()
        same = same and torch.equal(og.detach(), o)
        grads = [ff._bhnd(t.grad, bnhd) for t in (qg, kg, vg)]
    ob = ff._bhnd(o, bnhd)
    got = [dict(O=ob[b], lse=lse[b] / LN2, **(dict(dQ=grads[0][b], dK=grads[1][b], dV=grads[2][b]) if d["bwd"] else {})) for b in range(B)]
    return got, same


def _call_packed(d, inp):
    from rocwmma_fattn.FlashAttn import flash_attention_varlen
    dev, lq, lk, tq = inp["q"].device, d["lens_q"], d["lens_k"], inp["total_q"]
    cu = lambda lens: torch.tensor([0] + [sum(lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32, device=dev)      # noqa: E731
    up = {"exact": lambda n: n, "round64": lambda n: -(-n // 64) * 64, "none": lambda n: None}[d["max_kind"]]
    kw = dict(max_seqlen_q=up(max(lq)), max_seqlen_k=up(max(lk)), causal=d["causal"], scale=ff.scale_of(d), window=None if d["window"] is None else tuple(d["window"]),
              bottom_right=d["bottom_right"], dropout_p=float(d["p"]), dropout_seed=d["seed"] if d["p"] > 0 else None, softcap=d["softcap"],
              alibi_slopes=inp["slopes"])
    cq, ck = cu(lq), cu(lk)
    with torch.no_grad():
        o, lse = flash_attention_varlen(inp["q"], inp["k"], inp["v"], cq, ck, return_lse=True, **kw)
    same, grads = True, [None] * 3
    if d["fam"] == "scoremod":
        same = torch.equal(o[:tq], flash_attention_varlen(inp["q"], inp["k"], inp["v"], cq, ck, **kw)[:tq])
    if d["bwd"]:
        qg, kg, vg = (inp[n].detach().requires_grad_(True) for n in ("q", "k", "v"))
        if d["fam"] == "scoremod":
            og = flash_attention_varlen(qg, kg, vg, cq, ck, **kw)
            og.backward(inp["do"])
        else:
            og, lg = flash_attention_varlen(qg, kg, vg, cq, ck, return_lse=True, **kw)
            same = same and torch.equal(lg.detach()[:, :tq], lse[:, :tq])
            dol = inp["do"].clone()
            dol[tq:] = 0                                     # (the surplus rows of dO are NaN: outside the loss)
            _loss(og[:tq], lg[:, :tq], dol[:tq], inp["u"][:, :tq], d["u"]).backward()
        same = same and torch.equal(og.detach()[:tq], o[:tq])
        grads = [t.grad for t in (qg, kg, vg)]
    got = []
    hm = lambda t, a, n: t[a:a + n].transpose(0, 1)                          # noqa: E731
    for un, nq, nk in zip(inp["units"], lq, lk):
        g = dict(O=hm(o, un["q0"], nq), lse=lse[:, un["q0"]:un["q0"] + nq] / LN2)
        if d["bwd"]:
            g.update(dQ=hm(grads[0], un["q0"], nq), dK=hm(grads[1], un["k0"], nk), dV=hm(grads[2], un["k0"], nk))
        got.append(g)
    return got, same


def chain_emulation(d, inp, refs):
    """The emulation of a chain case follows the path: each part's emulated out (rounded to the I/O dtype) and LSE, merged as the merge kernel does,
    rounded once; backwards the merge kernel's dO_k (rounded) and dlse_k into each part's emulated backward, dQ accumulated in the I/O dtype."""
    dt, scale, Hkv = getattr(torch, d["dtype"]), ff.scale_of(d), d["Hkv"]
    for ref, r in zip(inp["refs"], refs):
        allow_parts = [ref["allow"][:, c0:c1] for c0, c1 in parts_of(d)]
        sub = lambda t, c0, c1: t[:, c0:c1]                                  # noqa: E731
        kw = lambda c0: dict(ref["kw"], off=ref["kw"]["off"] - c0)            # noqa: E731
        fw = [emulate(ref["q"], sub(ref["ke"], c0, c1), sub(ref["ve"], c0, c1), ref["do"], None, al, scale, dt, **kw(c0)) for (c0, c1), al in zip(parts_of(d), allow_parts)]
        outs, lses = [e["O"].to(dt) for e in fw], [(e["lse"] * LN2).float() for e in fw]
        out, lse, dos, dls = merge_emulate(outs, lses, ref["do"], ref["u"].masked_fill(torch.isnan(ref["u"]), 0.0), True, dt)
        emu = dict(O=out.double(), lse=(lse.double() / LN2))
        dQ, dK, dV = None, [], []
        for (c0, c1), al, do_k, dl_k in zip(parts_of(d), allow_parts, dos, dls):
            e = emulate(ref["q"], sub(ref["ke"], c0, c1), sub(ref["ve"], c0, c1), do_k, dl_k, al, scale, dt, **kw(c0))
            dQ = e["dQ"].to(dt) if dQ is None else (dQ + e["dQ"].to(dt))
            dK.append(e["dK"])
            dV.append(e["dV"])
        emu.update(dQ=dQ.double(), dK=fold(torch.cat(dK, 1), Hkv), dV=fold(torch.cat(dV, 1), Hkv))
        r["emu"], r["bars"] = emu, bars_of(r["true"], emu, dt)
    return refs


def _call_chain(d, inp):
    from rocwmma_fattn.FlashAttn import flash_attention, merge_attention
    qg, kg, vg = (inp[n].detach().requires_grad_(True) for n in ("q", "k", "v"))
    kw = dict(causal=d["causal"], scale=ff.scale_of(d), window=None if d["window"] is None else tuple(d["window"]), softcap=d["softcap"], alibi_slopes=inp["slopes"])
    outs, lses = [], []
    for c0, c1 in parts_of(d):
        o, l = flash_attention(qg, kg[:, :, c0:c1], vg[:, :, c0:c1], q_offset=d["q_offset"] - c0, return_lse=True, **kw)
        outs.append(o)
        lses.append(l)
    out, lse = merge_attention(outs, lses)
    got_dead_part = any(bool(torch.isneginf(l).all()) for l in lses)
    if d["bwd"]:
        _loss(out, lse, inp["do"], inp["u"], "randn").backward()
    got = [dict(O=out.detach()[b], lse=lse.detach()[b] / LN2, **(dict(dQ=qg.grad[b], dK=kg.grad[b], dV=vg.grad[b]) if d["bwd"] else {})) for b in range(d["B"])]
    return got, got_dead_part


def _run_attention(d, gen):
    inp = build_case(d, gen)
    refs, margin = references(d, inp)
    out = dict(d, margin=margin, quiet=margin is not None and margin < QUIET_BARS)
    if d["fam"] == "chain":
        refs = chain_emulation(d, inp, refs)
        call = lambda: _call_chain(d, inp)                                   # noqa: E731
    else:
        call = lambda: ff._with_rows(d["rows"], lambda: (_call_packed if d["mode"] == "packed" else _call_dense)(d, inp))        # noqa: E731
        if d["bwd"] and d["u"] != "none":
            out["plan"] = bwd_plan(d, True)
    got, flag = call()
    fails, fig = check_units(d, refs, got)
    if d["fam"] == "chain":
        out["dead_part"] = flag
        if flag != _chain_dead_part(d):
            fails.append("the draw says %s all-dead part, the parts' LSEs say otherwise" % ("an" if _chain_dead_part(d) else "no"))
    elif not flag:
        fails.append("the calls with and without return_lse / a gradient differ bit-wise")
    if d["twice"]:
        for b, (g, g2) in enumerate(zip(got, call()[0])):
            fails += ["unit %d: %s differs between two runs" % (b, n) for n in g if not torch.equal(g[n], g2[n])]
    out.update(fig, fails=fails)
    return out


# ---------------------------------------------------------------------------------------------------------------- merge
def merge_inputs(d, gen):
    """The parts of a merge case on gen's device, as [B, H, N, D] / [B, H, N] views plus the tensors in the kernel's layout: LSEs spread over the case's
    range (spread 300: whole parts sit ZERO_GAP+ log2 units below others, weight exactly 0 in f32), row 0 and a share of the rows dead in every part,
    NaN / inf under every weight of exactly 0, dO and dlse."""
    dev, dt, n, B, H, N, D = gen.device, getattr(torch, d["dtype"]), d["nparts"], d["B"], d["H"], d["Nq"], d["D"]
    unit = 1.0 if d["natural"] else LOG2E
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)              # noqa: E731
    dead_all = torch.rand((B, H, N), generator=gen, device=dev) < d["dead_frac"]
    if N > 1:
        dead_all[:, :, 0] = True
    sigma = {0: 0.0, 40: 6.0, 300: 2.0}[d["spread"]]
    outs, lses, raw = [], [], []
    for k in range(n):
        l = rnd(B, H, N) * sigma + 0.25 * rnd(B, H, N)                       # natural-log units
        if d["spread"] == 300:
            l = l - 300.0 * LN2 * (torch.rand((B, H, N), generator=gen, device=dev) < 0.4)
        l = l.masked_fill((torch.rand((B, H, N), generator=gen, device=dev) < (0.2 if n > 1 else 0.0)) | dead_all, float("-inf"))
        raw.append(l)
    top = torch.stack(raw).max(0).values
    for k in range(n):
        zero = torch.isneginf(raw[k]) | ((raw[k] - top) / LN2 < -ZERO_GAP)
        assert not (((raw[k] - top) / LN2 < -120.0) & ~zero).any()          # (no weight in the denormal range: either a normal f32 or exactly 0)
        shape = {"bhnd": (B, H, N, D), "bnhd": (B, N, H, D), "packed": (N, H, D)}[d["layout"]]
        if d["strides"] == "rowpad" or (d["mixed_strides"] and k % 3 == 1):
            t = torch.full(shape[:-1] + (D + d["par"] * (1 if d["strides"] == "rowpad" else 8),), float("nan"), dtype=dt, device=dev)[..., :D]
        elif d["strides"] == "headslice" or (d["mixed_strides"] and k % 3 == 2):
            hax = {"bhnd": 1, "bnhd": 2, "packed": 1}[d["layout"]]
            big = list(shape)
            big[hax] += d["par"] if d["strides"] == "headslice" else 1
            t = torch.full(big, float("nan"), dtype=dt, device=dev).narrow(hax, (d["par"] if d["strides"] == "headslice" else 1) // 2, H)
        else:
            t = torch.empty(shape, dtype=dt, device=dev)
        view = t if d["layout"] == "bhnd" else t.transpose(1, 2) if d["layout"] == "bnhd" else t.transpose(0, 1).unsqueeze(0)
        view.copy_(rnd(B, H, N, D).to(dt))
        view[zero] = torch.tensor([float("nan"), float("inf"), -65504.0][k % 3], dtype=dt, device=dev)
        lt = (raw[k] * unit).contiguous()
        outs.append(dict(t=t, view=view, zero=zero))
        lses.append(lt)
    dshape = {"bhnd": (B, H, N, D), "bnhd": (B, N, H, D), "packed": (N, H, D)}[d["layout"]]
    dout = rnd(*dshape).to(dt)
    dlse = rnd(B, H, N)
    return dict(outs=outs, lses=lses, dout=dout, dlse=dlse, dead_all=dead_all)


def _views(layout):
    """(outs' view as [B, H, N, D], lses' kernel form of a [B, H, N] tensor) of the kernel's layout."""
    if layout == "packed":
        return (lambda t: t.transpose(0, 1).unsqueeze(0)), (lambda t: t[0])
    if layout == "bnhd":
        return (lambda t: t.transpose(1, 2)), (lambda t: t)
    return (lambda t: t), (lambda t: t)


def _raw_merge(d, mi):
    """fa2_merge_fwd, then fa2_merge_bwd, straight through the C-ABI -> (out, lse, do parts, dlse parts) as [B, H, N, D] / [B, H, N] views."""
    lib, n, layout = _fa2_lib.load(), d["nparts"], d["layout"]
    vo, kl = _views(layout)
    parts, lses = [o["t"] for o in mi["outs"]], [kl(l).contiguous() for l in mi["lses"]]
    o0, dlse = parts[0], kl(mi["dlse"]).contiguous() if d["dlse"] else None
    if layout == "packed":
        geo, s3, s2 = (1, o0.shape[1], o0.shape[0], o0.shape[2]), (lambda t: _fa2_lib.strides3(0, t.stride(1), t.stride(0))), (lambda t: _fa2_lib.strides2(0, t.stride(0)))
    elif layout == "bnhd":
        geo, s3, s2 = (o0.shape[0], o0.shape[2], o0.shape[1], o0.shape[3]), (lambda t: _fa2_lib.strides3(t.stride(0), t.stride(2), t.stride(1))), (lambda t: _fa2_lib.strides2(t.stride(0), t.stride(1)))
    else:
        geo, s3, s2 = tuple(o0.shape), (lambda t: _fa2_lib.strides3(t.stride(0), t.stride(1), t.stride(2))), (lambda t: _fa2_lib.strides2(t.stride(0), t.stride(1)))
    arr = lambda ts: (ctypes.c_void_p * n)(*(t.data_ptr() for t in ts))      # noqa: E731
    out, lse = torch.full_like(mi["dout"], 7.0), torch.full_like(lses[0], 7.0)
    flags = _fa2_lib.FA2_MERGE_NATURAL_LSE if d["natural"] else 0
    stream, code = torch.cuda.current_stream().cuda_stream, 0 if o0.dtype == torch.float16 else 1
    _fa2_lib.check(lib.fa2_merge_fwd(code, n, arr(parts), arr(lses), out.data_ptr(), lse.data_ptr(), *geo, s3(o0), s2(lses[0]), s3(out), s2(lse), flags, stream))
    res = [vo(out), lse if layout != "packed" else lse.unsqueeze(0)]
    if d["bwd"]:
        dos, dls = [torch.full_like(mi["dout"], 7.0) for _ in range(n)], [torch.full_like(lse, 7.0) for _ in range(n)]
        _fa2_lib.check(lib.fa2_merge_bwd(code, n, arr(parts), arr(lses), lse.data_ptr(), mi["dout"].data_ptr(), None if dlse is None else dlse.data_ptr(), arr(dos),
                                         arr(dls), *geo, s3(o0), s2(lses[0]), s2(lse), s3(mi["dout"]), None if dlse is None else s2(dlse), s3(dos[0]), s2(dls[0]),
                                         flags, stream))
        res += [[vo(t) for t in dos], [t if layout != "packed" else t.unsqueeze(0) for t in dls]]
    torch.cuda.synchronize()
    return res


def _op_merge(d, mi):
    """merge_attention on the parts (natural-log LSEs) and, for a backward case, its autograd -> as _raw_merge."""
    from rocwmma_fattn.FlashAttn import merge_attention
    vo, kl = _views(d["layout"])
    parts = [o["t"].detach().requires_grad_(d["bwd"]) for o in mi["outs"]]
    lses = [kl(l).contiguous().requires_grad_(d["bwd"]) for l in mi["lses"]]
    out, lse = merge_attention(parts, lses, BNHD_fmt=d["layout"] == "bnhd")
    up = (lambda t: t.unsqueeze(0)) if d["layout"] == "packed" else (lambda t: t)
    res = [vo(out.detach()), up(lse.detach())]
    if d["bwd"]:
        live = ~torch.isneginf(lse.detach())
        loss = (out.float() * mi["dout"].float()).sum()
        if d["dlse"]:
            loss = loss + (lse * kl(mi["dlse"])).masked_fill(~live, 0.0).sum()
        loss.backward()
        res += [[vo(p.grad) for p in parts], [up(l.grad) for l in lses]]
    return res


def merge_folds(n):
    """The number of fa2_merge_fwd calls merge_attention makes for n parts (groups of 16, each later one led by the previous result)."""
    return 1 if n <= 16 else 1 + -(-(n - 16) // 15)


def check_merge(d, mi, res):
    """merge_check on a merge case's results (res: out, lse and, for a backward case, the parts' gradients, as [B, H, N, D] / [B, H, N] views); more
    than 16 parts: the forward under test_seventeen_parts_fold_in_groups' bar with one rounding per fold.  Parts of weight exactly 0 enter the float64
    reference as zeros (float64 would give 2^-300 times a NaN) and must get zero gradients."""
    dt, fails = getattr(torch, d["dtype"]), []
    clean = [torch.where(o["zero"].unsqueeze(-1), torch.zeros_like(o["view"]), o["view"]) for o in mi["outs"]]
    vo, _ = _views(d["layout"])
    if not all(torch.isfinite(t.float()).all() for t in [res[0]] + (res[2] + res[3] if d["bwd"] else [])):
        return ["non-finite output"], {}
    unit = 1.0 if d["natural"] else LN2
    fig = {}
    if d["nparts"] > 16 or not d["bwd"]:
        O64, L64 = merge64(clean, [l * unit for l in mi["lses"]])
        dead = torch.isneginf(L64)
        if not torch.equal(dead, mi["dead_all"] | dead) or not (torch.isneginf(res[1][dead]).all() and (res[0][dead] == 0).all()):
            fails.append("dead rows: O = 0, lse = -inf")
        live = ~dead
        err_o = (res[0].double() - O64).abs().max().item()
        err_l = ((res[1].double() * unit - L64)[live] / LN2).abs().max().item() if live.any() else 0.0
        bar_o = 2 * merge_folds(d["nparts"]) * MERGE_EPS[dt] * max(1.0, O64.abs().max().item())
        fig = dict(o_ratio=err_o / bar_o, lse_ratio=err_l / LSE_TOL)
        if not (err_o <= bar_o and err_l <= LSE_TOL):
            fails.append("O err %.3e (bar %.3e), lse err %.3e" % (err_o, bar_o, err_l))
        if d["nparts"] == 1 and not torch.equal(res[0][live], mi["outs"][0]["view"][live]):
            fails.append("one part: its rows must come back bit for bit")
        return fails, fig
    dlse = mi["dlse"] if d["dlse"] else torch.zeros_like(mi["dlse"])
    try:
        merge_check("case %d" % d["i"], dt, d["natural"], clean, mi["lses"], vo(mi["dout"]), dlse, res[0], res[1], res[2], res[3])
    except AssertionError as e:
        fails.append("merge_check: %s" % (e,))
    for k, o in enumerate(mi["outs"]):
        if (res[2][k][o["zero"]] != 0).any() or (res[3][k][o["zero"]] != 0).any():
            fails.append("part %d: a weight of exactly 0 must give zero gradients" % k)
    return fails, fig


def _run_merge(d, gen):
    mi = merge_inputs(d, gen)
    call = lambda: (_op_merge if d["via"] == "op" else _raw_merge)(d, mi)    # noqa: E731
    res = call()
    fails, fig = check_merge(d, mi, res)
    if d["twice"]:
        flat = lambda r: [r[0], r[1]] + (r[2] + r[3] if len(r) > 2 else [])      # noqa: E731
        if not all(torch.equal(a, b) for a, b in zip(flat(res), flat(call()))):
            fails.append("two runs differ")
    return dict(d, fails=fails, **fig)


def run_case(desc, gen):
    """Build the tensors of a drawn case on gen's device, run the operator, check: desc plus the figures and `fails`."""
    return _run_merge(desc, gen) if desc["fam"] == "merge" else _run_attention(desc, gen)


def quiet_share(results):
    """(quiet cases, cases that carry a margin) of run or reference-only results."""
    with_margin = [r for r in results if r.get("margin") is not None]
    return sum(r["margin"] < QUIET_BARS for r in with_margin), len(with_margin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--bwd-every", type=int, default=2, help="every n-th case also runs the backward (0 = never)")
    ap.add_argument("--mode", default="scoremod", choices=MODES)
    ap.add_argument("--long", action="store_true", help="lengths up to 1500 at head dims <= 128")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", type=int, default=None, help="run this case of the sweep alone (the earlier ones only draw their tensors, so that it sees the same inputs)")
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(args.seed)
    bad, worst, n_bwd, results = [], dict(o_ratio=0.0, grad_ratio=0.0, lse_ratio=0.0), 0, []
    for desc in draw_sweep(args.seed, [((args.mode, args.long), args.cases)], args.bwd_every):
        if args.only is not None and desc["i"] != args.only:
            if desc["i"] < args.only:
                (merge_inputs if desc["fam"] == "merge" else build_case)(desc, gen)
            continue
        try:
            d = run_case(desc, gen)
        except Exception as e:                      # a refused shape or a launch error is a finding too
            d = dict(desc, fails=["exception: %r" % (e,)])
        n_bwd += int(desc["bwd"])
        results.append(d)
        for key in worst:
            worst[key] = max(worst[key], d.get(key, 0.0))
        if d["fails"]:
            bad.append(d)
            print("FAIL", json.dumps(d), flush=True)
    quiet, margined = quiet_share(results)
    summary = dict(tool="fuzz_lse", mode=args.mode, cases=args.cases, backward_cases=n_bwd, seed=args.seed, failures=len(bad), worst_o_err_over_bar=worst["o_ratio"],
                   worst_grad_err_over_bar=worst["grad_ratio"], worst_lse_err_over_bar=worst["lse_ratio"], quiet_cases=quiet, cases_with_a_margin=margined,
                   coverage=coverage([{k: v for k, v in r.items()} for r in results]), device=torch.cuda.get_device_name(0), failing=bad)
    line = json.dumps(summary)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
