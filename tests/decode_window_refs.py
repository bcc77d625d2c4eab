"""References, cases and bars of the windowed decode tests (tests/test_decode_window.py, tests/test_decode_window_gpu.py).

The contract of fa2_fwd_decode_window (include/fa2_gfx950.h), per sequence, for query row i at pos = len - Nq + i, query head h and key j:
    x = (q_i . K_j) * scale;  s = softcap > 0 ? softcap * tanh(x / softcap) : x;  s -= slope[b, h] * (pos - j)
    keep(j) = 0 <= j <= pos and (window_left < 0 or j >= pos - window_left), the masks last.
truth64 is dense float64 of exactly that; emulate is the kernels' contract in torch (f32 scores, transform and sums; P rounded to the I/O dtype; one
rounding of O), in the style of tests/test_scoremod_gpu.py, forward only.  Bars: the project's rule, tools/fuzz_features.py: error_and_bar,
    max|got - true| <= max(2 * err_emu, FLOOR[code] * max(1, max|true|)) for O, max(LSE_TOL, 2 * err_emu) for the log2 LSE,
taken per sequence.  Inputs: q, k, v = 2 * N(0, 1).  Plain CPU code: nothing here touches a device."""
import functools
import importlib.util
import math
import os

import torch

from conftest import FLOOR, LSE_TOL

LN2 = math.log(2.0)
F16, BF16 = torch.float16, torch.bfloat16
LENS = (1, 63, 64, 65, 127, 129, 1000, 0, 2)
NMAX = 1024
SPLITS = (0, 1, 3, 16)
# (H, Hkv, Nq, D, dtype) of tests/test_decode_gpu.py's SHAPES: 12, 4, 20, 64 and 48 rows per K / V head — one, one, two, four and (three ->) four row
# tiles; both head dims and both dtypes; the 64-row D = 128 shape is the instantiation with the fewest registers to spare
SHAPES = [(8, 2, 3, 128, BF16), (8, 2, 1, 64, F16), (10, 2, 4, 128, F16), (16, 1, 4, 128, BF16), (16, 1, 3, 64, F16)]
IDS = ["H%d_Hkv%d_Nq%d_D%d_%s" % (s[0], s[1], s[2], s[3], "f16" if s[4] == F16 else "bf16") for s in SHAPES]
# name -> (window_left, softcap, slopes: None, "H" or "BH"); window 0: each row sees its own key alone
CASES = {"window31": (31, 0.0, None), "window100": (100, 0.0, None), "window0": (0, 0.0, None), "softcap8": (-1, 8.0, None), "softcap30": (-1, 30.0, None),
         "slopes_H": (-1, 0.0, "H"), "slopes_BH": (-1, 0.0, "BH"), "all": (100, 8.0, "BH")}

_spec = importlib.util.spec_from_file_location("_fuzz_features", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "tools", "fuzz_features.py"))
_ff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ff)


def code_of(dt):
    return 0 if dt == F16 else 1


def alibi_slopes(h, mul=1.0):
    """tests/test_scoremod_gpu.py's"""
    return torch.tensor([mul * 2.0 ** (-8.0 * (i + 1) / h) for i in range(h)], dtype=torch.float32)


def slopes_of(kind, B, H):
    """None, the [H] vector, or a [B, H] tensor whose rows differ"""
    if kind is None:
        return None
    if kind == "H":
        return alibi_slopes(H)
    return torch.stack([alibi_slopes(H, 0.5 + 0.25 * b) for b in range(B)])


def window_lo(n, Nq, window_left):
    """the lowest key any row of a sequence of n keys sees"""
    return 0 if window_left < 0 else max(0, n - Nq - window_left)


def keep_mask(n, Nq, window_left):
    """bool [Nq, n]"""
    pos = (n - Nq + torch.arange(Nq)).unsqueeze(1)
    j = torch.arange(n).unsqueeze(0)
    keep = j <= pos
    if window_left >= 0:
        keep = keep & (j >= pos - window_left)
    return keep


def _scores(q, k, scale, softcap, slopes, f, pos=None, cap_last=False):
    """q [H, Nq, D], k [H, n, D] -> S [H, Nq, n] in dtype f, before the masks.  scale: a float, or a tensor that broadcasts over [H, Nq, n] (an e4m3
    cache: scale * k_descale per head).  pos / cap_last exist for the mutants of tests/test_fuzz_decode.py: other row positions than len - Nq + i, and
    the cap applied after the ALiBi term."""
    Nq, n = q.shape[1], k.shape[1]
    S = (q.to(f) @ k.to(f).transpose(-1, -2)) * (scale.to(f) if torch.is_tensor(scale) else scale)
    if softcap > 0 and not cap_last:
        S = softcap * torch.tanh(S / softcap)
    if slopes is not None:
        pos = n - Nq + torch.arange(Nq) if pos is None else pos
        dist = (pos.unsqueeze(1) - torch.arange(n).unsqueeze(0)).to(f)
        S = S - slopes.to(f)[:, None, None] * dist
    if softcap > 0 and cap_last:
        S = softcap * torch.tanh(S / softcap)
    return S


def _softmax_parts(S, keep):
    S = S.masked_fill(~keep, float("-inf"))
    m = S.max(-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    E = torch.exp(S - m)
    l = E.sum(-1, keepdim=True)
    l1 = torch.where(l > 0, l, torch.ones_like(l))
    lse = ((m + torch.log(l)) / LN2).squeeze(-1)
    lse[..., ~keep.any(-1)] = float("-inf")
    return E, l1, lse


def truth64(q, k, v, scale, window_left, softcap, slopes, keep=None, pos=None, cap_last=False):
    """float64 of the contract for [H, Nq, D] q and [H, n, D] k / v (grouped heads already expanded), n >= 1 -> O [H, Nq, D], lse [H, Nq] (log2 units).
    keep (bool [Nq, n]), pos and cap_last replace the contract's own mask, row positions and order: the mutants of tests/test_fuzz_decode.py."""
    keep = keep_mask(k.shape[1], q.shape[1], window_left) if keep is None else keep
    E, l1, lse = _softmax_parts(_scores(q, k, scale, softcap, slopes, torch.float64, pos, cap_last), keep)
    return (E / l1) @ v.double(), lse


def emulate(q, k, v, scale, window_left, softcap, slopes, dt, v_descale=None):
    """The kernel's contract in torch: f32 scores, transform and sums; P rounded to the I/O dtype; O rounded once.  An e4m3 cache with general descales
    (tests/test_decode_fp8_gpu.py: test_general_descales_against_float64): k and v are the upcast codes, k_descale is folded into `scale` (a tensor
    [H, 1, 1]) and v_descale [H, 1, 1] multiplies the normalised f32 row before its one rounding."""
    keep = keep_mask(k.shape[1], q.shape[1], window_left)
    E, l1, lse = _softmax_parts(_scores(q, k, scale, softcap, slopes, torch.float32), keep)
    O = (E.to(dt).float() @ v.float()) / l1
    if v_descale is not None:
        O = O * v_descale.float()
    return O.to(dt).double(), lse.double()


def bars_of(true, emu, code):
    """(O bar, lse bar) of one sequence"""
    (to, tl), (eo, el) = true, emu
    _, _, obar = _ff.error_and_bar(eo, to, eo, FLOOR[code])
    live = ~torch.isinf(tl)
    e = (el[live] - tl[live]).abs().max().item() if live.any() else 0.0
    return obar, max(LSE_TOL, 2 * e)


def seq_refs(q, k, v, lens, scale, window_left, softcap, slopes, dt):
    """q [B, Nq, H, D], k / v [B, Nmax, Hkv, D] float tensors holding I/O-dtype values (an e4m3 cache: upcast and descaled) -> per sequence None (no
    keys) or dict(true, plain, emu, bars): float64 with the keywords, float64 without them, the emulation, the bars."""
    G, out = q.shape[2] // k.shape[2], []
    for b, n in enumerate(lens):
        if n == 0:
            out.append(None)
            continue
        qs = q[b].transpose(0, 1)
        ks, vs = (t[b, :n].transpose(0, 1).repeat_interleave(G, dim=0) for t in (k, v))
        sl = None if slopes is None else (slopes if slopes.dim() == 1 else slopes[b])
        true = truth64(qs, ks, vs, scale, window_left, softcap, sl)
        plain = truth64(qs, ks, vs, scale, -1, 0.0, None)
        emu = emulate(qs, ks, vs, scale, window_left, softcap, sl, dt)
        out.append(dict(true=true, plain=plain, emu=emu, bars=bars_of(true, emu, code_of(dt))))
    return out


def margins(refs):
    """(O margin, lse margin) of a case: (float64 with the keywords - float64 without) / the bar, the largest over the batch — short sequences lie inside
    any window.  Rows that see no key in either are left out of the LSE difference (-inf - -inf)."""
    mo = ml = 0.0
    for r in refs:
        if r is None:
            continue
        (to, tl), (po, pl) = r["true"], r["plain"]
        mo = max(mo, (to - po).abs().max().item() / r["bars"][0])
        live = ~torch.isinf(tl)
        if live.any():
            ml = max(ml, (tl[live] - pl[live]).abs().max().item() / r["bars"][1])
    return mo, ml


@functools.lru_cache(maxsize=None)
def inputs(H, Hkv, Nq, D, dt):
    """CPU tensors of one shape, 2 * N(0, 1) rounded to the I/O dtype; every cache row holds a finite value here (dirty() makes the device copies)."""
    g = torch.Generator(device="cpu").manual_seed(4200 + 1000 * H + 100 * Hkv + 10 * Nq + D)
    B = len(LENS)
    q = (2 * torch.randn((B, Nq, H, D), generator=g)).to(dt)
    k = (2 * torch.randn((B, NMAX, Hkv, D), generator=g)).to(dt)
    v = (2 * torch.randn((B, NMAX, Hkv, D), generator=g)).to(dt)
    return q, k, v


@functools.lru_cache(maxsize=None)
def case_refs(shape, name):
    """The shared references of (shape, case): computed once, never modified."""
    H, Hkv, Nq, D, dt = shape
    wl, cap, kind = CASES[name]
    q, k, v = inputs(*shape)
    return seq_refs(q.float(), k.float(), v.float(), LENS, D ** -0.5, wl, cap, slopes_of(kind, len(LENS), H), dt)


# Windows almost as wide as the cache: window_left in [NMAX - Nq, NMAX - 2] reaches across the cache for row 0 but NOT for the later rows of a full
# sequence, which must still drop the first keys (row i drops j < i + NMAX - Nq - window_left).  Only a few keys of 1 024 fall out, so the first Nq keys
# are loud (k and v four times the rest): a row that wrongly keeps them is off by far more than a bar.
EDGE_LENS = (NMAX, NMAX - 1, NMAX, 1000, 3)
EDGE_SHAPES = [(10, 2, 4, 128, F16), (8, 2, 3, 128, BF16), (16, 1, 4, 128, BF16)]
EDGE_IDS = ["H%d_Hkv%d_Nq%d_D%d_%s" % (s[0], s[1], s[2], s[3], "f16" if s[4] == F16 else "bf16") for s in EDGE_SHAPES]


def edge_windows(Nq):
    """(name, window_left): both ends of the range between row 0's and the last row's reach"""
    return (("NMAX-Nq", NMAX - Nq), ("NMAX-2", NMAX - 2))


@functools.lru_cache(maxsize=None)
def edge_inputs(H, Hkv, Nq, D, dt):
    g = torch.Generator(device="cpu").manual_seed(9100 + 1000 * H + 100 * Hkv + 10 * Nq + D)
    B = len(EDGE_LENS)
    q = (2 * torch.randn((B, Nq, H, D), generator=g)).to(dt)
    k = 2 * torch.randn((B, NMAX, Hkv, D), generator=g)
    v = 2 * torch.randn((B, NMAX, Hkv, D), generator=g)
    k[:, :Nq] *= 4
    v[:, :Nq] *= 4
    return q, k.to(dt), v.to(dt)


@functools.lru_cache(maxsize=None)
def edge_refs(shape, window_left):
    H, Hkv, Nq, D, dt = shape
    q, k, v = edge_inputs(*shape)
    return seq_refs(q.float(), k.float(), v.float(), EDGE_LENS, D ** -0.5, window_left, 0.0, None, dt)


def dirty(t, Nq, window_left, fill=float("nan"), lens=LENS):
    """A copy of the cache [B, Nmax, Hkv, D] with `fill` in every row at or beyond a length and below the sequence's lowest visible key."""
    t = t.clone()
    for b, n in enumerate(lens):
        t[b, n:] = fill
        t[b, :window_lo(n, Nq, window_left)] = fill
    return t


def check(o, lse2, refs, tag, verbose=False):
    """o [B, Nq, H, D] and the log2 lse [B, H, Nq] against float64 under the bars; rows that see no key exactly 0 / -inf, every element written."""
    got_o, got_l = o.detach().double().cpu(), lse2.detach().double().cpu()
    assert torch.isfinite(got_o).all(), (tag, "O not finite: an element was not written, or a NaN outside the visible keys leaked")
    assert not torch.isnan(got_l).any(), (tag, "LSE not written, or NaN")
    for b, r in enumerate(refs):
        go, gl = got_o[b].transpose(0, 1), got_l[b]
        if r is None:
            assert bool((go == 0).all()) and bool(torch.isneginf(gl).all()), (tag, b, "a sequence without keys")
            continue
        (to, tl), (obar, lbar) = r["true"], r["bars"]
        dead = torch.isinf(tl)
        assert bool((go[dead] == 0).all()) and bool(torch.isneginf(gl[dead]).all()), (tag, b, "rows that see no key")
        err = (go - to).abs().max().item()
        lerr = (gl[~dead] - tl[~dead]).abs().max().item() if (~dead).any() else 0.0
        if verbose:
            print(tag, "seq", b, "O err %.3g bar %.3g" % (err, obar), "lse err %.3g bar %.3g" % (lerr, lbar))
        assert err <= obar, (tag, b, "float64 O", err, obar)
        assert lerr <= lbar, (tag, b, "float64 LSE", lerr, lbar)
