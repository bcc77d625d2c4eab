"""Randomised float64 sweep of the windowed, packed, grouped and dropout calls (developer tool; the committed output lives under profiles/).

tools/fuzz_parity.py draws the plain call and tools/fuzz_mask.py the masked one; this tool draws what they never pass: `window=` / `q_offset=`,
k / v with fewer heads, `dropout_p=` / `dropout_seed=`, option "rows", scales other than D^-0.5 on those paths, and flash_attention_varlen.  Four
families (--mode, draw_case's `force`):
    dense          flash_attention(window, q_offset, dropout_p, grouped k / v, four layouts per tensor, BNHD or BHND)
    packed         flash_attention_varlen(lengths with zeros, top-left / bottom-right, window, dropout, surplus NaN rows behind cu[B])
    dropout_long   dropout with Nq > 512 and Nkv > 1024 on grids of several workgroups per head, head dims 64 / 128 / 256
    readback       the keep mask each of the three passes used, decoded bit for bit from O (forward), dV (dK / dV pass) and dQ (dQ pass)
The reference is dense float64 attention with the band as -inf, the keep mask from the library's host function and grouped k / v expanded (ref64); the
bar is the dropout suite's, err <= max(2 * err_emu, tol * max(1, max|true|)), err_emu = the error of a same-contract emulation (emu) on that case,
tol = FLOOR / GRAD_TOL of tests/conftest.py; the LSE (log2 units, that of the undropped probabilities) takes fuzz_parity's rule.  Rows that see no key
must return O = dQ = 0 exactly and LSE = -inf; everything is finite; every fourth case runs twice and must repeat bit for bit.

The draw (draw_case, pure Python) is separate from the run (run_case) so that tests/test_fuzz_features.py can check the draw's coverage, the
checker's power against mutant outputs and the readback decode on the CPU.

    python tools/fuzz_features.py --mode dense --cases 1500 --seed 1 [--bwd-every 2] [--out FILE]
"""
import argparse
import concurrent.futures
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
import fuzz_parity as fzp  # noqa: E402 - the draw's lists, the contract of a folded launch, the LSE rule
from rocwmma_fattn import _fa2_lib  # noqa: E402

LN2 = math.log(2.0)
FLOOR, GRAD_TOL = fzp.FLOOR, fzp.GRAD_TOL              # tests/conftest.py's, by dtype
MODES = ("dense", "packed", "dropout_long", "readback")
WINDOW_EDGES = [-1, 0, 1, 31, 32, 63, 64, 65, 127, 128]
PACKED_LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257]
HEAD_COUNTS = [1, 2, 3, 4, 6, 8]
DROPOUT_PS = [2.0 ** -18, 2.0 ** -16, 0.1, 0.5, 0.9]    # 2^-18: threshold 0 (keeps everything, through the dropout kernels), 2^-16: threshold 1
READBACK_DIMS = [64, 128, 256, 512, 72, 200]
READBACK_PASSES = ("fwd", "dkv", "dq")
READBACK_STARTS = ("zero", "last_partial", "beyond", "random")
BITS = 4                                                # mask bits per output column of a readback call (eight are not exact in bf16)


# ---------------------------------------------------------------------------------------------------------------- the references
def p_eff(p):
    return round(p * 65536) / 65536.0


def threshold(p):
    return int(round(p * 65536))


def band(Nq, Nkv, left, right, off, causal, device=None):
    """The band as a bool [Nq, Nkv] (True = attend): row i sits at key position i + off; -1 = unbounded; causal means right = 0."""
    if causal:
        right = 0
    pos = torch.arange(Nq, device=device).unsqueeze(1) + off
    j = torch.arange(Nkv, device=device).unsqueeze(0)
    keep = torch.ones(Nq, Nkv, dtype=torch.bool, device=device)
    if left >= 0:
        keep &= j >= pos - left
    if right >= 0:
        keep &= j <= pos + right
    return keep


def ref64(q, k, v, do, keep, band, scale, p):
    """float64 truth for [H, Nq, D] q and [H, Nkv, D] k / v (already expanded): O, lse (log2 units), dQ, dK, dV.  scale: a number or [H, 1, 1]."""
    rs = 1.0 / (1.0 - p_eff(p))
    q, k, v = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    S = (q @ k.transpose(-1, -2)) * scale
    S = S.masked_fill(~band, float("-inf"))
    dead = ~band.any(-1)
    m = S.max(-1, keepdim=True).values.detach()                  # (a shift: the softmax does not depend on it)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    E = torch.exp(S - m)
    l = E.sum(-1, keepdim=True)
    P = E / torch.where(l > 0, l, torch.ones_like(l))
    O = (P * keep * rs) @ v
    lse = ((m + torch.log(l)) / LN2).squeeze(-1).detach()
    lse[..., dead] = float("-inf")
    O.backward(do.double())
    return O.detach(), lse, q.grad, k.grad, v.grad


def emu(q, k, v, do, keep, band, scale, p, dt, rs=None):
    """The kernels' contract in torch: f32 scores and sums, P rounded to the I/O dtype, outputs rounded once.  rs: 1 / (1 - p_eff) unless given."""
    rs = torch.tensor(1.0 / (1.0 - p_eff(p)) if rs is None else rs, dtype=torch.float32).item()
    qf, kf, vf, gf = q.float(), k.float(), v.float(), do.float()
    S = (qf @ kf.transpose(-1, -2)) * scale
    S = S.masked_fill(~band, float("-inf"))
    m = S.max(-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    E = torch.exp(S - m)
    l = E.sum(-1, keepdim=True)
    l1 = torch.where(l > 0, l, torch.ones_like(l))
    kf32 = keep.float()
    O = (((E.to(dt).float() * kf32) @ vf) / l1 * rs).to(dt)
    Pn = E / l1
    Pn16 = Pn.to(dt).float()
    dV = (((Pn16 * kf32).transpose(-1, -2) @ gf) * rs).to(dt)
    dP = (gf @ vf.transpose(-1, -2)) * kf32 * rs
    delta = (gf * O.float()).sum(-1, keepdim=True)
    dS = (Pn * (dP - delta)).to(dt).float()
    dQ = ((dS @ kf) * scale).to(dt)
    dK = ((dS.transpose(-1, -2) @ qf) * scale).to(dt)
    return O.double(), dQ.double(), dK.double(), dV.double()


def error_and_bar(got, true, emulated, tol):
    """The bar rule: (err, err_emu, bar) with bar = max(2 * err_emu, tol * max(1, max|true|))."""
    err, err_emu = (got.double() - true).abs().max().item(), (emulated - true).abs().max().item()
    return err, err_emu, max(2 * err_emu, tol * max(1.0, true.abs().max().item()))


def keep_block(seed, p, H, b, h, i0, i1, j0, j1):
    """The host's keep mask of the rectangle [i0, i1) x [j0, j1) of (b, h) in a call with H query heads: CPU bool [i1 - i0, j1 - j0].  p = 0: ones."""
    if i1 <= i0 or j1 <= j0:
        return torch.ones((max(i1 - i0, 0), max(j1 - j0, 0)), dtype=torch.bool)
    if p == 0:
        return torch.ones((i1 - i0, j1 - j0), dtype=torch.bool)
    out = torch.empty((i1 - i0, j1 - j0), dtype=torch.uint8)
    _fa2_lib.check(_fa2_lib.load().fa2_dropout_keep_mask(int(seed), float(p), int(H), int(b), int(h), i0, i1, j0, j1, out.data_ptr()))
    return out.bool()


_POOL = []


def _heads(fn, n):
    """[fn(0), ..., fn(n - 1)], the heads in parallel: the host's mask function is one Philox call per element and runs without the interpreter lock."""
    if n < 2:
        return [fn(h) for h in range(n)]
    if not _POOL:
        _POOL.append(concurrent.futures.ThreadPoolExecutor(max_workers=8))
    return list(_POOL[0].map(fn, range(n)))


def keep_unit(seed, p, H, b, nq, nk, i0=0, hmap=None):
    """[H, nq, nk] keep mask of batch / sequence b (rows counted from i0; hmap: (heads of the mask call, head of query head h) — the mutants' knobs)."""
    Hm, hof = (H, lambda h: h) if hmap is None else hmap
    return torch.stack(_heads(lambda h: keep_block(seed, p, Hm, b, hof(h), i0, i0 + nq, 0, nk), H))


# ---------------------------------------------------------------------------------------------------------------- the draw (pure Python)
def _window_edge(rng, Nkv):
    return rng.choice(WINDOW_EDGES + [rng.randint(0, max(Nkv, 1))])


def _draw_window(rng, Nkv):
    if rng.random() < 0.3:
        return None
    return [_window_edge(rng, Nkv), _window_edge(rng, Nkv)]


def _draw_dropout(rng, always=False):
    p = 0.0 if (not always and rng.random() < 0.35) else rng.choice(DROPOUT_PS)
    seed = rng.choice([0, rng.getrandbits(31), 2 ** 32, (1 << 63) | rng.getrandbits(63)])
    return p, seed


def _draw_scale_mul(rng):
    r = rng.random()
    return -1.0 if r < 0.1 else rng.choice([0.25, 3.0]) if r < 0.2 else 1.0


def _draw_heads(rng, choices=HEAD_COUNTS):
    H = rng.choice(choices)
    return H, rng.choice([d for d in range(1, H + 1) if H % d == 0])


def _draw_layout(rng, names):
    name = rng.choice(names)
    return [name, 8 * rng.randint(1, 4) if name == "rowpad" else rng.randint(1, 3) if name == "headslice" else 0]


def _draw_dense(i, rng, long):
    dtype = rng.choice(["float16", "bfloat16"])
    if long:            # dropout far from row 0 and key 0, several workgroups per head
        D = rng.choice([64, 128, 256])
        Nq, Nkv = rng.randint(513, 1500), rng.randint(1025, 2100)
        B, (H, Hkv) = rng.randint(1, 2), _draw_heads(rng, [1, 2, 4])
    else:
        D = rng.choice(fzp.HEAD_DIMS)
        nmax = 1500 if D <= 128 else 700 if D <= 256 else 300
        pick = lambda: rng.choice(fzp.EDGE_LENGTHS + [1023, 1024, 1025]) if rng.random() < 0.35 else rng.randint(1, nmax)  # noqa: E731
        Nq, Nkv = pick(), pick()
        if rng.random() < 0.4:
            Nkv = Nq
        B, (H, Hkv) = rng.randint(1, 3), _draw_heads(rng)
    causal = rng.random() < 0.4
    window = _draw_window(rng, Nkv)
    q_offset = rng.choice([0, max(Nkv - Nq, 0), rng.randint(0, Nkv + 70)])
    p, seed = _draw_dropout(rng, always=long)
    layouts = [_draw_layout(rng, ["contig", "bnhd_view", "rowpad", "headslice"]) for _ in range(3)]
    return dict(i=i, mode="dense", long=long, dtype=dtype, D=D, B=B, H=H, Hkv=Hkv, Nq=Nq, Nkv=Nkv, causal=causal, window=window, q_offset=q_offset, p=p,
                seed=seed, bnhd=rng.random() < 0.5, layouts=layouts, scale_mul=_draw_scale_mul(rng), dist=rng.choice(["rand", "randn"]),
                rows=rng.choice([0, 128, 256]), bwd=False, twice=i % 4 == 0)


def _draw_packed(i, rng, long):
    dtype = rng.choice(["float16", "bfloat16"])
    D = rng.choice([64, 128, 256]) if long else rng.choice(fzp.HEAD_DIMS)
    nseq = rng.randint(1, 4) if long else rng.randint(1, 8)
    one = lambda: rng.choice(PACKED_LENGTHS) if rng.random() < 0.4 else rng.randint(0, 150 if long else 300 if D > 256 else 600)  # noqa: E731
    lens_q = [one() for _ in range(nseq)]
    same = rng.random() < 0.5
    lens_k = list(lens_q) if same else [one() for _ in range(nseq)]
    if long:
        s = rng.randrange(nseq)
        lens_q[s], lens_k[s] = rng.randint(513, 1500), rng.randint(1025, 1500)
    elif D <= 256 and rng.random() < 0.3:       # at most one long sequence per case
        s = rng.randrange(nseq)
        lens_q[s] = rng.randint(601, 1500)
        lens_k[s] = lens_q[s] if same else rng.randint(601, 1500)
    H, Hkv = _draw_heads(rng, [1, 2, 4] if long else HEAD_COUNTS)
    causal, bottom_right = rng.choice([(False, False), (True, False), (True, True), (False, True)])
    window = _draw_window(rng, max(lens_k))
    p, seed = _draw_dropout(rng, always=long)
    layouts = [_draw_layout(rng, ["contig", "rowpad", "headslice"]) for _ in range(3)]
    return dict(i=i, mode="packed", long=long, dtype=dtype, D=D, H=H, Hkv=Hkv, lens_q=lens_q, lens_k=lens_k, causal=causal, bottom_right=bottom_right,
                window=window, p=p, seed=seed, max_kind=rng.choice(["exact", "round64", "none"]), layouts=layouts,
                surplus=rng.randint(1, 70) if rng.random() < 0.25 else 0, scale_mul=_draw_scale_mul(rng), dist=rng.choice(["rand", "randn"]),
                rows=rng.choice([0, 128, 256]), bwd=False, twice=i % 4 == 0)


def _draw_readback(i, rng):
    """One pass, one block of BITS * D keys (forward, dQ pass) or rows (dK / dV pass).  The pass, dense / packed and the kind of block start cycle with i,
    so that any 24 consecutive draws hold every combination."""
    pass_, packed, start_kind = READBACK_PASSES[i % 3], (i // 3) % 2 == 1, READBACK_STARTS[(i // 6) % 4]
    D = rng.choice(READBACK_DIMS)
    axis_base = 512 if pass_ == "dkv" else 1024          # the axis the block lies on: rows for the dK / dV pass, keys otherwise
    if start_kind == "zero":
        L, start = rng.randint(1, 700), 0
    elif start_kind == "last_partial":
        t, r = rng.randint(0, 9), rng.randint(1, 63)
        L, start = 64 * t + r, 64 * t + rng.randint(0, r - 1)
    elif start_kind == "beyond":
        start = axis_base + rng.randint(1, 200)
        L = start + rng.randint(1, 300)
    else:
        L = rng.randint(2, 900)
        start = rng.randint(0, L - 1)
    M = rng.randint(1, 300)                              # the other axis
    Nq, Nkv = (L, M) if pass_ == "dkv" else (M, L)
    H, Hkv = _draw_heads(rng, [1, 2, 4])
    d = dict(i=i, mode="readback", packed=packed, pass_=pass_, start_kind=start_kind, start=start, dtype=rng.choice(["float16", "bfloat16"]), D=D,
             H=H, Hkv=Hkv, member=rng.randrange(H // Hkv), p=rng.choice([0.1, 0.5]), seed=_draw_dropout(rng, True)[1], rows=rng.choice([0, 128, 256]),
             causal=False, bottom_right=False, window=None, q_offset=0)
    if pass_ == "fwd":                                   # any band; the backward passes are read under the full band
        d["causal"] = rng.random() < 0.3
        d["window"] = _draw_window(rng, Nkv) if rng.random() < 0.6 else None
        if packed:
            d["bottom_right"] = rng.random() < 0.5
        else:
            d["q_offset"] = rng.choice([0, max(Nkv - Nq, 0), rng.randint(0, Nkv)])
    if packed:
        nseq = rng.randint(2, 4)
        s = rng.randrange(nseq)
        d["lens_q"] = [Nq if t == s else rng.choice([0, 1, rng.randint(1, 200)]) for t in range(nseq)]
        d["lens_k"] = [Nkv if t == s else rng.choice([1, rng.randint(1, 300), rng.randint(1, 300)]) for t in range(nseq)]
    else:
        d.update(B=rng.randint(1, 2), Nq=Nq, Nkv=Nkv, bnhd=rng.random() < 0.5)
    return d


def draw_case(i, rng, force=None):
    """Case i of a sweep as a dict that describes the call completely; force: None | "dense" | "packed" | "dropout_long" | "readback".  Pure Python."""
    if force == "readback":
        return _draw_readback(i, rng)
    if force == "dropout_long":
        return _draw_packed(i, rng, True) if rng.random() < 0.3 else _draw_dense(i, rng, True)
    if force == "packed" or (force is None and rng.random() < 0.4):
        return _draw_packed(i, rng, False)
    return _draw_dense(i, rng, False)


def draw_sweep(seed, counts, bwd_every=2):
    """The cases of a sweep: counts = [(force, n), ...] drawn in that order from one generator; every bwd_every-th case of a family runs the backward."""
    rng = random.Random(seed)
    out = []
    for force, n in counts:
        for j in range(n):
            d = draw_case(len(out), rng, force)
            d["bwd"] = d["mode"] != "readback" and bwd_every > 0 and j % bwd_every == 0
            out.append(d)
    return out


SLICE_SEED, SLICE_COUNTS = 7, [("dense", 60), ("packed", 40), ("dropout_long", 12)]           # tests/test_fuzz_gpu.py::test_randomised_feature_sweep_slice
READBACK_SEED, READBACK_COUNTS = 7, [("readback", 24)]                                        # ... ::test_dropout_mask_readback_all_passes_slice


def units_of(desc):
    """The (batch or sequence) units of a call: [(nq, nk, left, right, off)], right with the causal flag folded in; the list index is the mask's b."""
    left, right = desc["window"] if desc["window"] is not None else (-1, -1)
    if desc["causal"]:
        right = 0
    if "lens_q" in desc:
        return [(nq, nk, left, right, nk - nq if desc["bottom_right"] else 0) for nq, nk in zip(desc["lens_q"], desc["lens_k"])]
    return [(desc["Nq"], desc["Nkv"], left, right, desc["q_offset"])] * desc["B"]


def _row_dead(i, nk, left, right, off):
    lo = 0 if left < 0 else max(0, i + off - left)
    hi = nk - 1 if right < 0 else min(nk - 1, i + off + right)
    return lo > hi


def has_dead_rows(desc):
    return any(nq > 0 and (_row_dead(0, nk, l, r, off) or _row_dead(nq - 1, nk, l, r, off)) for nq, nk, l, r, off in units_of(desc))


def family(D):
    return 64 if D <= 64 else 128 if D <= 128 else 256 if D <= 256 else 512


def coverage(descs):
    """What a list of drawn cases reaches, as counts by name (the slices of tests/test_fuzz_gpu.py must have every one of them >= 1)."""
    c = {}

    def hit(name, cond=True):
        c[name] = c.get(name, 0) + int(bool(cond))
    for d in descs:
        if d["mode"] == "readback":
            for ps in READBACK_PASSES:
                for pk in (False, True):
                    hit("readback %s %s" % (ps, "packed" if pk else "dense"), d["pass_"] == ps and d["packed"] == pk)
            hit("readback block beyond key 1024", d["pass_"] != "dkv" and d["start"] > 1024)
            hit("readback block beyond row 512", d["pass_"] == "dkv" and d["start"] > 512)
            hit("readback block inside the last partial tile", d["start_kind"] == "last_partial")
            hit("readback off-family head dim", family(d["D"]) != d["D"])
            continue
        drop, units, packed = d["p"] > 0, units_of(d), d["mode"] == "packed"
        for f in (64, 128, 256, 512):
            hit("family %d with a backward" % f, family(d["D"]) == f and d["bwd"])
            hit("family %d off-family head dim under dropout" % f, family(d["D"]) == f and d["D"] != f and drop)
        for r in (128, 256):
            hit("rows %d under dropout" % r, d["rows"] == r and drop)
        hit("group >= 4 with dropout and a backward", d["H"] // d["Hkv"] >= 4 and drop and d["bwd"])
        edge = False
        if not packed and d["window"] is not None and d["q_offset"] > 0:
            _, nk, l, r, off = units[0]
            edge = (l >= 0 and 0 < off - l < nk and (off - l) % 64) or (r >= 0 and off + r + 1 < nk and (off + r + 1) % 64)
        hit("dense window with q_offset > 0 and a band edge inside a 64-key tile", edge)
        hit("dead rows, %s" % d["mode"], has_dead_rows(d))
        hit("zero-length sequence on the q side", packed and any(u[0] == 0 and u[1] > 0 for u in units))
        hit("zero-length sequence on the k side", packed and any(u[1] == 0 and u[0] > 0 for u in units))
        hit("bottom-right with fewer keys than queries", packed and d["bottom_right"] and (d["causal"] or d["window"] is not None) and
            any(0 < u[1] < u[0] for u in units))
        hit("packed with window, dropout and a backward", packed and d["window"] is not None and drop and d["bwd"])
        hit("row-padded or head-sliced input under dropout", drop and any(l[0] in ("rowpad", "headslice") for l in d["layouts"]))
        hit("dropout threshold 0", drop and threshold(d["p"]) == 0)
        hit("dropout threshold 1", threshold(d["p"]) == 1)
        hit("seed >= 2^32", drop and d["seed"] >= 2 ** 32)
        hit("dropout beyond row 512 and key 1024", drop and any(u[0] > 512 and u[1] > 1024 for u in units))
        hit("packed surplus NaN rows", packed and d["surplus"] > 0)
        hit("scale other than D^-0.5 on a windowed, packed or dropout call", d["scale_mul"] != 1.0 and (packed or drop or d["window"] is not None))
    return c


def shrink(desc, nmax):
    """The same call with every length capped at nmax and at most two batches (tests/test_fuzz_features.py: the checker on the CPU)."""
    d = dict(desc)
    if "lens_q" in d:
        d["lens_q"], d["lens_k"] = [min(n, nmax) for n in d["lens_q"]], [min(n, nmax) for n in d["lens_k"]]
    else:
        d["Nq"], d["Nkv"], d["B"] = min(d["Nq"], nmax), min(d["Nkv"], nmax), min(d["B"], 2)
        d["q_offset"] = min(d["q_offset"], d["Nkv"] + 70)
    return d


# ---------------------------------------------------------------------------------------------------------------- tensors of a case
def _draw_tensor(shape, gen, device, dist):
    return (torch.randn if dist == "randn" else torch.rand)(*shape, generator=gen, device=device)


def _dense_tensor(shape, dt, layout, gen, device, dist):
    """fuzz_parity.make()'s four layouts of a [B, H, N, D] tensor, the padding and the extra heads taken from the description."""
    (B, H, N, D), (name, par) = shape, layout
    if name == "contig":
        return _draw_tensor((B, H, N, D), gen, device, dist).to(dt)
    if name == "bnhd_view":
        return _draw_tensor((B, N, H, D), gen, device, dist).to(dt).permute(0, 2, 1, 3)
    if name == "rowpad":
        return _draw_tensor((B, H, N, D + par), gen, device, dist).to(dt)[..., :D]
    if name == "headslice":
        return _draw_tensor((B, H + par, N, D), gen, device, dist).to(dt)[:, par // 2: par // 2 + H]
    raise ValueError(name)


def _packed_tensor(shape, dt, layout, gen, device, dist):
    (T, H, D), (name, par) = shape, layout
    if name == "contig":
        return _draw_tensor((T, H, D), gen, device, dist).to(dt)
    if name == "rowpad":
        return _draw_tensor((T, H, D + par), gen, device, dist).to(dt)[..., :D]
    if name == "headslice":
        return _draw_tensor((T, H + par, D), gen, device, dist).to(dt)[:, par // 2: par // 2 + H]
    raise ValueError(name)


def scale_of(desc):
    return desc["D"] ** -0.5 * desc.get("scale_mul", 1.0)


def build_inputs(desc, gen):
    """The tensors of a dense or packed case on gen's device: q, k, v, do as the operator takes them (packed: with the surplus NaN rows), and per
    unit the views [H, nq, D] / [Hkv, nk, D] of them."""
    dev, dt, D, H, Hkv = gen.device, getattr(torch, desc["dtype"]), desc["D"], desc["H"], desc["Hkv"]
    inp = dict(units=[])
    if desc["mode"] == "dense":
        B, Nq, Nkv = desc["B"], desc["Nq"], desc["Nkv"]
        q = _dense_tensor((B, H, Nq, D), dt, desc["layouts"][0], gen, dev, desc["dist"])
        k = _dense_tensor((B, Hkv, Nkv, D), dt, desc["layouts"][1], gen, dev, desc["dist"])
        v = _dense_tensor((B, Hkv, Nkv, D), dt, desc["layouts"][2], gen, dev, desc["dist"])
        do = torch.randn(B, H, Nq, D, generator=gen, device=dev).to(dt)
        inp.update(q=q, k=k, v=v, do=do)
        inp["units"] = [dict(q=q[b], k=k[b], v=v[b], do=do[b]) for b in range(B)]
        return inp
    tq, tk, sp = sum(desc["lens_q"]), sum(desc["lens_k"]), desc["surplus"]
    q = _packed_tensor((tq + sp, H, D), dt, desc["layouts"][0], gen, dev, desc["dist"])
    k = _packed_tensor((tk + sp, Hkv, D), dt, desc["layouts"][1], gen, dev, desc["dist"])
    v = _packed_tensor((tk + sp, Hkv, D), dt, desc["layouts"][2], gen, dev, desc["dist"])
    do = torch.randn(tq + sp, H, D, generator=gen, device=dev).to(dt)
    if sp:                                               # rows behind cu[B] belong to nobody: nothing of them may reach an output below cu[B]
        for t, n in ((q, tq), (k, tk), (v, tk), (do, tq)):
            t[n:] = float("nan")
    inp.update(q=q, k=k, v=v, do=do, total_q=tq, total_k=tk)
    q0 = k0 = 0
    for nq, nk in zip(desc["lens_q"], desc["lens_k"]):
        hm = lambda t, a, n: t[a:a + n].transpose(0, 1)                          # noqa: E731 - [n, heads, D] -> [heads, n, D]
        inp["units"].append(dict(q=hm(q, q0, nq), k=hm(k, k0, nk), v=hm(v, k0, nk), do=hm(do, q0, nq), q0=q0, k0=k0))
        q0, k0 = q0 + nq, k0 + nk
    return inp


def truths(desc, inp, folded=None):
    """Per unit: the band, the keep mask, float64 truth and the emulation (None for a unit without queries or without keys).  folded: bool [B, H] of
    the heads a dense launch served with scale * log2(e) folded into Q — those are held to the truth of that contract (fuzz_parity.prescaled_q)."""
    dt, H, g, scale, p, out = getattr(torch, desc["dtype"]), desc["H"], desc["H"] // desc["Hkv"], scale_of(desc), desc["p"], []
    for b, (u, (nq, nk, left, right, off)) in enumerate(zip(inp["units"], units_of(desc))):
        if nq == 0 or nk == 0:
            out.append(None)
            continue
        dev = u["q"].device
        bd = band(nq, nk, left, right, off, False, dev)
        keep = keep_unit(desc["seed"], p, H, b, nq, nk).to(dev)
        q, sc = u["q"], scale
        if folded is not None and folded[b].any():
            qs, s_alt = fzp.prescaled_q(q, scale, dt)
            q = torch.where(folded[b][:, None, None], qs, q)
            sc = torch.where(folded[b], torch.tensor(s_alt, dtype=torch.float64, device=dev), torch.tensor(scale, dtype=torch.float64, device=dev))[:, None, None]
        ke, ve = u["k"].repeat_interleave(g, 0), u["v"].repeat_interleave(g, 0)
        true = ref64(q, ke, ve, u["do"], keep, bd, sc, p)
        em = emu(q, ke, ve, u["do"], keep, bd, sc if not torch.is_tensor(sc) else sc.float(), p, dt)
        out.append(dict(band=bd, keep=keep, true=true, emu=em, q=q, ke=ke, ve=ve, scale=sc))
    return out


def fold_groups(t, Hkv):
    """dK / dV of expanded heads [H, n, D] summed per group -> [Hkv, n, D]."""
    return t.unflatten(0, (Hkv, t.shape[0] // Hkv)).sum(1)


def emulate(desc, inp, tr, mutate=None):
    """The emulation's outputs in the shape of the operator's (per unit: O, lse, dQ, dK, dV) — "the kernel's output" of the CPU tests.  mutate(b, unit of
    truths()) -> dict(band=, keep=, rs=) replaces what the emulation is given (a wrong kernel); None: the emulation as it is."""
    dt, Hkv, p, got = getattr(torch, desc["dtype"]), desc["Hkv"], desc["p"], []
    for b, (u, t, (nq, nk, *_)) in enumerate(zip(inp["units"], tr, units_of(desc))):
        if t is None:
            z = lambda n, h: torch.zeros(h, n, desc["D"], dtype=dt)             # noqa: E731
            got.append(dict(O=z(nq, desc["H"]), lse=torch.full((desc["H"], nq), float("-inf")), dQ=z(nq, desc["H"]), dK=z(nk, Hkv), dV=z(nk, Hkv)))
            continue
        m = dict(band=t["band"], keep=t["keep"], rs=None)
        if mutate is not None:
            m.update(mutate(b, t))
        sc = t["scale"].float() if torch.is_tensor(t["scale"]) else t["scale"]
        O, dQ, dK, dV = emu(t["q"], t["ke"], t["ve"], u["do"], m["keep"], m["band"], sc, p, dt, rs=m["rs"])
        lse = t["true"][1] if m["band"] is t["band"] else ref64(t["q"], t["ke"], t["ve"], u["do"], m["keep"], m["band"], t["scale"], p)[1]
        got.append(dict(O=O.to(dt), lse=lse.float(), dQ=dQ.to(dt), dK=fold_groups(dK, Hkv).to(dt), dV=fold_groups(dV, Hkv).to(dt)))
    return got


def check_units(desc, inp, tr, got, plan=None):
    """The checks of one case on the outputs `got` (per unit: O, lse, and with a backward dQ, dK, dV): -> (fails, figures)."""
    dt, Hkv, fails, fig = getattr(torch, desc["dtype"]), desc["Hkv"], [], dict(o_ratio=0.0, grad_ratio=0.0, lse_err=0.0)
    real = [u for u, t in zip(inp["units"], tr) if t is not None]
    lse_lim = None
    if real:
        plan = plan if plan is not None else _fa2_lib.FwdPlan()
        qs, ks = torch.cat([u["q"].reshape(-1) for u in real]), torch.cat([u["k"].reshape(-1) for u in real])
        lse_lim = fzp.lse_limit(plan, qs, ks, desc["D"], scale_of(desc), dt)
    names = ("O", "dQ", "dK", "dV") if desc["bwd"] else ("O",)
    for b, (t, g, (nq, nk, *_)) in enumerate(zip(tr, got, units_of(desc))):
        tag = "unit %d (%d x %d)" % (b, nq, nk)
        for n in names + ("lse",):
            x = g[n].float()
            if n == "lse":
                x = torch.where(torch.isneginf(x), torch.zeros_like(x), x)
            if not torch.isfinite(x).all():
                fails.append("%s: %s non-finite" % (tag, n))
        if fails:
            continue
        if t is None:       # no queries or no keys: nothing flows
            if any((g[n] != 0).any() for n in names) or not torch.isneginf(g["lse"]).all():
                fails.append("%s: an empty side must give zeros and LSE = -inf" % tag)
            continue
        O, lse, dQ, dK, dV = t["true"]
        eO, edQ, edK, edV = t["emu"]
        pairs = [("O", O, eO, FLOOR[dt])]
        if desc["bwd"]:
            pairs += [("dQ", dQ, edQ, GRAD_TOL[dt]), ("dK", fold_groups(dK, Hkv), fold_groups(edK, Hkv), GRAD_TOL[dt]),
                      ("dV", fold_groups(dV, Hkv), fold_groups(edV, Hkv), GRAD_TOL[dt])]
        for n, true, em, tol in pairs:
            err, err_emu, bar = error_and_bar(g[n], true, em, tol)
            key = "o_ratio" if n == "O" else "grad_ratio"
            fig[key] = max(fig[key], err / bar)
            if not err <= bar:
                fails.append("%s: %s err %.3e > %.3e (emulation %.3e)" % (tag, n, err, bar, err_emu))
        dead = ~t["band"].any(-1)
        live = ~dead
        if dead.any():
            if (g["O"][:, dead] != 0).any() or not torch.isneginf(g["lse"][:, dead]).all() or (desc["bwd"] and (g["dQ"][:, dead] != 0).any()):
                fails.append("%s: rows that see no key must give O = dQ = 0 and LSE = -inf" % tag)
        if live.any():
            lerr = (g["lse"][:, live].double() - lse[:, live]).abs().max().item()
            fig["lse_err"] = max(fig["lse_err"], lerr)
            if not lerr <= lse_lim:
                fails.append("%s: LSE err %.3e > %.3e" % (tag, lerr, lse_lim))
    return fails, fig


# ---------------------------------------------------------------------------------------------------------------- running a case on the device
def _with_rows(rows, fn):
    lib = _fa2_lib.load()
    old = lib.fa2_get_option(b"rows")
    _fa2_lib.set_option("rows", rows)
    try:
        return fn()
    finally:
        _fa2_lib.set_option("rows", old)


def _bhnd(t, bnhd):
    return t.transpose(1, 2) if bnhd else t


def _call_dense(desc, inp):
    """-> (got per unit, plan, folded heads or None)."""
    from rocwmma_fattn.FlashAttn import flash_attention, flash_attn_wmma
    bnhd, scale, p, bwd = desc["bnhd"], scale_of(desc), desc["p"], desc["bwd"]
    B, H, Hkv, Nq, Nkv, D = (desc[n] for n in ("B", "H", "Hkv", "Nq", "Nkv", "D"))
    window = None if desc["window"] is None else tuple(desc["window"])
    kw = dict(causal=desc["causal"], scale=scale, BNHD_fmt=bnhd, window=window, q_offset=desc["q_offset"], dropout_p=float(p), dropout_seed=desc["seed"])
    qo, ko, vo, doo = (_bhnd(inp[n], bnhd) for n in ("q", "k", "v", "do"))                     # as the operator takes them
    grads = [None, None, None]
    if bwd:
        qg, kg, vg = (t.detach().requires_grad_(True) for t in (qo, ko, vo))                  # (leaves that keep the strides of the views)
        o = flash_attention(qg, kg, vg, **kw)
        o.backward(doo)
        o, grads = o.detach(), [qg.grad, kg.grad, vg.grad]
    else:
        o = flash_attention(qo, ko, vo, **kw)
    # the LSE and the plan of the same call through the extension's forward, flagged as the operator flags it
    left, right, off = _fa2_lib.parse_window(window, desc["q_offset"])
    flags = (_fa2_lib.FA2_FLAG_CAUSAL if desc["causal"] else 0) | (_fa2_lib.FA2_FLAG_EXACT_SCALE if bwd or p > 0 else 0)
    Br, plan = 32 if D > 384 else 64, _fa2_lib.FwdPlan()                                     # (a zeroed plan: contract 0, as the dropout calls are)
    if p > 0:
        ret = flash_attn_wmma.forward_py(qo, ko, vo, Br, 128, flags, scale, bnhd, window=(left, right, off), dropout=(p, desc["seed"]))
    elif window is not None or off:
        ret = flash_attn_wmma.forward_window(qo, ko, vo, Br, 128, flags, scale, bnhd, (left, right, off))
        plan = _fa2_lib.window_plan(_bhnd(ret[1], bnhd), _bhnd(ret[2], bnhd), flags, left, right, off, scale)
    else:
        ret = flash_attn_wmma.forward(qo, ko, vo, Br, 128, flags, scale, bnhd)
        qk, kk, code, lib = _bhnd(ret[1], bnhd), _bhnd(ret[2], bnhd), 0 if desc["dtype"] == "float16" else 1, _fa2_lib.load()
        if Hkv == H:
            ws = 0 if desc["causal"] else lib.fa2_fwd_workspace_bytes(code, B, H, Nq, Nkv, qk.shape[3], 0)
            plan = _fa2_lib.fwd_plan(qk, kk, flags, scale, workspace_bytes=ws)
        else:
            ws = 0 if desc["causal"] else lib.fa2_fwd_gqa_workspace_bytes(code, B, H, Hkv, Nq, Nkv, qk.shape[3], 0)
            plan = _fa2_lib.gqa_plan(qk, kk, flags, scale, workspace_bytes=ws)
    same = torch.equal(o, ret[0])
    lse = ret[5][:, :, :Nq]
    folded = None if flags & _fa2_lib.FA2_FLAG_EXACT_SCALE else fzp.folded_heads(plan, B, H, o.device)
    ob, gq, gk, gv = (None if t is None else _bhnd(t, bnhd) for t in [o] + grads)
    got = [dict(O=ob[b], lse=lse[b], dQ=gq[b], dK=gk[b], dV=gv[b]) if bwd else dict(O=ob[b], lse=lse[b]) for b in range(B)]
    return got, plan, folded, same


def _call_packed(desc, inp):
    from rocwmma_fattn.FlashAttn import flash_attention_varlen, flash_attn_wmma
    scale, p, bwd, dev = scale_of(desc), desc["p"], desc["bwd"], inp["q"].device
    window = None if desc["window"] is None else tuple(desc["window"])
    lq, lk = desc["lens_q"], desc["lens_k"]
    cu = lambda lens: torch.tensor([0] + [sum(lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32, device=dev)      # noqa: E731
    cu_q, cu_k = cu(lq), cu(lk)
    up = {"exact": lambda n: n, "round64": lambda n: -(-n // 64) * 64, "none": lambda n: None}[desc["max_kind"]]
    kw = dict(max_seqlen_q=up(max(lq)), max_seqlen_k=up(max(lk)), causal=desc["causal"], scale=scale, window=window, bottom_right=desc["bottom_right"],
              dropout_p=float(p), dropout_seed=desc["seed"])
    grads = [None, None, None]
    if bwd:
        qg, kg, vg = (inp[n].detach().requires_grad_(True) for n in ("q", "k", "v"))
        o = flash_attention_varlen(qg, kg, vg, cu_q, cu_k, **kw)
        o.backward(inp["do"])
        o, grads = o.detach(), [qg.grad, kg.grad, vg.grad]
    else:
        o = flash_attention_varlen(inp["q"], inp["k"], inp["v"], cu_q, cu_k, **kw)
    left, right, _ = _fa2_lib.parse_window(window, 0)
    flags = (_fa2_lib.FA2_FLAG_CAUSAL if desc["causal"] else 0) | (_fa2_lib.FA2_FLAG_BOTTOM_RIGHT if desc["bottom_right"] else 0)
    fl = flags | (_fa2_lib.FA2_FLAG_EXACT_SCALE if bwd else 0)
    mq, mk = (kw["max_seqlen_q"], kw["max_seqlen_k"]) if desc["max_kind"] != "none" else (max(lq), max(lk))
    ret = flash_attn_wmma.forward_varlen(inp["q"], inp["k"], inp["v"], cu_q, cu_k, mq, mk, fl, scale, (left, right), (p, desc["seed"]) if p > 0 else None)
    plan = _fa2_lib.varlen_plan(ret[1], ret[2], max(mq, 1), max(mk, 1), len(lq), fl, left, right, scale)
    tq = inp["total_q"]
    same = torch.equal(o[:tq], ret[0][:tq])
    lse, got = ret[5], []
    for u, nq, nk in zip(inp["units"], lq, lk):
        hm = lambda t, a, n: t[a:a + n].transpose(0, 1)                          # noqa: E731
        g = dict(O=hm(o, u["q0"], nq), lse=lse[:, u["q0"]:u["q0"] + nq])
        if bwd:
            g.update(dQ=hm(grads[0], u["q0"], nq), dK=hm(grads[1], u["k0"], nk), dV=hm(grads[2], u["k0"], nk))
        got.append(g)
    return got, plan, None, same


def _run_checked(desc, gen):
    inp = build_inputs(desc, gen)
    call = _call_packed if desc["mode"] == "packed" else _call_dense
    got, plan, folded, same = _with_rows(desc["rows"], lambda: call(desc, inp))
    out = dict(desc, plan=[plan.kernel, plan.contract, plan.heads_main, plan.kernel_tail, plan.contract_tail, plan.rows])
    fails, fig = check_units(desc, inp, truths(desc, inp, folded), got, plan)
    if not same:
        fails.append("operator and extension forward differ bit-wise")
    if desc["twice"]:    # the same call on the same inputs once more: every output bit for bit
        got2 = _with_rows(desc["rows"], lambda: call(desc, inp))[0]
        for b, (g, g2) in enumerate(zip(got, got2)):
            for n in g:
                if not torch.equal(g[n], g2[n]):
                    fails.append("unit %d: %s differs between two runs" % (b, n))
    out.update(fig, fails=fails)
    return out


# ---------------------------------------------------------------------------------------------------------------- readback
def readback_inputs(desc, gen):
    """The tensors of a readback call (module docstring; per unit [heads, n, D] like build_inputs) and the geometry the decode needs."""
    dev, dt, D, H, Hkv, s0, ps = gen.device, getattr(torch, desc["dtype"]), desc["D"], desc["H"], desc["Hkv"], desc["start"], desc["pass_"]
    g, units = H // Hkv, []
    for nq, nk, *_ in units_of(desc):
        q = torch.randn(H, nq, D, generator=gen, device=dev).to(dt)
        k = torch.zeros(Hkv, nk, D, dtype=dt, device=dev)
        v = torch.randn(Hkv, nk, D, generator=gen, device=dev).to(dt)
        do = torch.randn(H, nq, D, generator=gen, device=dev).to(dt)
        code = torch.zeros(nq if ps == "dkv" else nk, D, dtype=dt, device=dev)               # one-hot rows: element (start + g * D + c, c) = 2^g inside the block
        x = torch.arange(min(s0, code.shape[0]), min(s0 + BITS * D, code.shape[0]), device=dev)
        if x.numel():
            code[x, (x - s0) % D] = (2.0 ** ((x - s0) // D)).to(dt)
        e0 = torch.zeros(D, dtype=dt, device=dev)
        e0[0] = 1
        if ps == "fwd":
            v = code.expand(Hkv, nk, D).contiguous()
        elif ps == "dkv":                                # one query head of each group carries the coded dO: dV of a group is then that head's alone
            do = torch.zeros(H, nq, D, dtype=dt, device=dev)
            do[desc["member"]::g] = code
        else:
            q = torch.zeros(H, nq, D, dtype=dt, device=dev)
            k = code.expand(Hkv, nk, D).contiguous()
            v, do = e0.expand(Hkv, nk, D).contiguous(), e0.expand(H, nq, D).contiguous()
        units.append(dict(q=q, k=k, v=v, do=do, colsum=code.float().sum(0)))
    return units


def readback_decode(desc, units, got):
    """The keep bits a readback call's outputs hold against the host's mask: -> (wrong bits, compared bits, largest distance of a count from an integer).
    got per unit: O [H, nq, D] and, for the backward passes, dQ [H, nq, D] / dV [Hkv, nk, D]."""
    D, H, Hkv, s0, ps, p, seed = desc["D"], desc["H"], desc["Hkv"], desc["start"], desc["pass_"], desc["p"], desc["seed"]
    g, rs, scale = H // Hkv, 1.0 / (1.0 - p_eff(p)), scale_of(desc)
    wrong = total = 0
    frac = 0.0
    for b, (u, o, (nq, nk, left, right, off)) in enumerate(zip(units, got, units_of(desc))):
        if nq == 0 or nk == 0:
            continue
        if ps == "fwd":
            bd = band(nq, nk, left, right, off, False)
            cnt = bd.sum(-1).clamp(min=1).double()
            n = o["O"].double().cpu() * cnt[None, :, None] / rs                                  # [H, nq, D]
            w = min(BITS * D, nk - s0)
            want = torch.zeros(H, nq, BITS * D, dtype=torch.bool)
            if w > 0:
                want[:, :, :w] = torch.stack(_heads(lambda h: keep_block(seed, p, H, b, h, 0, nq, s0, s0 + w), H)) & bd[None, :, s0:s0 + w]
        elif ps == "dq":
            delta = o["O"].double().cpu()[:, :, :1]                                            # dO = e_0: delta_i = O[i, 0], the device's own
            n = (o["dQ"].double().cpu() * (nk / scale) + delta * u["colsum"].double().cpu()) / rs
            w = min(BITS * D, nk - s0)
            want = torch.zeros(H, nq, BITS * D, dtype=torch.bool)
            if w > 0:
                want[:, :, :w] = torch.stack(_heads(lambda h: keep_block(seed, p, H, b, h, 0, nq, s0, s0 + w), H))
        else:
            n = o["dV"].double().cpu() * (nk / rs)                                               # [Hkv, nk, D]
            w = min(BITS * D, nq - s0)
            want = torch.zeros(Hkv, nk, BITS * D, dtype=torch.bool)
            if w > 0:
                want[:, :, :w] = torch.stack(_heads(lambda hk: keep_block(seed, p, H, b, hk * g + desc["member"], s0, s0 + w, 0, nk).t(), Hkv))
        if not torch.isfinite(n).all():
            return 1, 1, float("inf")
        frac = max(frac, (n - n.round()).abs().max().item())
        ni = n.round().long()
        if (ni < 0).any() or (ni >= 2 ** BITS).any():
            wrong += int(((ni < 0) | (ni >= 2 ** BITS)).sum())
            ni = ni.clamp(0, 2 ** BITS - 1)
        dec = torch.cat([((ni >> gi) & 1).bool() for gi in range(BITS)], dim=-1)             # bit g of column c: element start + g * D + c of the block
        wrong += int((dec != want).sum())
        total += want.numel()
    return wrong, total, frac


def readback_emulate(desc, units, flip=None):
    """The emulation's outputs of a readback call (CPU).  flip = (b, h, i, j): that one keep bit inverted — a kernel with one wrong mask bit."""
    dt, H, g, p, scale, got = getattr(torch, desc["dtype"]), desc["H"], desc["H"] // desc["Hkv"], desc["p"], scale_of(desc), []
    for b, (u, (nq, nk, left, right, off)) in enumerate(zip(units, units_of(desc))):
        if nq == 0 or nk == 0:
            got.append(None)
            continue
        keep = keep_unit(desc["seed"], p, H, b, nq, nk)
        if flip is not None and flip[0] == b:
            keep[flip[1], flip[2], flip[3]] ^= True
        O, dQ, _, dV = emu(u["q"], u["k"].repeat_interleave(g, 0), u["v"].repeat_interleave(g, 0), u["do"], keep, band(nq, nk, left, right, off, False),
                           scale, p, dt)
        got.append(dict(O=O.to(dt), dQ=dQ.to(dt), dV=fold_groups(dV, desc["Hkv"]).to(dt)))
    return got


def _call_readback(desc, units):
    from rocwmma_fattn.FlashAttn import flash_attention, flash_attention_varlen
    bwd, dev = desc["pass_"] != "fwd", units[0]["q"].device
    window = None if desc["window"] is None else tuple(desc["window"])
    if desc["packed"]:
        q, k, v, do = (torch.cat([u[n].transpose(0, 1) for u in units]).contiguous() for n in ("q", "k", "v", "do"))
        lq, lk = desc["lens_q"], desc["lens_k"]
        cu = lambda lens: torch.tensor([0] + [sum(lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32, device=dev)      # noqa: E731
        run = lambda a, b, c: flash_attention_varlen(a, b, c, cu(lq), cu(lk), max(lq), max(lk), causal=desc["causal"], window=window,      # noqa: E731
                                                     bottom_right=desc["bottom_right"], dropout_p=desc["p"], dropout_seed=desc["seed"])
    else:
        bnhd = desc["bnhd"]
        q, k, v, do = (_bhnd(torch.stack([u[n] for u in units]), bnhd).contiguous() for n in ("q", "k", "v", "do"))
        run = lambda a, b, c: flash_attention(a, b, c, causal=desc["causal"], BNHD_fmt=bnhd, window=window, q_offset=desc["q_offset"],      # noqa: E731
                                              dropout_p=desc["p"], dropout_seed=desc["seed"])
    if bwd:
        q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    o = run(q, k, v)
    outs = dict(O=o.detach())
    if bwd:
        o.backward(do)
        outs.update(dQ=q.grad, dV=v.grad)
    got, q0, k0 = [], 0, 0
    for b, (nq, nk, *_) in enumerate(units_of(desc)):
        if desc["packed"]:
            cut = lambda n, a, m: outs[n][a:a + m].transpose(0, 1)                # noqa: E731
            got.append({n: cut(n, k0 if n == "dV" else q0, nk if n == "dV" else nq) for n in outs})
            q0, k0 = q0 + nq, k0 + nk
        else:
            got.append({n: _bhnd(outs[n], desc["bnhd"])[b] for n in outs})
    return got


def _run_readback(desc, gen):
    units = readback_inputs(desc, gen)
    got = _with_rows(desc["rows"], lambda: _call_readback(desc, units))
    wrong, total, frac = readback_decode(desc, units, got)
    fails = []
    if wrong:
        fails.append("%d of %d mask bits of the %s pass differ from the host's" % (wrong, total, desc["pass_"]))
    if not frac <= 0.25:
        fails.append("decode not exact: a count lies %.3f from an integer" % frac)
    return dict(desc, bits=total, frac=frac, fails=fails)


def run_case(desc, gen):
    """Build the tensors of a drawn case on gen's device, run the operator, check: desc plus the figures and `fails`."""
    return _run_readback(desc, gen) if desc["mode"] == "readback" else _run_checked(desc, gen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--bwd-every", type=int, default=2, help="every n-th case also runs the backward (0 = never)")
    ap.add_argument("--mode", default="dense", choices=MODES)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(args.seed)
    bad, worst, n_bwd, bits = [], dict(o_ratio=0.0, grad_ratio=0.0, lse_err=0.0, frac=0.0), 0, 0
    for desc in draw_sweep(args.seed, [(args.mode, args.cases)], args.bwd_every):
        try:
            d = run_case(desc, gen)
        except Exception as e:                      # a refused shape or a launch error is a finding too
            d = dict(desc, fails=["exception: %r" % (e,)])
        n_bwd += int(desc["bwd"] or (desc["mode"] == "readback" and desc["pass_"] != "fwd"))
        bits += d.get("bits", 0)
        for key in worst:
            worst[key] = max(worst[key], d.get(key, 0.0))
        if d["fails"]:
            bad.append(d)
            print("FAIL", json.dumps(d), flush=True)
    summary = dict(tool="fuzz_features", mode=args.mode, cases=args.cases, backward_cases=n_bwd, seed=args.seed, failures=len(bad),
                   worst_o_err_over_bar=worst["o_ratio"], worst_grad_err_over_bar=worst["grad_ratio"], worst_lse_err=worst["lse_err"],
                   readback_bits=bits, readback_worst_distance_from_integer=worst["frac"], device=torch.cuda.get_device_name(0), failing=bad)
    line = json.dumps(summary)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
