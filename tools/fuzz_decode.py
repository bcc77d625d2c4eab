"""Randomised float64 sweep of the KV-cache serving path (developer tool; the long runs are recorded in profiles/fuzz_runs.md).

tools/fuzz_features.py draws the dense and packed calls; this tool draws what it never passes: the decode and append entries.  Three families (--mode,
draw_case's `force`):
    decode   one call of fa2_fwd_decode_window through _fa2_lib (the superset entry reaches the plain, the e4m3 and the banded kernels): drawn dtype,
             head dim, heads, rows per K / V head, batch, contiguous capacity or page size / table width, lengths at the edges of Nq, the 32-key tile,
             the page and the capacity, window / softcap / slopes / scale, 16-bit or e4m3 cache with general descales, split, strided views; paged
             caches in shuffled physical order with a block-table stride wider than the table and, in a third of the cases, two sequences that share
             their leading pages.  NaN (0x7f) in every slot no row may see.  Against tests/decode_window_refs.py's float64 and emulation under its bars.
    append   one call of kvcache_append: head dims 64 .. 256, 1 .. 16 new tokens, rotary dims 16 .. D in both pairings, f32 or 16-bit tables (a quarter
             of them shorter than the largest position), 16-bit or e4m3 caches with general descales, strided inputs.  The whole pool is compared byte
             for byte with the image tests/kvappend_refs.py: append_rows gives.
    trace    a serving loop on a paged cache: prompts appended in one chunk, then 40 .. 70 steps of `lens += Nq` on the device and the fused
             flash_attention_decode(k=, v=, rotary_*=), sequences that finish and hand their pages, NOT cleared, to a new prompt, pages that fall out
             of a window and are reused.  Every step's O and LSE against float64 over the CPU's image of the pool; the pool itself bit for bit at drawn
             steps; optionally the same trace replayed from one captured graph, bit for bit against the eager one.
The rows per K / V head 17, 33 and 49 have no factorisation inside Nq 1 .. 8 x G {1, 2, 3, 4, 5, 8, 16}: the biased draw of the row count may use any
group size that gives them (G = 17, 11, 33, 7, 49).

The draw (draw_case, pure Python) is separate from the run (run_case) so that tests/test_fuzz_decode.py can check coverage, the checker's power against
float64 mutants and that the drawn features are not idle, all on the CPU.  No case feeds a length outside [0, capacity_keys] or a page id outside
[0, num_pages) to the GPU; the draw redraws what the library would refuse.

    python tools/fuzz_decode.py --mode decode --cases 1500 --seed 1 [--out FILE]
"""
import argparse
import json
import math
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
for _p in (os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import decode_abi as dc  # noqa: E402 - decode_c: the one copy of the C argument lists
import decode_window_refs as wr  # noqa: E402 - truth64, emulate, bars_of, check: the one copy of the decode contract
import kvappend_refs as kr  # noqa: E402 - append_rows: the one copy of the append contract
from rocwmma_fattn import _fa2_lib  # noqa: E402

MODES = ("decode", "append", "trace")
TILE = 32
F16, BF16, E4M3 = torch.float16, torch.bfloat16, torch.float8_e4m3fn
DT = {"f16": F16, "bf16": BF16}
NAN_BYTE = 0x7F
HKV = [1, 2, 3, 4, 8]
GROUPS = [1, 2, 3, 4, 5, 8, 16]
ROWS_BIAS = [16, 17, 32, 33, 48, 49, 64]
BATCHES = [1, 2, 3, 5, 9]
CAPACITIES = [1, 31, 32, 33, 64, 100, 257, 520, 1000, 1056]
PAGES = [64, 128, 192, 256, 320]
MAX_KEYS = 1100
SOFTCAPS = [0.0, 1.0, 8.0, 30.0, 50.0]
SCALE_MULS = [1.0, 0.5, 2.0, 3.0]
AMPS = [3.0, 4.0, 6.0, 8.0]
APPEND_DIMS = [64, 80, 96, 128, 256]
ROTARY_DIMS = [16, 32, 48, 64, "D"]


# ---------------------------------------------------------------------------------------------------------------- the plan's rule, mirrored
def plan_mirror(B, Hkv, Nq, G, capacity_keys, window_left, num_splits, cus):
    """include/fa2_gfx950.h, fa2_fwd_decode_plan / _window_plan -> (row_tiles, nsplit): row tiles from the rows per K / V head (three run as four), the
    split from B * Hkv * row_tiles, the CU count and the span a sequence can sweep.  Never a function of the lengths."""
    rt = -(-(Nq * G) // 16)
    rt = 4 if rt == 3 else rt
    span = -(-capacity_keys // TILE)
    if window_left >= 0:
        span = min(span, -(-(window_left + Nq) // TILE) + 1)
    if num_splits > 0:
        return rt, num_splits
    work = B * Hkv * rt
    if work >= cus:
        return rt, 1
    return rt, max(1, min(2 * cus // work, 16, span // 8))


def workspace_mirror(B, Hkv, Nq, G, D, nsplit):
    return 0 if nsplit == 1 else B * Hkv * nsplit * Nq * G * (D + 1) * 4


def device_cus():
    """the CU count the library's plan sees: the device's, 256 without one (csrc/host.cpp: device_cus)"""
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count if torch.cuda.is_available() else 256


# ---------------------------------------------------------------------------------------------------------------- the draw
def _draw_rows(rng):
    """(Nq, G) with Nq * G <= 64, biased towards the row counts at and one past a 16-row tile"""
    if rng.random() < 0.4:
        rows = rng.choice(ROWS_BIAS)
        nq = rng.choice([n for n in range(1, 9) if rows % n == 0])
        return nq, rows // nq
    while True:
        nq, g = rng.randint(1, 8), rng.choice(GROUPS)
        if nq * g <= 64:
            return nq, g


def _draw_cache(rng):
    """paged: (page, entries, block-table padding); contiguous: (0, capacity, 0)"""
    if rng.random() < 0.5:
        page = rng.choice(PAGES)
        return page, rng.randint(1, min(6, MAX_KEYS // page)), rng.choice([1, 3, 8])
    return 0, rng.choice(CAPACITIES), 0


def _draw_len(rng, nq, page, cap_keys):
    if rng.random() < 0.5:
        edges = [0, 1, nq - 1, nq, nq + 1, 31, 32, 33, cap_keys - 1, cap_keys]
        if page:
            for k in range(1, cap_keys // page + 1):
                edges += [k * page, k * page + 1]
        return rng.choice([e for e in edges if 0 <= e <= cap_keys])
    return rng.randint(0, cap_keys)


def _draw_window(rng, nq, lens, cap_keys):
    r = rng.random()
    if r < 0.3:
        return -1
    if r < 0.55:
        return rng.choice([0, 1, 31, 32, 33])
    if r < 0.8:                                     # lo = n - Nq - window_left on a tile edge of a drawn length, and one key either side of it
        long = [n for n in lens if n - nq > TILE]
        if long:
            n = rng.choice(long)
            return n - nq - TILE * rng.randint(1, (n - nq - 1) // TILE) + rng.choice([-1, 0, 1])
    return rng.choice([w for w in (cap_keys - 2, cap_keys - 1, 5000) if w >= 0])


def _draw_decode(i, rng):
    nq, g = _draw_rows(rng)
    page, capacity, bt_pad = _draw_cache(rng)
    cap_keys = page * capacity if page else capacity
    B = rng.choice(BATCHES)
    lens = [_draw_len(rng, nq, page, cap_keys) for _ in range(B)]
    share = None
    if page and B >= 2 and rng.random() < 1 / 3:     # sequence `b` names the first `n` physical pages of sequence `a` (prefix sharing)
        a, b = rng.sample(range(B), 2)
        n = rng.randint(1, capacity)
        lens[a] = max(lens[a], n * page)
        lens[b] = max(lens[b], (n - 1) * page + rng.randint(1, page))
        share = (a, b, n)
    if rng.random() < 0.5:                           # one sequence fills the cache, so that a drawn window, cap or slope has something to act on
        lens[rng.randrange(B)] = cap_keys
    fp8 = rng.random() < 0.4
    slopes = rng.choice([None, None, "H", "BH"])
    return dict(mode="decode", i=i, seed=rng.getrandbits(48), dtype=rng.choice(["f16", "bf16"]), D=rng.choice([64, 128]), Hkv=rng.choice(HKV), G=g, Nq=nq,
                B=B, page=page, capacity=capacity, bt_pad=bt_pad, lens=lens, share=share, window_left=_draw_window(rng, nq, lens, cap_keys),
                softcap=rng.choice([0.0, 0.0, 0.0] + SOFTCAPS[1:]), slopes=slopes, slopes_pad=rng.choice([0, 3]) if slopes == "BH" else 0,
                scale_mul=rng.choice([1.0] + SCALE_MULS), fp8=fp8, descale=rng.choice(["none", "k", "v", "both"]) if fp8 else "none",
                descale_pad=rng.choice([0, 2]), num_splits=rng.choice([0, 0, 1] + [rng.randint(2, 16)] * 3),
                q_layout=rng.choice(["plain", "headslice", "rowpad"]), cache_layout=rng.choice(["plain", "nmaxpad", "headslice"]),
                amp=rng.choice(AMPS) if rng.random() < 1 / 3 else 1.0, operator=i % 4 == 1, twice=i % 4 == 3)


def _draw_append(i, rng):
    nnew = rng.randint(1, 16)
    page, capacity, bt_pad = _draw_cache(rng)
    cap_keys = page * capacity if page else capacity
    B, D = rng.choice(BATCHES), rng.choice(APPEND_DIMS)
    lens = []
    for _ in range(B):
        if rng.random() < 0.6:
            edges = [0, 1, nnew - 1, nnew, nnew + 1, cap_keys - 1, cap_keys]
            if page:
                for k in range(1, cap_keys // page + 1):
                    edges += [k * page, k * page + 1, k * page + nnew // 2]
            lens.append(rng.choice([e for e in edges if 0 <= e <= cap_keys]))
        else:
            lens.append(rng.randint(0, cap_keys))
    rot = 0
    if rng.random() < 0.85:
        rot = rng.choice(ROTARY_DIMS)
        rot = D if rot == "D" else min(rot, D)
    fp8 = rng.random() < 0.4
    return dict(mode="append", i=i, seed=rng.getrandbits(48), dtype=rng.choice(["f16", "bf16"]), D=D, Hkv=rng.choice(HKV), G=rng.choice(GROUPS), Nnew=nnew,
                B=B, page=page, capacity=capacity, bt_pad=bt_pad, lens=lens, rot=rot, inter=rng.random() < 0.5, table=rng.choice(["f32", "io"]),
                short_table=rng.random() < 0.25, with_q=rot > 0 and rng.random() < 0.7, fp8=fp8,
                descale=rng.choice(["none", "k", "v", "both"]) if fp8 else "none", descale_pad=rng.choice([0, 2]),
                new_layout=rng.choice(["plain", "headslice"]), cache_layout=rng.choice(["plain", "nmaxpad", "headslice"]))


def trace_lengths(desc):
    """[(lengths before the step's increment, after it)] of a trace's steps: a finished slot restarts at its new prompt's length before the increment"""
    lens, out = list(desc["prompts"]), []
    for s in range(desc["steps"]):
        for (step, slot, new) in desc["events"]:
            if step == s:
                lens[slot] = new
        before = list(lens)
        lens = [n + desc["Nq"] for n in lens]
        out.append((before, list(lens)))
    return out


def trace_crossings(desc):
    """per slot: crossed a tile edge, crossed a page edge; and whether some slot's window edge lo crossed a page edge"""
    B, nq, page, wl = desc["B"], desc["Nq"], desc["page"], desc["window_left"]
    tile, pg, lo_pg = [False] * B, [False] * B, False
    for before, after in trace_lengths(desc):
        for b in range(B):
            tile[b] |= before[b] // TILE != after[b] // TILE
            pg[b] |= before[b] // page != after[b] // page
            lo_pg |= wl >= 0 and wr.window_lo(before[b], nq, wl) // page != wr.window_lo(after[b], nq, wl) // page
    return tile, pg, lo_pg


def _draw_trace(i, rng):
    while True:
        B, nq, page, steps = rng.randint(3, 5), rng.choice([1, 2, 3]), rng.choice([64, 128]), rng.randint(40, 70)
        wl = rng.choice([-1, 40, 70])
        prompts = [rng.choice([1, 2]) * page - rng.randint(1, min(30, steps * nq - 1)) for _ in range(B)]
        if wl >= 0:                                  # slot 0's window edge reaches the first page edge during the trace
            prompts[0] = page + wl + nq - rng.randint(1, 20)
        events = sorted((rng.randint(8, steps - 8), slot, rng.randint(1, page + 20)) for slot in rng.sample(range(1, B), rng.randint(1, 2)))
        slopes = rng.choice([None, "H", "BH"])
        D = rng.choice([64, 128])
        d = dict(mode="trace", i=i, seed=rng.getrandbits(48), dtype=rng.choice(["f16", "bf16"]), D=D, Hkv=rng.choice([1, 2, 4]), G=rng.choice([1, 2, 4, 8]),
                 Nq=nq, B=B, page=page, steps=steps, window_left=wl, softcap=rng.choice([0.0, 0.0, 30.0]), slopes=slopes, fp8=rng.random() < 0.5,
                 rot=rng.choice([32, D]), inter=rng.random() < 0.5, num_splits=rng.choice([0, 1, 3]), prompts=prompts, events=events,
                 check_steps=sorted(rng.sample(range(steps), 3)), graph=False)
        d["capacity"] = -(-max(max(after) for _, after in trace_lengths(d)) // page) + 1
        tile, pg, lo_pg = trace_crossings(d)
        if all(tile) and all(pg) and (wl < 0 or lo_pg):
            return d


def draw_case(i, rng, force=None):
    """Case i of a sweep as a dict that describes the call completely; force: "decode" | "append" | "trace" (None: decode).  Pure Python."""
    return {"append": _draw_append, "trace": _draw_trace}.get(force, _draw_decode)(i, rng)


def draw_sweep(seed, counts):
    """The cases of a sweep: counts = [(force, n), ...] drawn in that order from one generator."""
    rng = random.Random(seed)
    out = []
    for force, n in counts:
        for _ in range(n):
            out.append(draw_case(len(out), rng, force))
    return out


# the slices of tests/test_fuzz_decode_gpu.py; tests/test_fuzz_decode.py proves on the CPU what these seeds reach
DECODE_SEED, DECODE_COUNTS = 4, [("decode", 120)]
APPEND_SEED, APPEND_COUNTS = 1, [("append", 60)]
TRACE_SEED, TRACE_COUNTS = 5, [("trace", 6)]


def cap_keys_of(d):
    return d["page"] * d["capacity"] if d["page"] else d["capacity"]


def banded(d):
    """the call runs the banded kernels: a window that does not reach across the cache for every row, a cap or slopes (include/fa2_gfx950.h)"""
    return 0 <= d["window_left"] < cap_keys_of(d) - 1 or d["softcap"] > 0 or d["slopes"] is not None


def has_empty_part(d):
    """under a forced split, a sequence with keys whose last parts sweep no tile (fa2_decode_window_part_range)"""
    if d["num_splits"] < 2:
        return False
    for n in d["lens"]:
        t0, t1 = wr.window_lo(n, d["Nq"], d["window_left"]) // TILE, -(-n // TILE)
        if n and (d["num_splits"] - 1) * -(-(t1 - t0) // d["num_splits"]) >= t1 - t0:
            return True
    return False


def coverage(descs):
    """What a list of drawn cases reaches, as counts by name (the slices of tests/test_fuzz_decode_gpu.py must have every one of them >= 1)."""
    c = {}

    def hit(name, cond=True):
        c[name] = c.get(name, 0) + int(bool(cond))
    for d in descs:
        if d["mode"] == "decode":
            rows, ck, wl, nq = d["Nq"] * d["G"], cap_keys_of(d), d["window_left"], d["Nq"]
            rt = plan_mirror(d["B"], d["Hkv"], nq, d["G"], ck, wl, d["num_splits"], 256)[0]
            los = [wr.window_lo(n, nq, wl) for n in d["lens"]]
            pure = d["softcap"] == 0 and d["slopes"] is None
            for t in (1, 2, 4):
                hit("row tiles %d" % t, rt == t)
            for r in (16, 17, 32, 33, 48, 49, 64):
                hit("rows per K / V head exactly %d" % r, rows == r)
            for fmt in (False, True):
                for bd in (False, True):
                    hit("%s cache, %s" % ("e4m3" if fmt else "16-bit", "banded" if bd else "windowless"), d["fp8"] == fmt and banded(d) == bd)
            hit("paged with shared pages", d["share"] is not None)
            hit("contiguous capacity below one tile", not d["page"] and ck < TILE)
            hit("capacity no multiple of the tile, a length at it", ck % TILE and ck in d["lens"])
            hit("a length equal to the capacity", ck in d["lens"])
            hit("a length one below the capacity", ck - 1 in d["lens"])
            hit("an all-empty part under a forced split", has_empty_part(d))
            hit("the plan's own split", d["num_splits"] == 0)
            hit("lo on a tile edge", wl >= 0 and any(lo > 0 and lo % TILE == 0 for lo in los))
            hit("lo one key below a tile edge", wl >= 0 and any(lo % TILE == TILE - 1 for lo in los))
            hit("lo one key above a tile edge", wl >= 0 and any(lo > 1 and lo % TILE == 1 for lo in los))
            hit("window_left = capacity_keys - 1: the plain route", pure and wl == ck - 1)
            hit("window_left = capacity_keys - 2: the banded route", pure and wl == ck - 2 and wl >= 0)
            hit("either route on an odd capacity", pure and ck % 2 and wl >= 0 and wl in (ck - 1, ck - 2))
            for p in PAGES:
                hit("page size %d" % p, d["page"] == p)
            for b in (1, 2, 3):
                hit("batch %d" % b, d["B"] == b)
            hit("slopes [B, H] with a padded stride", d["slopes"] == "BH" and d["slopes_pad"] > 0)
            hit("descales with a padded stride", d["descale"] != "none" and d["descale_pad"] > 0)
            for kind in ("k", "v", "both"):
                hit("e4m3 descale: %s" % kind, d["descale"] == kind)
            hit("scale other than D^-0.5", d["scale_mul"] != 1.0)
            hit("amplified logits under a cap", d["amp"] > 1 and d["softcap"] > 0)
            hit("Nq 5 .. 8", nq >= 5)
            hit("a zero-length sequence", 0 in d["lens"])
        elif d["mode"] == "append":
            ck = cap_keys_of(d)
            for r in ROTARY_DIMS:
                for inter in (True, False):
                    hit("rotary dim %s, %s" % (r, "GPT-J" if inter else "GPT-NeoX"), d["rot"] == (d["D"] if r == "D" else r) and d["inter"] == inter)
            hit("no rotary", d["rot"] == 0)
            hit("a short rotary table", d["rot"] and d["short_table"] and max(d["lens"]) > 2)
            hit("rotary at head dim 80 or 256", d["rot"] and d["D"] in (80, 256))
            hit("len < Nnew", any(n < d["Nnew"] for n in d["lens"]))
            hit("len < Nnew, paged", d["page"] and any(0 < n < d["Nnew"] for n in d["lens"]))
            hit("len = capacity", ck in d["lens"])
            hit("Nnew 5 .. 16", d["Nnew"] >= 5)
            hit("e4m3 with rotary", d["fp8"] and d["rot"])
            hit("e4m3 with both descales", d["descale"] == "both")
            hit("q rotated", d["with_q"])
            hit("16-bit tables", d["rot"] and d["table"] == "io")
            hit("strided new tokens", d["new_layout"] != "plain")
        else:
            hit("trace with a recycle", bool(d["events"]))
            hit("trace with a window crossing a page", d["window_left"] >= 0 and trace_crossings(d)[2])
            hit("trace on an e4m3 cache", d["fp8"])
            hit("trace on a 16-bit cache", not d["fp8"])
            hit("trace with Nq > 1", d["Nq"] > 1)
    return c


def shrink(desc, still_fails):
    """Greedy reduction of a failing decode / append draw: drop sequences, then plain layouts, one at a time, keeping a change only while
    still_fails(candidate) holds.  -> the smallest description found."""
    d = dict(desc)
    b = d["B"] - 1
    while b >= 0 and d["B"] > 1:
        if not (d.get("share") and b in d["share"][:2]):
            c = dict(d, B=d["B"] - 1, lens=d["lens"][:b] + d["lens"][b + 1:])
            if c.get("share"):
                c["share"] = tuple(x - (x > b) for x in c["share"][:2]) + (c["share"][2],)
            if still_fails(c):
                d = c
        b -= 1
    for key, plain in (("q_layout", "plain"), ("cache_layout", "plain"), ("new_layout", "plain"), ("amp", 1.0), ("scale_mul", 1.0), ("slopes_pad", 0),
                       ("descale_pad", 0), ("bt_pad", 1 if d["page"] else 0)):
        if key in d and d[key] != plain:
            c = dict(d, **{key: plain})
            if still_fails(c):
                d = c
    return d


# ---------------------------------------------------------------------------------------------------------------- tensors of a decode case
def _randn(shape, g):
    return torch.randn(shape, generator=g)


def general_descale(x, g):
    """[B, Hkv] from x [B, n, Hkv, D]: the largest magnitude over 448 times a factor in [1, 1.37) — no power of two, nothing clamps"""
    return (x.abs().amax(dim=(1, 3)).clamp_min(1e-3) / 448.0) * (1.0 + 0.37 * torch.rand(x.shape[0], x.shape[2], generator=g))


def slopes_of(desc):
    """None, [H] or [B, H] (tests/decode_window_refs.py: slopes_of)"""
    return wr.slopes_of(desc["slopes"], desc["B"], desc["Hkv"] * desc["G"])


def build_decode(desc):
    """CPU tensors of a decode case: q, the clean logical caches kc / vc [B, capacity_keys, Hkv, D] in the cache format (a sharer's leading pages
    copied from the owner's), the descales, the slopes, the scale."""
    g = torch.Generator().manual_seed(desc["seed"])
    dt, B, nq, Hkv, G, D = DT[desc["dtype"]], desc["B"], desc["Nq"], desc["Hkv"], desc["G"], desc["D"]
    ck, a = cap_keys_of(desc), desc["amp"] ** 0.5
    q = (2 * a * _randn((B, nq, Hkv * G, D), g)).to(dt)
    xk, xv = 2 * a * _randn((B, ck, Hkv, D), g), 2 * _randn((B, ck, Hkv, D), g)
    kd = vd = None
    if desc["fp8"]:
        kd = general_descale(xk, g) if desc["descale"] in ("k", "both") else None
        vd = general_descale(xv, g) if desc["descale"] in ("v", "both") else None
        kc, vc = kr.quantise(xk, kd), kr.quantise(xv, vd)
    else:
        kc, vc = xk.to(dt), xv.to(dt)
    if desc["share"]:
        a_, b_, n = desc["share"]
        for t in (kc, vc):
            t.view(torch.uint8 if desc["fp8"] else torch.int16)[b_, :n * desc["page"]] = t.view(torch.uint8 if desc["fp8"] else torch.int16)[a_, :n * desc["page"]]
    return dict(q=q, kc=kc, vc=vc, kd=kd, vd=vd, slopes=slopes_of(desc), scale=D ** -0.5 * desc["scale_mul"])


def seq_parts(desc, inp, b, n=None):
    """The [H, ., D] operands of sequence b's reference: q, the upcast cache rows (raw codes for e4m3), their float64 meaning, the descales per query
    head [H, 1, 1] (None: 1.0) and the slopes [H] (None: off)."""
    G = desc["G"]
    n = desc["lens"][b] if n is None else n
    qs = inp["q"][b].transpose(0, 1).float()
    kraw, vraw = (t[b, :n].float().transpose(0, 1).repeat_interleave(G, dim=0) for t in (inp["kc"], inp["vc"]))
    kdh, vdh = (None if d is None else d[b].repeat_interleave(G)[:, None, None] for d in (inp["kd"], inp["vd"]))
    sl = inp["slopes"]
    return dict(q=qs, kraw=kraw, vraw=vraw, k=kraw.double() if kdh is None else kraw.double() * kdh.double(),
                v=vraw.double() if vdh is None else vraw.double() * vdh.double(), kd=kdh, vd=vdh, slopes=None if sl is None else (sl if sl.dim() == 1 else sl[b]))


def refs_of_parts(p, scale, wl, cap, dt):
    """dict(true, plain, emu, bars) of one sequence: tests/decode_window_refs.py's float64 with and without the keywords, its emulation (an e4m3 cache:
    k_descale folded into the score scale, v_descale on the normalised f32 row) and its bars"""
    true = wr.truth64(p["q"], p["k"], p["v"], scale, wl, cap, p["slopes"])
    plain = wr.truth64(p["q"], p["k"], p["v"], scale, -1, 0.0, None)
    emu = wr.emulate(p["q"], p["kraw"], p["vraw"], scale if p["kd"] is None else scale * p["kd"], wl, cap, p["slopes"], dt, v_descale=p["vd"])
    return dict(true=true, plain=plain, emu=emu, bars=wr.bars_of(true, emu, wr.code_of(dt)))


def decode_refs(desc, inp):
    dt = DT[desc["dtype"]]
    return [None if n == 0 else refs_of_parts(seq_parts(desc, inp, b), inp["scale"], desc["window_left"], desc["softcap"], dt) for b, n in enumerate(desc["lens"])]


def emulated_outputs(desc, refs):
    """(o [B, Nq, H, D], log2 lse [B, H, Nq]) of the emulation, float64: what tests/test_fuzz_decode.py feeds the checker in a kernel's place"""
    B, nq, H, D = desc["B"], desc["Nq"], desc["Hkv"] * desc["G"], desc["D"]
    o, lse = torch.zeros((B, nq, H, D), dtype=torch.float64), torch.full((B, H, nq), float("-inf"), dtype=torch.float64)
    for b, r in enumerate(refs):
        if r is not None:
            o[b], lse[b] = r["emu"][0].transpose(0, 1), r["emu"][1]
    return o, lse


def _raw(t):
    """the bit patterns of a cache tensor (NaN fills and copies go through these)"""
    return t.view(torch.uint8) if t.dtype == E4M3 else t.view(torch.int16)


def _nan_like(t):
    return torch.full(t.shape, NAN_BYTE, dtype=torch.uint8).view(E4M3) if t.dtype == E4M3 else torch.full(t.shape, float("nan"), dtype=t.dtype)


def physical_caches(desc, inp):
    """The caches as the device gets them: NaN (0x7f) wherever no row may look — at or beyond a length, below a sequence's lo, in spare pages and in
    pages every user has freed.  Paged: shuffled physical order, unused and freed entries name an all-NaN page, a page two sequences name keeps what
    either of them sees.  -> k, v [B | pages, slots, Hkv, D], block table [B, capacity + bt_pad] or None"""
    B, nq, wl, page, cap = desc["B"], desc["Nq"], desc["window_left"], desc["page"], desc["capacity"]
    vis = [(wr.window_lo(n, nq, wl), n) for n in desc["lens"]]
    if not page:
        out = []
        for t in (inp["kc"], inp["vc"]):
            p = t.clone()
            for b, (lo, n) in enumerate(vis):
                _raw(p)[b, n:] = _raw(_nan_like(p[b, n:]))
                _raw(p)[b, :lo] = _raw(_nan_like(p[b, :lo]))
            out.append(p)
        return out[0], out[1], None
    owner = lambda b, j: (desc["share"][0] if desc["share"] and b == desc["share"][1] and j < desc["share"][2] else b, j)    # noqa: E731
    needs = {}                                        # (owner, logical page) -> [(b, lo, n)] of the sequences that read it
    for b, (lo, n) in enumerate(vis):
        for j in range(-(-n // page)):
            if (j + 1) * page > lo:
                needs.setdefault(owner(b, j), []).append((b, lo, n))
    rng = random.Random(desc["seed"])
    total = len(needs) + 3
    order = list(range(total))
    rng.shuffle(order)
    nan_page = order[-1]
    bt = torch.full((B, cap + desc["bt_pad"]), nan_page, dtype=torch.int32)
    pk, pv = (_nan_like(t.new_empty((total, page) + tuple(t.shape[2:]))) for t in (inp["kc"], inp["vc"]))
    for pid, ((a, j), users) in zip(order, sorted(needs.items())):
        seen = torch.zeros(page, dtype=torch.bool)
        for (b, lo, n) in users:
            bt[b, j] = pid
            s = torch.arange(j * page, (j + 1) * page)
            seen |= (s >= lo) & (s < n)
        for src, dst in ((inp["kc"], pk), (inp["vc"], pv)):
            _raw(dst)[pid][seen] = _raw(src)[a, j * page:(j + 1) * page][seen]
    return pk, pv, bt


def _place(t, layout, dev, fill=None):
    """t on the device as a view of a wider tensor: a padded slot stride (nmaxpad), a head slice (headslice), a padded row pitch (rowpad); the padding
    holds NaN (0x7f), or `fill` where given -> (view, wide tensor)"""
    raw = _raw(t) if t.dtype in (E4M3, F16, BF16) else t
    X, n, h, D = raw.shape
    shape = {"plain": (X, n, h, D), "nmaxpad": (X, n + 40, h, D), "headslice": (X, n, h + 1, D), "rowpad": (X, n, h, D + 8)}[layout]
    if fill is None:
        fill = NAN_BYTE if t.dtype == E4M3 else 0x7E00 if t.dtype == F16 else 0x7FC0
    wide = torch.full(shape, fill, dtype=raw.dtype)
    wide[:, :n, :h, :D] = raw
    wide = wide.to(dev).view(t.dtype)
    return wide[:, :n, :h, :D], wide


def _padded2(t, pad, dev):
    """a [B, n] tensor as a slice of [B, n + pad] on the device"""
    wide = torch.full((t.shape[0], t.shape[1] + pad), float("nan") if t.is_floating_point() else 0, dtype=t.dtype)
    wide[:, :t.shape[1]] = t
    return wide.to(dev)[:, :t.shape[1]]


def figures(o, lse2, refs):
    """(worst O error over its bar, worst LSE error) of outputs [B, Nq, H, D] / [B, H, Nq] against the float64 of refs; non-finite differences count as inf"""
    ratio = lerr = 0.0
    go, gl = o.detach().double().cpu(), lse2.detach().double().cpu()
    for b, r in enumerate(refs):
        if r is None:
            continue
        (to, tl), (obar, _) = r["true"], r["bars"]
        e = (go[b].transpose(0, 1) - to).abs().max().item()
        ratio = max(ratio, e / obar if math.isfinite(e) else float("inf"))
        live = ~torch.isinf(tl)
        if live.any():
            e = (gl[b][live] - tl[live]).abs().max().item()
            lerr = max(lerr, e if math.isfinite(e) else float("inf"))
    return ratio, lerr


def checked(o, lse2, refs, tag):
    """tests/decode_window_refs.py: check, as a list of failures"""
    try:
        wr.check(o, lse2, refs, tag)
    except AssertionError as e:
        return ["%s" % (e.args[0],) if e.args else "check failed"]
    return []


def _run_decode(desc):
    from rocwmma_fattn import FlashAttn
    dev = torch.device("cuda", torch.cuda.current_device())
    dt, B, nq, Hkv, G, D, wl = DT[desc["dtype"]], desc["B"], desc["Nq"], desc["Hkv"], desc["G"], desc["D"], desc["window_left"]
    ck, fails = cap_keys_of(desc), []
    assert all(0 <= n <= ck for n in desc["lens"]), "a drawn length outside the cache"
    inp = build_decode(desc)
    refs = decode_refs(desc, inp)
    pk, pv, bt = physical_caches(desc, inp)
    assert bt is None or (0 <= int(bt.min()) and int(bt.max()) < pk.shape[0]), "a drawn page id outside the pool"
    q = _place(inp["q"], desc["q_layout"], dev)[0]
    k, v = (_place(t, desc["cache_layout"], dev)[0] for t in (pk, pv))
    lens = torch.tensor(desc["lens"], dtype=torch.int32, device=dev)
    btd = None if bt is None else bt.to(dev)[:, :desc["capacity"]]
    kd, vd = (None if t is None else _padded2(t, desc["descale_pad"], dev) for t in (inp["kd"], inp["vd"]))
    sl = inp["slopes"]
    if sl is not None:
        sl = sl.to(dev) if sl.dim() == 1 else _padded2(sl, desc["slopes_pad"], dev)
    # the plan and the workspace against their mirrors
    lib = _fa2_lib.load()
    plan = _fa2_lib.decode_window_plan(dc.code(dt), B, Hkv * G, Hkv, nq, D, desc["capacity"], desc["page"], desc["num_splits"], wl)
    want = plan_mirror(B, Hkv, nq, G, ck, wl, desc["num_splits"], device_cus())
    if (plan.row_tiles, plan.nsplit) != want or plan.key_tile != TILE:
        fails.append("plan (%d, %d) tile %d, mirror %s" % (plan.row_tiles, plan.nsplit, plan.key_tile, want))
    need = lib.fa2_fwd_decode_window_workspace_bytes(dc.code(dt), B, Hkv * G, Hkv, nq, D, desc["capacity"], desc["page"], desc["num_splits"], wl)
    if need != workspace_mirror(B, Hkv, nq, G, D, plan.nsplit):
        fails.append("workspace %d bytes, the header's formula %d" % (need, workspace_mirror(B, Hkv, nq, G, D, plan.nsplit)))
    def window_c():
        """fa2_fwd_decode_window as tests/test_decode_window_gpu.py calls it: NaN-filled outputs and workspace -> (rc, o, lse)"""
        return dc.decode_c("window", q, k, v, lens, desc["num_splits"], wl, desc["softcap"], sl, block_table=btd, kd=kd, vd=vd, scale=inp["scale"], check=False)

    rc, o, lse = window_c()
    if rc != 0:
        return dict(desc, fails=fails + ["fa2_fwd_decode_window: %s" % _fa2_lib.error_string(rc)], o_ratio=float("inf"), lse_err=float("inf"))
    fails += checked(o, lse, refs, "case %d" % desc["i"])
    ratio, lerr = figures(o, lse, refs)
    if desc["twice"]:
        rc2, o2, lse2 = window_c()
        if rc2 != 0 or not dc.same_bits((o, lse), (o2, lse2)):
            fails.append("a second run differs")
    if desc["operator"]:
        po, pl = FlashAttn.flash_attention_decode(q, k, v, lens, block_table=btd, scale=inp["scale"], return_lse=True, num_splits=desc["num_splits"],
                                                  k_descale=kd, v_descale=vd, window=None if wl < 0 else (wl, 0), softcap=desc["softcap"], alibi_slopes=sl)
        torch.cuda.synchronize()
        if not dc.same_bits((o, lse * FlashAttn._LN2), (po, pl)):
            fails.append("flash_attention_decode differs from the C call")
    return dict(desc, fails=fails, o_ratio=ratio, lse_err=lerr, nsplit=plan.nsplit, row_tiles=plan.row_tiles)


# ---------------------------------------------------------------------------------------------------------------- append
def pattern(nbytes, salt=0):
    """a per-byte poison pattern without a short period (tests/test_kvappend_gpu.py's)"""
    i = torch.arange(nbytes, dtype=torch.int64)
    return ((i * 131 + (i >> 8) * 7 + (i >> 16) * 3 + 89 + salt) % 251).to(torch.uint8)


def rotary_tables(rot, dt, rows):
    """cos / sin [rows, rot / 2] from base 10 000 in float64, cast to dt (tests/test_kvappend_gpu.py's)"""
    inv = 10000.0 ** (-torch.arange(0, rot, 2, dtype=torch.float64) / rot)
    ang = torch.arange(rows, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().to(dt), ang.sin().to(dt)


def build_append(desc):
    """CPU tensors of an append case: the new tokens, the tables, the descales, the block table (shuffled pages, unused entries name a spare page), the
    pool's shape"""
    g = torch.Generator().manual_seed(desc["seed"])
    dt, B, nnew, Hkv, D = DT[desc["dtype"]], desc["B"], desc["Nnew"], desc["Hkv"], desc["D"]
    q, k, v = (_randn((B, nnew, h, D), g).to(dt) for h in (Hkv * desc["G"], Hkv, Hkv))
    kd = vd = None
    if desc["fp8"]:
        kd = 0.02 + 0.03 * torch.rand((B, Hkv), generator=g) if desc["descale"] in ("k", "both") else None
        vd = 0.02 + 0.03 * torch.rand((B, Hkv), generator=g) if desc["descale"] in ("v", "both") else None
    cos = sin = None
    if desc["rot"]:
        rows = max(1, (max(desc["lens"]) - 1) // 2) if desc["short_table"] else cap_keys_of(desc)
        cos, sin = rotary_tables(desc["rot"], torch.float32 if desc["table"] == "f32" else dt, rows)
    bt, shape = None, (B, desc["capacity"], Hkv, D)
    if desc["page"]:
        used = [-(-n // desc["page"]) for n in desc["lens"]]
        total = sum(used) + 3
        order = list(range(total))
        random.Random(desc["seed"]).shuffle(order)
        bt = torch.full((B, desc["capacity"] + desc["bt_pad"]), order[-1], dtype=torch.int32)
        nxt = 0
        for b, u in enumerate(used):
            for j in range(u):
                bt[b, j] = order[nxt]
                nxt += 1
        shape = (total, desc["page"], Hkv, D)
    return dict(q=q if desc["with_q"] else None, k=k, v=v, kd=kd, vd=vd, cos=cos, sin=sin, bt=bt, shape=shape)


def append_expected(desc, inp, pools):
    """pools: the two pattern-filled caches (views of their wide tensors, CPU) — written in place at the targets with tests/kvappend_refs.py: append_rows.
    -> the rotated q (or None)"""
    rk, rv, q_rot = kr.append_rows(inp["k"], inp["v"], desc["lens"], q=inp["q"], cos=inp["cos"], sin=inp["sin"], inter=desc["inter"], fp8=desc["fp8"],
                                   kd=inp["kd"], vd=inp["vd"])
    page = desc["page"]
    for (b, i, p) in kr.targets(desc["lens"], desc["Nnew"], cap_keys_of(desc)):
        for pool, rows in zip(pools, (rk, rv)):
            if page:
                _raw(pool)[int(inp["bt"][b, p // page]), p % page] = _raw(rows)[b, i]
            else:
                _raw(pool)[b, p] = _raw(rows)[b, i]
    return q_rot, rk


def _run_append(desc):
    from rocwmma_fattn import FlashAttn
    dev = torch.device("cuda", torch.cuda.current_device())
    dt, fails = DT[desc["dtype"]], []
    cdt = E4M3 if desc["fp8"] else dt
    inp = build_append(desc)
    assert all(0 <= n <= cap_keys_of(desc) for n in desc["lens"]), "a drawn length outside the cache"
    assert inp["bt"] is None or (0 <= int(inp["bt"].min()) and int(inp["bt"].max()) < inp["shape"][0]), "a drawn page id outside the pool"
    X, n, h, D = inp["shape"]
    wshape = {"plain": (X, n, h, D), "nmaxpad": (X, n + 40, h, D), "headslice": (X, n, h + 1, D)}[desc["cache_layout"]]
    nbytes = wshape[0] * wshape[1] * wshape[2] * wshape[3] * (1 if desc["fp8"] else 2)
    wide = [pattern(nbytes, salt).view(cdt).reshape(wshape) for salt in (0, 5)]
    want = [w.clone() for w in wide]
    q_rot, rk = append_expected(desc, inp, [w[:, :n, :h, :D] for w in want])
    dwide = [w.to(dev) for w in wide]
    kc, vc = (w[:, :n, :h, :D] for w in dwide)
    kn, vn = (_place(t, desc["new_layout"], dev, fill=0)[0] for t in (inp["k"], inp["v"]))
    lens = torch.tensor(desc["lens"], dtype=torch.int32, device=dev)
    bt = None if inp["bt"] is None else inp["bt"].to(dev)[:, :desc["capacity"]]
    kd, vd = (None if t is None else _padded2(t, desc["descale_pad"], dev) for t in (inp["kd"], inp["vd"]))
    got_q = FlashAttn.kvcache_append(kc, vc, kn, vn, lens, block_table=bt, rotary_cos=None if inp["cos"] is None else inp["cos"].to(dev),
                                     rotary_sin=None if inp["sin"] is None else inp["sin"].to(dev), rotary_interleaved=desc["inter"], k_descale=kd,
                                     v_descale=vd, q=None if inp["q"] is None else inp["q"].to(dev))
    torch.cuda.synchronize()
    wrong = 0
    for name, g, w in (("k", dwide[0], want[0]), ("v", dwide[1], want[1])):
        bad = int((_raw(g.cpu()) != _raw(w)).sum())
        wrong += bad
        if bad:
            fails.append("%s cache: %d elements differ from the expected image, first at %s" % (name, bad, (_raw(g.cpu()) != _raw(w)).nonzero()[0].tolist()))
    if (got_q is None) != (q_rot is None):
        fails.append("q_out present / absent")
    elif q_rot is not None:
        bad = int((_raw(got_q.cpu()) != _raw(q_rot)).sum())
        wrong += bad
        if bad:
            fails.append("q_out: %d elements differ from the host arithmetic" % bad)
    # the figure: written rotated 16-bit K rows against float64 as a share of tests/kvappend_refs.py's bar
    ratio = 0.0
    tg = kr.targets(desc["lens"], desc["Nnew"], cap_keys_of(desc))
    if desc["rot"] and not desc["fp8"] and tg:
        bi = (torch.tensor([t[0] for t in tg]), torch.tensor([t[1] for t in tg]))
        rows = torch.tensor([t[2] for t in tg]).clamp(0, inp["cos"].shape[0] - 1)
        ref, mag = kr.rotary_ref64(inp["k"][bi].double(), inp["cos"][rows].double()[:, None, :], inp["sin"][rows].double()[:, None, :], desc["rot"], desc["inter"])
        page = desc["page"]
        got = torch.stack([dwide[0][int(inp["bt"][b, p // page]), p % page, :h] if page else dwide[0][b, p, :h] for (b, i, p) in tg]).cpu()
        ratio = float(((got.double() - ref).abs() / kr.rotary_bar(ref, mag, dt)).max())
        if not ratio <= 1.0:
            fails.append("rotated K against float64: %.3g of the bar" % ratio)
    return dict(desc, fails=fails, o_ratio=ratio, lse_err=0.0, wrong=wrong, written=len(tg))


# ---------------------------------------------------------------------------------------------------------------- traces
class Trace:
    """A serving loop's state on the CPU, and on the device when `dev` is given.  The CPU keeps an image of the whole pool, written by the append
    reference alone; page hand-outs come from a last-in-first-out free list, so a finished sequence's pages (and pages that fell out of a window) go to
    the next taker with their old, finite contents.  Entry 0 of the pool is the all-NaN page unused block-table entries name."""

    def __init__(self, desc, dev=None):
        self.d, self.dev = desc, dev
        self.g = torch.Generator().manual_seed(desc["seed"])
        self.dt = DT[desc["dtype"]]
        B, Hkv, D, page, cap = desc["B"], desc["Hkv"], desc["D"], desc["page"], desc["capacity"]
        self.H = Hkv * desc["G"]
        total = B * cap + 3
        x = [2 * _randn((total, page, Hkv, D), self.g) for _ in range(2)]
        self.kd = self.vd = None
        if desc["fp8"]:
            self.kd, self.vd = (0.02 + 0.03 * torch.rand((B, Hkv), generator=self.g) for _ in range(2))
            self.pool = [kr.quantise(t, None) for t in x]
        else:
            self.pool = [t.to(self.dt) for t in x]
        for t in self.pool:
            _raw(t)[0] = _raw(_nan_like(t[0]))
        self.free = list(range(1, total))
        random.Random(desc["seed"]).shuffle(self.free)
        self.bt = torch.zeros((B, cap), dtype=torch.int32)
        self.owned = [dict() for _ in range(B)]
        self.lens = [0] * B
        self.cos, self.sin = rotary_tables(desc["rot"], torch.float32, cap * page)
        self.slopes = wr.slopes_of(desc["slopes"], B, self.H)
        self.scale = D ** -0.5
        self.recycled = set()                          # slots whose pages came from a finished sequence
        if dev is not None:
            self.dpool = [t.to(dev) for t in self.pool]
            self.dbt, self.dlens = self.bt.to(dev), torch.zeros(B, dtype=torch.int32, device=dev)
            self.dcos, self.dsin = self.cos.to(dev), self.sin.to(dev)
            self.dkd, self.dvd = (None if t is None else t.to(dev) for t in (self.kd, self.vd))
            self.dslopes = None if self.slopes is None else self.slopes.to(dev)
        for b, n in enumerate(desc["prompts"]):
            self.start(b, n)

    # -- pages: every hand-out is a block-table write on the CPU copy and, between launches, on the device tensor
    def _hand_out(self, b, whole=False):
        """pages for every logical page of slot b that holds a key at or above its lo (whole: for all of them — a prompt is appended in full)"""
        page = self.d["page"]
        lo = 0 if whole else wr.window_lo(self.lens[b], self.d["Nq"], self.d["window_left"])
        for j in range(-(-self.lens[b] // page)):
            if j not in self.owned[b] and (j + 1) * page > lo:
                pid = self.free.pop()
                self.owned[b][j] = pid
                self.bt[b, j] = pid
                if self.dev is not None:
                    self.dbt[b, j] = pid

    def _free_below_window(self, b):
        lo = wr.window_lo(self.lens[b], self.d["Nq"], self.d["window_left"])
        for j in [j for j in self.owned[b] if (j + 1) * self.d["page"] <= lo]:
            self.free.append(self.owned[b].pop(j))      # the entry keeps the stale id: the kernel never reads it

    def _write(self, b, rows_k, rows_v, nnew):
        """rows [1 | B, nnew, Hkv, D] of sequence b into the CPU image at the append's targets"""
        page = self.d["page"]
        for i in range(nnew):
            p = self.lens[b] - nnew + i
            if 0 <= p < self.d["capacity"] * page and p // page in self.owned[b]:
                for pool, rows in zip(self.pool, (rows_k, rows_v)):
                    _raw(pool)[self.owned[b][p // page], p % page] = _raw(rows)[i]

    def release(self, b):
        """slot b's sequence ends: its pages return to the free list as they are"""
        if self.owned[b]:
            self.recycled.add(b)
        for j in sorted(self.owned[b]):
            self.free.append(self.owned[b][j])
        self.owned[b] = {}

    def start(self, b, n):
        """slot b's sequence ends (release) and a prompt of n tokens takes the slot: one append chunk"""
        from rocwmma_fattn import FlashAttn
        self.release(b)
        self.lens[b] = n
        self._hand_out(b, whole=True)                  # (pages of a long prompt that lie below the window are freed at the next step)
        k, v = (_randn((1, n, self.d["Hkv"], self.d["D"]), self.g).to(self.dt) for _ in range(2))
        kd, vd = (None if t is None else t[b:b + 1] for t in (self.kd, self.vd))
        rk, rv, _ = kr.append_rows(k, v, [n], cos=self.cos, sin=self.sin, inter=self.d["inter"], fp8=self.d["fp8"], kd=kd, vd=vd)
        self._write(b, rk[0], rv[0], n)
        if self.dev is not None:
            self.dlens[b] = n
            FlashAttn.kvcache_append(self.dpool[0], self.dpool[1], k.to(self.dev), v.to(self.dev), self.dlens[b:b + 1], block_table=self.dbt[b:b + 1],
                                     rotary_cos=self.dcos, rotary_sin=self.dsin, rotary_interleaved=self.d["inter"],
                                     k_descale=None if self.dkd is None else self.dkd[b:b + 1], v_descale=None if self.dvd is None else self.dvd[b:b + 1])

    def begin_step(self, s):
        """the host's work in front of step s: finished slots restart, lengths grow by Nq (the CPU's copy: the device increments its own), pages are
        freed and handed out.  -> the new tokens q, k, v of the step"""
        for (step, slot, n) in self.d["events"]:
            if step == s:
                self.start(slot, n)
        nq = self.d["Nq"]
        for b in range(self.d["B"]):
            self.lens[b] += nq
            self._free_below_window(b)
            self._hand_out(b)
        return tuple((2 * _randn((self.d["B"], nq, h, self.d["D"]), self.g)).to(self.dt) for h in (self.H, self.d["Hkv"], self.d["Hkv"]))

    def apply_step(self, q, k, v):
        """the append reference on the CPU image -> the rotated q"""
        rk, rv, q_rot = kr.append_rows(k, v, self.lens, q=q, cos=self.cos, sin=self.sin, inter=self.d["inter"], fp8=self.d["fp8"], kd=self.kd, vd=self.vd)
        for b in range(self.d["B"]):
            self._write(b, rk[b], rv[b], self.d["Nq"])
        return q_rot

    def gather(self, b, n):
        """sequence b's keys [0, n) from the CPU image, zeros where it owns no page (below its window) -> k, v [n, Hkv, D] in the cache format.  n beyond
        the length reads what the page holds there: the previous owner's keys (the mutant of tests/test_fuzz_decode.py)."""
        page, out = self.d["page"], []
        for pool in self.pool:
            t = torch.zeros((n,) + tuple(pool.shape[2:]), dtype=torch.uint8 if self.d["fp8"] else torch.int16)
            for j in range(-(-n // page)):
                m = min(page, n - j * page)
                if j in self.owned[b]:
                    t[j * page:j * page + m] = _raw(pool)[self.owned[b][j], :m]
            out.append(t.view(pool.dtype))
        return out

    def parts(self, b, q_rot, n=None):
        """seq_parts of slot b at this step (n: as if the sequence had that many keys, positions unchanged — for mutants)"""
        G = self.d["G"]
        k, v = self.gather(b, self.lens[b] if n is None else n)
        kraw, vraw = (t.float().transpose(0, 1).repeat_interleave(G, dim=0) for t in (k, v))
        kdh, vdh = (None if d is None else d[b].repeat_interleave(G)[:, None, None] for d in (self.kd, self.vd))
        sl = self.slopes
        return dict(q=q_rot[b].transpose(0, 1).float(), kraw=kraw, vraw=vraw, k=kraw.double() if kdh is None else kraw.double() * kdh.double(),
                    v=vraw.double() if vdh is None else vraw.double() * vdh.double(), kd=kdh, vd=vdh,
                    slopes=None if sl is None else (sl if sl.dim() == 1 else sl[b]))

    def refs(self, q_rot):
        return [refs_of_parts(self.parts(b, q_rot), self.scale, self.d["window_left"], self.d["softcap"], self.dt) for b in range(self.d["B"])]

    def pool_mismatches(self):
        """elements of the pages some slot owns that differ between the device pool and the CPU image"""
        pids = sorted(p for o in self.owned for p in o.values())
        return sum(int((_raw(dp[pids].cpu()) != _raw(cp)[pids]).sum()) for dp, cp in zip(self.dpool, self.pool))


def _fused(tr, q, k, v, lens):
    from rocwmma_fattn import FlashAttn
    d = tr.d
    return FlashAttn.flash_attention_decode(q, tr.dpool[0], tr.dpool[1], lens, block_table=tr.dbt, return_lse=True, num_splits=d["num_splits"],
                                            k_descale=tr.dkd, v_descale=tr.dvd, k=k, v=v, rotary_cos=tr.dcos, rotary_sin=tr.dsin,
                                            rotary_interleaved=d["inter"], window=None if d["window_left"] < 0 else (d["window_left"], 0),
                                            softcap=d["softcap"], alibi_slopes=tr.dslopes)


def _run_trace(desc, graph=False, keep=None):
    """The eager trace (graph=False) or its replay from one captured step.  keep: a list that receives every step's (o, lse) on the CPU."""
    from rocwmma_fattn import FlashAttn
    dev = torch.device("cuda", torch.cuda.current_device())
    tr = Trace(desc, dev)
    B, nq, D = desc["B"], desc["Nq"], desc["D"]
    fails, ratio, lerr, wrong = [], 0.0, 0.0, 0
    if graph:                                        # one step — the in-place increment and the fused call — captured on a side stream, single-stream
        qi, ki, vi = (torch.zeros((B, nq, h, D), dtype=tr.dt, device=dev) for h in (tr.H, desc["Hkv"], desc["Hkv"]))
        scratch = (tr.dpool, tr.dlens)
        tr.dpool, tr.dlens = [t.clone() for t in tr.dpool], tr.dlens.clone()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                # warm-up outside the capture, on a pool and lengths of its own
            tr.dlens.add_(nq)
            _fused(tr, qi, ki, vi, tr.dlens)
        torch.cuda.current_stream().wait_stream(side)
        tr.dpool, tr.dlens = scratch
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(cg, stream=side):
                tr.dlens.add_(nq)
                go, gl = _fused(tr, qi, ki, vi, tr.dlens)
        torch.cuda.current_stream().wait_stream(side)
    for s in range(desc["steps"]):
        q, k, v = tr.begin_step(s)
        if graph:
            qi.copy_(q.to(dev))
            ki.copy_(k.to(dev))
            vi.copy_(v.to(dev))
            go.zero_()
            gl.zero_()
            cg.replay()
            o, lse = go, gl
        else:
            tr.dlens.add_(nq)
            o, lse = _fused(tr, q.to(dev), k.to(dev), v.to(dev), tr.dlens)
        torch.cuda.synchronize()
        refs = tr.refs(tr.apply_step(q, k, v))
        lse2 = lse / FlashAttn._LN2
        fails += checked(o, lse2, refs, "trace %d step %d" % (desc["i"], s))
        r, e = figures(o, lse2, refs)
        ratio, lerr = max(ratio, r), max(lerr, e)
        if keep is not None:
            keep.append((o.cpu().clone(), lse.cpu().clone()))
        if s in desc["check_steps"] or s == desc["steps"] - 1:
            bad = tr.pool_mismatches()
            wrong += bad
            if bad:
                fails.append("step %d: %d elements of the owned pages differ from the image" % (s, bad))
        if len(fails) > 8:
            break
    if tr.dlens.cpu().tolist() != tr.lens:
        fails.append("the device's lengths %s, the host's %s" % (tr.dlens.cpu().tolist(), tr.lens))
    return dict(desc, fails=fails, o_ratio=ratio, lse_err=lerr, wrong=wrong, steps_run=s + 1, recycled=len(tr.recycled))


def run_trace_with_graph(desc):
    """the eager trace, then the same trace replayed from a captured step: every step's O and LSE bit for bit"""
    eager, replay = [], []
    out = _run_trace(desc, keep=eager)
    g = _run_trace(desc, graph=True, keep=replay)
    fails = out["fails"] + ["graph: " + f for f in g["fails"]]
    if len(eager) != len(replay) or not all(dc.same_bits(a, b) for a, b in zip(eager, replay)):
        fails.append("the graph replay differs from the eager trace")
    return dict(out, fails=fails, graph=True, o_ratio=max(out["o_ratio"], g["o_ratio"]), lse_err=max(out["lse_err"], g["lse_err"]))


def run_case(desc, gen=None):
    """Build the tensors of a drawn case (from desc["seed"]; gen is unused and kept for the shape of tools/fuzz_features.py), run it on the current
    device, check: desc plus `fails`, `o_ratio` (the worst error over its bar) and `lse_err`."""
    if desc["mode"] == "append":
        return _run_append(desc)
    if desc["mode"] == "trace":
        return run_trace_with_graph(desc) if desc["graph"] else _run_trace(desc)
    return _run_decode(desc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--mode", default="decode", choices=MODES)
    ap.add_argument("--graph-every", type=int, default=10, help="every n-th trace is also replayed from a captured graph (0 = never)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bad, worst = [], dict(o_ratio=0.0, lse_err=0.0)
    for desc in draw_sweep(args.seed, [(args.mode, args.cases)]):
        if desc["mode"] == "trace" and args.graph_every > 0 and desc["i"] % args.graph_every == 0:
            desc = dict(desc, graph=True)
        try:
            d = run_case(desc)
        except Exception as e:                      # a refused shape or a launch error is a finding too
            d = dict(desc, fails=["exception: %r" % (e,)])
        for key in worst:
            worst[key] = max(worst[key], d.get(key, 0.0))
        if d["fails"]:
            bad.append(d)
            print("FAIL", json.dumps(d), flush=True)
    summary = dict(tool="fuzz_decode", mode=args.mode, cases=args.cases, seed=args.seed, failures=len(bad), worst_o_err_over_bar=worst["o_ratio"],
                   worst_lse_err=worst["lse_err"], device=torch.cuda.get_device_name(0), failing=bad)
    line = json.dumps(summary)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
