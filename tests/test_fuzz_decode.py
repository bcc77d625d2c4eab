"""CPU tests of tools/fuzz_decode.py, the randomised sweep of the decode and append calls and of serving traces: that the slices the `-m gpu` suite runs
(tests/test_fuzz_decode_gpu.py) reach what they are there for, that the sweep's checker flags wrong kernels — float64 mutants of the contract that lie at
least 5 bars from the truth, the margin of tests/test_decode_window.py — that the drawn windows, caps and slopes are not idle, and that the tool's own
references agree with each other, with the header's plan rule and with the library's host-side rotary arithmetic.  "The kernel's output" here is the
same-contract emulation; nothing touches a device."""
import ctypes
import importlib.util
import os

import pytest
import torch

import decode_window_refs as wr
import kvappend_refs as kr
from rocwmma_fattn import _fa2_lib

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
MARGIN = 5.0
TILE = 32


@pytest.fixture(scope="module")
def fd():
    spec = importlib.util.spec_from_file_location("_fuzz_decode", os.path.join(ROOT, "tools", "fuzz_decode.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def decode_slice(fd):
    """[(desc, inputs, refs)] of the GPU slice, computed once and never modified"""
    out = []
    for d in fd.draw_sweep(fd.DECODE_SEED, fd.DECODE_COUNTS):
        inp = fd.build_decode(d)
        out.append((d, inp, fd.decode_refs(d, inp)))
    return out


def test_draw_is_pure_and_reproducible(fd):
    for seed, counts in ((fd.DECODE_SEED, fd.DECODE_COUNTS), (fd.APPEND_SEED, fd.APPEND_COUNTS), (fd.TRACE_SEED, fd.TRACE_COUNTS)):
        a, b = fd.draw_sweep(seed, counts), fd.draw_sweep(seed, counts)
        assert a == b and len(a) == sum(n for _, n in counts)
        for d in a:
            ck = fd.cap_keys_of(d)
            assert d["mode"] == counts[0][0] and ck <= 1100 + 320 and (d["page"] % 64 == 0)
            if d["mode"] == "decode":
                assert all(0 <= n <= ck for n in d["lens"]) and len(d["lens"]) == d["B"] and 1 <= d["Nq"] <= 8 and d["Nq"] * d["G"] <= 64
                assert d["window_left"] >= -1 and 0 <= d["num_splits"] <= 16 and d["D"] in (64, 128)
                if d["share"]:
                    a_, b_, n = d["share"]
                    assert a_ != b_ and 1 <= n <= d["capacity"] and d["lens"][a_] >= n * d["page"] and d["lens"][b_] > (n - 1) * d["page"]
            elif d["mode"] == "append":
                assert all(0 <= n <= ck for n in d["lens"]) and 1 <= d["Nnew"] <= 16 and d["rot"] % 16 == 0 and d["rot"] <= d["D"]
                assert d["D"] % 16 == 0 and (d["rot"] or not d["with_q"])
            else:
                assert 3 <= d["B"] <= 5 and 40 <= d["steps"] <= 70 and d["page"] in (64, 128)
                assert max(max(after) for _, after in fd.trace_lengths(d)) <= ck
                tile, pg, _ = fd.trace_crossings(d)
                assert all(tile) and all(pg), "every slot crosses a tile edge and a page edge"


def test_slices_reach_what_they_are_there_for(fd):
    cov = {}
    for seed, counts in ((fd.DECODE_SEED, fd.DECODE_COUNTS), (fd.APPEND_SEED, fd.APPEND_COUNTS), (fd.TRACE_SEED, fd.TRACE_COUNTS)):
        cov.update(fd.coverage(fd.draw_sweep(seed, counts)))
    for name in sorted(cov):
        print("%4d  %s" % (cov[name], name))
    for name in ("row tiles 1", "row tiles 2", "row tiles 4", "rows per K / V head exactly 17", "rows per K / V head exactly 33", "e4m3 cache, banded",
                 "e4m3 cache, windowless", "16-bit cache, banded", "16-bit cache, windowless", "paged with shared pages", "contiguous capacity below one tile",
                 "a length equal to the capacity", "an all-empty part under a forced split", "lo on a tile edge",
                 "window_left = capacity_keys - 1: the plain route", "window_left = capacity_keys - 2: the banded route", "rotary dim 48, GPT-J",
                 "rotary dim D, GPT-NeoX", "a short rotary table", "trace with a recycle", "trace with a window crossing a page"):
        assert name in cov, name
    assert len(cov) >= 60 and not [n for n, c in cov.items() if c < 1]


# ---- the plan mirror against the header's rule, by hand: (B, Hkv, Nq, G, capacity_keys, window_left, num_splits, CUs) -> (row_tiles, nsplit)
PLAN_TABLE = [
    ((1, 8, 1, 4, 8192, -1, 0, 256), (1, 16)),       # 8 workgroups: 2 * 256 / 8 = 64 -> 16, and 256 tiles / 8 = 32 allow it
    ((32, 8, 1, 4, 4096, -1, 0, 256), (1, 1)),       # 256 workgroups cover 256 CUs
    ((1, 1, 1, 1, 700, -1, 0, 256), (1, 2)),         # 22 tiles: 22 / 8 = 2 parts
    ((1, 1, 1, 1, 255, -1, 0, 256), (1, 1)),         # 8 tiles would be one part of 8; 255 keys are 8 tiles -> 1
    ((1, 1, 1, 1, 257, -1, 0, 256), (1, 1)),         # 9 tiles / 8 = 1
    ((3, 4, 3, 4, 100, -1, 0, 256), (1, 1)),         # 12 rows, 4 tiles: no split
    ((2, 2, 4, 5, 2048, -1, 0, 256), (2, 8)),        # 20 rows -> 2 row tiles; work 8: 64 -> 16; 64 tiles / 8 = 8
    ((2, 1, 3, 11, 4096, -1, 0, 256), (4, 16)),      # 33 rows -> 3 -> 4 row tiles; work 8; 128 tiles / 8 = 16
    ((1, 2, 8, 8, 1024, -1, 0, 304), (4, 4)),        # 64 rows, work 8 on 304 CUs: 76 -> 16; 32 tiles / 8 = 4
    ((1, 1, 1, 17, 4096, 100, 0, 256), (2, 1)),      # a window of 100 keys: span ceil(101 / 32) + 1 = 5 tiles -> 5 / 8 = 0 -> 1
    ((1, 1, 2, 1, 4096, 1000, 0, 256), (1, 4)),      # span ceil(1002 / 32) + 1 = 33 tiles -> 4
    ((1, 1, 1, 1, 64, 5000, 0, 256), (1, 1)),        # a window wider than the cache changes nothing: 2 tiles
    ((9, 8, 2, 8, 1000, 31, 7, 256), (1, 7)),        # forced
    ((1, 1, 8, 8, 1, -1, 16, 256), (4, 16)),         # forced, more parts than key tiles
]


def test_plan_mirror(fd, decode_slice):
    for args, want in PLAN_TABLE:
        assert fd.plan_mirror(*args) == want, (args, fd.plan_mirror(*args), want)
    assert fd.workspace_mirror(2, 3, 4, 5, 128, 1) == 0 and fd.workspace_mirror(2, 3, 4, 5, 128, 7) == 2 * 3 * 7 * 20 * 129 * 4
    # the library's host functions, which see 256 CUs without a device
    lib = _fa2_lib.load()
    for d, _, _ in decode_slice:
        H, ck = d["Hkv"] * d["G"], fd.cap_keys_of(d)
        plan = _fa2_lib.decode_window_plan(_fa2_lib.FA2_DTYPE_F16, d["B"], H, d["Hkv"], d["Nq"], d["D"], d["capacity"], d["page"], d["num_splits"], d["window_left"])
        want = fd.plan_mirror(d["B"], d["Hkv"], d["Nq"], d["G"], ck, d["window_left"], d["num_splits"], fd.device_cus())
        assert (plan.row_tiles, plan.nsplit) == want and plan.key_tile == TILE, (d, want)
        need = lib.fa2_fwd_decode_window_workspace_bytes(_fa2_lib.FA2_DTYPE_F16, d["B"], H, d["Hkv"], d["Nq"], d["D"], d["capacity"], d["page"], d["num_splits"],
                                                         d["window_left"])
        assert need == fd.workspace_mirror(d["B"], d["Hkv"], d["Nq"], d["G"], d["D"], plan.nsplit)


# ---- float64 mutants of the decode contract: wrong kernels the checker must flag.  Each returns the mutant's (O [H, Nq, D], lse [H, Nq]) for
# sequence b, or None where it does not apply.
def _pos(n, nq):
    return n - nq + torch.arange(nq)


def _t(d, inp, p, **kw):
    a = dict(q=p["q"], k=p["k"], v=p["v"], wl=d["window_left"], slopes=p["slopes"], keep=None, pos=None, cap_last=False)
    a.update(kw)
    return wr.truth64(a["q"], a["k"], a["v"], inp["scale"], a["wl"], d["softcap"], a["slopes"], keep=a["keep"], pos=a["pos"], cap_last=a["cap_last"])


def _key_at_len(fd, d, inp, b, p):
    n, nq = d["lens"][b], d["Nq"]
    if n >= fd.cap_keys_of(d):
        return None
    p2 = fd.seq_parts(d, inp, b, n=n + 1)
    keep = torch.cat([wr.keep_mask(n, nq, d["window_left"]), (_pos(n, nq) >= 0)[:, None]], dim=1)
    return _t(d, inp, p, k=p2["k"], v=p2["v"], keep=keep, pos=_pos(n, nq))


def _key_below_lo(fd, d, inp, b, p):
    n, nq = d["lens"][b], d["Nq"]
    lo = wr.window_lo(n, nq, d["window_left"])
    if lo < 1:
        return None
    keep = wr.keep_mask(n, nq, d["window_left"])
    keep[:, lo - 1] = True
    return _t(d, inp, p, keep=keep)


def _window_off_by_one(fd, d, inp, b, p):
    return _t(d, inp, p, wl=d["window_left"] + 1) if d["window_left"] >= 0 else None


def _position_i(fd, d, inp, b, p):
    n, nq, wl = d["lens"][b], d["Nq"], d["window_left"]
    if n <= nq:
        return None
    pos, j = torch.arange(nq)[:, None], torch.arange(n)[None, :]
    keep = (j <= pos) & (j >= pos - wl if wl >= 0 else torch.ones_like(j, dtype=torch.bool))
    return _t(d, inp, p, keep=keep, pos=torch.arange(nq))


def _slopes_by_kv_head(fd, d, inp, b, p):
    if p["slopes"] is None or d["G"] < 2:
        return None
    return _t(d, inp, p, slopes=p["slopes"][torch.arange(d["Hkv"] * d["G"]) // d["G"]])


def _slopes_of_batch_0(fd, d, inp, b, p):
    return _t(d, inp, p, slopes=inp["slopes"][0]) if d["slopes"] == "BH" and b > 0 else None


def _cap_after_alibi(fd, d, inp, b, p):
    return _t(d, inp, p, cap_last=True) if d["softcap"] > 0 and p["slopes"] is not None else None


def _v_descale_dropped(fd, d, inp, b, p):
    return _t(d, inp, p, v=p["vraw"].double()) if p["vd"] is not None else None


def _k_descale_of_the_neighbour(fd, d, inp, b, p):
    if p["kd"] is None or d["Hkv"] < 2:
        return None
    other = inp["kd"][b].roll(1).repeat_interleave(d["G"])[:, None, None]
    return _t(d, inp, p, k=p["kraw"].double() * other.double())


def _rows_in_g_i_order(fd, d, inp, b, p):
    Hkv, G, nq = d["Hkv"], d["G"], d["Nq"]
    if G < 2 or nq < 2:
        return None
    o, lse = _t(d, inp, p)
    # row r = i * G + g of a K / V head holds (i, g); the mutant stores it where r = g' * Nq + i' points
    o2 = o.reshape(Hkv, G, nq, -1).permute(0, 2, 1, 3).reshape(Hkv, G, nq, -1).reshape(Hkv * G, nq, -1)
    l2 = lse.reshape(Hkv, G, nq).permute(0, 2, 1).reshape(Hkv, G, nq).reshape(Hkv * G, nq)
    return o2, l2


def _private_pages_swapped(fd, d, inp, b, p):
    if not d["page"] or d["B"] < 2:
        return None
    n, page = d["lens"][b], d["page"]
    shared = d["share"][2] if d["share"] and b in d["share"][:2] else 0
    for c in range(d["B"]):
        cs = d["share"][2] if d["share"] and c in d["share"][:2] else 0
        j = max(shared, cs)
        if c != b and j * page < min(n, d["lens"][c]):
            pc = fd.seq_parts(d, inp, c, n=n)
            k, v = p["k"].clone(), p["v"].clone()
            k[:, j * page:(j + 1) * page], v[:, j * page:(j + 1) * page] = pc["k"][:, j * page:(j + 1) * page], pc["v"][:, j * page:(j + 1) * page]
            return _t(d, inp, p, k=k, v=v)
    return None


def _last_tile_dropped(fd, d, inp, b, p):
    n, nq = d["lens"][b], d["Nq"]
    if n <= TILE:
        return None
    keep = wr.keep_mask(n, nq, d["window_left"])
    keep[:, TILE * ((n - 1) // TILE):] = False
    return _t(d, inp, p, keep=keep)


MUTANTS = {"one key at len kept": _key_at_len, "one key at lo - 1 kept": _key_below_lo, "the window off by one": _window_off_by_one,
           "the position taken as i": _position_i, "slopes indexed by the K / V head": _slopes_by_kv_head, "batch 0's slopes for every sequence": _slopes_of_batch_0,
           "the cap applied after the ALiBi term": _cap_after_alibi, "v_descale dropped": _v_descale_dropped,
           "k_descale of the neighbouring head": _k_descale_of_the_neighbour, "rows of a group in (g, i) order": _rows_in_g_i_order,
           "two sequences' private pages swapped": _private_pages_swapped, "the last key tile dropped": _last_tile_dropped}


def distance_in_bars(mut, r):
    """how far a mutant (O, lse) lies from the truth of a sequence, in units of its bars: the larger of O and LSE; a row dead in one and live in the other: inf"""
    (to, tl), (obar, lbar) = r["true"], r["bars"]
    dist = (mut[0] - to).abs().max().item() / obar
    dead_t, dead_m = torch.isinf(tl), torch.isinf(mut[1])
    if not torch.equal(dead_t, dead_m):
        return float("inf")
    if (~dead_t).any():
        dist = max(dist, (mut[1][~dead_t] - tl[~dead_t]).abs().max().item() / lbar)
    return dist


def mutant_census(fd, cases, mutants=MUTANTS):
    """per mutant: [cases it applies to, cases where it lies >= MARGIN bars from the truth, of those the ones the checker flags]"""
    tally = {m: [0, 0, 0] for m in mutants}
    for d, inp, refs in cases:
        o, lse = fd.emulated_outputs(d, refs)
        assert not fd.checked(o, lse, refs, d["i"]), (d, "the emulation itself passes everywhere")
        order = sorted((b for b, n in enumerate(d["lens"]) if n), key=lambda b: -d["lens"][b])
        for name, fn in mutants.items():
            best = None
            for b in order[:3]:                                  # the longest sequences: where a mutant applies it shows there if anywhere
                mut = fn(fd, d, inp, b, fd.seq_parts(d, inp, b))
                if mut is not None:
                    dist = distance_in_bars(mut, refs[b])
                    if best is None or dist > best[0]:
                        best = (dist, b, mut)
            if best is None:
                continue
            tally[name][0] += 1
            if best[0] >= MARGIN:
                tally[name][1] += 1
                o2, l2 = o.clone(), lse.clone()
                o2[best[1]], l2[best[1]] = best[2][0].transpose(0, 1), best[2][1]
                tally[name][2] += bool(fd.checked(o2, l2, refs, d["i"]))
    return tally


def test_checker_flags_float64_mutants_of_the_decode_contract(fd, decode_slice):
    tally = mutant_census(fd, decode_slice)
    for name, (applies, far, flagged) in tally.items():
        print("%-42s applies to %3d of %d cases, >= %g bars from the truth on %3d, flagged on %3d" % (name, applies, len(decode_slice), MARGIN, far, flagged))
    assert all(far >= 1 and flagged == far for _, far, flagged in tally.values()), tally


def live_features(fd, cases):
    """(cases that draw a window that is not the plain route, a cap or slopes; those whose float64 differs from the plain call's by >= MARGIN bars in some sequence)"""
    drawn = [(d, refs) for d, _, refs in cases if fd.banded(d)]
    return len(drawn), sum(max(wr.margins(refs)) >= MARGIN for d, refs in drawn)


def trace_walk(fd, d, upto=None):
    """the CPU side of a trace up to and including step `upto` (the last one by default) -> (trace, rotated q of that step)"""
    tr = fd.Trace(d)
    for s in range(d["steps"] if upto is None else upto + 1):
        q, k, v = tr.begin_step(s)
        q_rot = tr.apply_step(q, k, v)
    return tr, q_rot


def test_drawn_features_are_not_idle(fd, decode_slice):
    drawn, live = live_features(fd, decode_slice)
    print("decode: %d cases draw a window, a cap or slopes; %d differ from the plain call by >= %g bars" % (drawn, live, MARGIN))
    assert drawn >= 60 and live >= 0.8 * drawn, (drawn, live)
    drawn = live = 0
    for d in fd.draw_sweep(fd.TRACE_SEED, fd.TRACE_COUNTS):
        if fd.banded(d):
            tr, q_rot = trace_walk(fd, d)
            drawn += 1
            live += max(wr.margins(tr.refs(q_rot))) >= MARGIN
    print("traces: %d draw a window, a cap or slopes; %d differ from the plain call at their last step" % (drawn, live))
    assert drawn >= 3 and live >= 0.8 * drawn, (drawn, live)


def test_checker_flags_a_recycled_pages_stale_keys(fd):
    """A trace's mutant: the keys the page holds behind the sequence's last one — the previous owner's, finite — take part.  At the first step after a
    recycle at which the new sequence does not end on a page edge."""
    far = 0
    for d in fd.draw_sweep(fd.TRACE_SEED, fd.TRACE_COUNTS):
        step, slot, _ = d["events"][0]
        tr, q_rot = trace_walk(fd, d, upto=step)
        assert slot in tr.recycled
        n, nq, page = tr.lens[slot], d["Nq"], d["page"]
        if n % page == 0:
            continue
        end = -(-n // page) * page
        p = tr.parts(slot, q_rot, n=end)
        assert torch.isfinite(p["k"]).all() and torch.isfinite(p["v"]).all(), "stale keys are finite: the quiet failure"
        keep = torch.cat([wr.keep_mask(n, nq, d["window_left"]), (_pos(n, nq) >= 0)[:, None].expand(nq, end - n)], dim=1)
        mut = wr.truth64(p["q"], p["k"], p["v"], tr.scale, d["window_left"], d["softcap"], p["slopes"], keep=keep, pos=_pos(n, nq))
        refs = tr.refs(q_rot)
        dist = distance_in_bars(mut, refs[slot])
        if dist >= MARGIN:
            far += 1
            B, H = d["B"], tr.H
            o, lse = torch.zeros((B, nq, H, d["D"]), dtype=torch.float64), torch.zeros((B, H, nq), dtype=torch.float64)
            for b, r in enumerate(refs):
                o[b], lse[b] = r["emu"][0].transpose(0, 1), r["emu"][1]
            assert not fd.checked(o, lse, refs, d["i"])
            o[slot], lse[slot] = mut[0].transpose(0, 1), mut[1]
            assert fd.checked(o, lse, refs, d["i"]), (d["i"], dist)
    assert far >= 1


def test_shrink_keeps_what_fails_and_drops_the_rest(fd, decode_slice):
    """shrink on a pretended failure (`the case holds a sequence of exactly the capacity`): what is left still fails, is a legal draw, and is smaller"""
    shrunk = 0
    for d, _, _ in decode_slice[:40]:
        ck = fd.cap_keys_of(d)
        fails = lambda c: ck in c["lens"]         # noqa: E731
        if not fails(d):
            continue
        s = fd.shrink(d, fails)
        assert fails(s) and len(s["lens"]) == s["B"] <= d["B"] and s["q_layout"] == s["cache_layout"] == "plain" and s["amp"] == 1.0
        if s["share"]:
            a, b, n = s["share"]
            assert a != b and max(a, b) < s["B"] and (s["lens"][a], s["lens"][b]) == (d["lens"][d["share"][0]], d["lens"][d["share"][1]])
        else:
            assert s["B"] == 1
        inp = fd.build_decode(s)                                     # the shrunk case still builds: caches, block table, references
        fd.physical_caches(s, inp)
        assert len(fd.decode_refs(s, inp)) == s["B"]
        shrunk += s["B"] < d["B"]
    assert shrunk >= 5


def test_every_slot_no_row_may_see_is_nan_and_every_other_holds_its_key(fd, decode_slice):
    """The caches as the device gets them: read back through the block table, a sequence finds its own keys in [lo, len) bit for bit; every other slot of
    the pool — beyond a length, below a window, spare and freed pages, behind unused entries — holds NaN (0x7f) unless another sequence sees it."""
    shared_seen = nan_slots = 0
    for d, inp, _ in decode_slice:
        pk, pv, bt = fd.physical_caches(d, inp)
        page, nq, wl = d["page"], d["Nq"], d["window_left"]
        assert bt is None or (bt.shape == (d["B"], d["capacity"] + d["bt_pad"]) and 0 <= int(bt.min()) and int(bt.max()) < pk.shape[0])
        for phys, logical in ((pk, inp["kc"]), (pv, inp["vc"])):
            raw, want = fd._raw(phys), fd._raw(logical)
            nan = fd._raw(fd._nan_like(phys[:1, :1]))[0, 0]
            seen = torch.zeros(raw.shape[:2], dtype=torch.bool)
            for b, n in enumerate(d["lens"]):
                lo = wr.window_lo(n, nq, wl)
                j = torch.arange(lo, n)
                where = (torch.full_like(j, b), j) if not page else (bt[b, j // page].long(), j % page)
                assert torch.equal(raw[where], want[b, lo:n]), (d["i"], b)
                shared_seen += int(seen[where].sum())
                seen[where] = True
            assert bool((raw[~seen] == nan).all()), (d["i"], "a slot nobody sees holds something else than NaN")
            nan_slots += int((~seen).sum())
            if page:                                              # entries no row reads name a valid all-NaN page
                for b, n in enumerate(d["lens"]):
                    used = set(range(wr.window_lo(n, nq, wl) // page, -(-n // page)))
                    for j in set(range(bt.shape[1])) - used:
                        assert not seen[int(bt[b, j])].any(), (d["i"], b, j)
    assert shared_seen > 0 and nan_slots > 0


# ---- the references against each other and against the library's host side
def test_a_traces_image_after_its_prompt_is_the_append_references(fd):
    for d in fd.draw_sweep(fd.TRACE_SEED, fd.TRACE_COUNTS)[:3]:
        tr = fd.Trace(d)
        twin = torch.Generator().manual_seed(d["seed"])                     # the trace's own stream: the pool, the descales, then one prompt per slot
        for _ in range(2):
            torch.randn((d["B"] * d["capacity"] + 3, d["page"], d["Hkv"], d["D"]), generator=twin)
        if d["fp8"]:
            for _ in range(2):
                torch.rand((d["B"], d["Hkv"]), generator=twin)
        for b, n in enumerate(d["prompts"]):
            k, v = (torch.randn((1, n, d["Hkv"], d["D"]), generator=twin).to(tr.dt) for _ in range(2))
            # the append mode's path: a pattern pool, the block table of the slot, append_expected
            desc = dict(mode="append", lens=[n], Nnew=n, page=d["page"], capacity=d["capacity"], inter=d["inter"], fp8=d["fp8"])
            inp = dict(k=k, v=v, q=None, cos=tr.cos, sin=tr.sin, kd=None if tr.kd is None else tr.kd[b:b + 1], vd=None if tr.vd is None else tr.vd[b:b + 1],
                       bt=tr.bt[b:b + 1])
            pools = [torch.zeros_like(t) for t in tr.pool]
            fd.append_expected(desc, inp, pools)
            for pool, got in zip(pools, tr.gather(b, n)):
                want = torch.cat([pool[int(tr.bt[b, j])] for j in range(-(-n // d["page"]))])[:n]
                assert torch.equal(fd._raw(got), fd._raw(want)), (d["i"], b)
            assert tr.lens[b] == n and sorted(tr.owned[b]) == list(range(-(-n // d["page"])))


def _rotary_eval(x, cos, sin, rot, inter, dt):
    """fa2_rotary_eval on one row (tests/test_kvappend.py's)"""
    lib = _fa2_lib.load()
    xb, y = x.contiguous().view(torch.int16), torch.zeros(x.numel(), dtype=torch.int16)
    c, s = cos.float().contiguous(), sin.float().contiguous()
    fp = ctypes.POINTER(ctypes.c_float)
    rc = lib.fa2_rotary_eval(_fa2_lib.FA2_DTYPE_F16 if dt == torch.float16 else _fa2_lib.FA2_DTYPE_BF16, xb.data_ptr(), ctypes.cast(c.data_ptr(), fp),
                             ctypes.cast(s.data_ptr(), fp), x.numel(), rot, int(inter), y.data_ptr())
    assert rc == 0, rc
    return y


def test_append_reference_is_the_host_side_arithmetic_bit_for_bit(fd):
    """tests/kvappend_refs.py: append_rows (16-bit cache) against fa2_rotary_eval, the function the kernel shares with the host, on rows of every append
    case of the slice that rotates."""
    rows = 0
    for d in fd.draw_sweep(fd.APPEND_SEED, fd.APPEND_COUNTS):
        if not d["rot"]:
            continue
        inp = fd.build_append(d)
        rk, _, _ = kr.append_rows(inp["k"], inp["v"], d["lens"], cos=inp["cos"], sin=inp["sin"], inter=d["inter"])
        for b, n in enumerate(d["lens"]):
            for i in (0, d["Nnew"] - 1):
                row = min(max(n - d["Nnew"] + i, 0), inp["cos"].shape[0] - 1)
                want = _rotary_eval(inp["k"][b, i, 0], inp["cos"][row], inp["sin"][row], d["rot"], d["inter"], inp["k"].dtype)
                assert torch.equal(rk[b, i, 0].view(torch.int16), want), (d["i"], b, i)
                rows += 1
    assert rows >= 100
