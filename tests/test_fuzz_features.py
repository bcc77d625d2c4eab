"""CPU tests of tools/fuzz_features.py, the randomised sweep of the windowed, packed, grouped and dropout calls: that the slices the `-m gpu` suite
runs (tests/test_fuzz_gpu.py) reach what they are there for, that the sweep's checker flags wrong kernels, and that the readback decode returns the
host's mask.  "The kernel's output" here is the same-contract emulation (fuzz_features.emu) on shapes capped for the CPU; the keep mask comes from the
library's host function, which needs the built library and no GPU."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
CPU_NMAX = 96            # every length of a checker case is capped here (readback cases keep their lengths: their blocks lie beyond key 1024 / row 512)


def _tool(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ff():
    return _tool("fuzz_features")


def test_draw_is_pure_and_reproducible(ff):
    a, b = ff.draw_sweep(ff.SLICE_SEED, ff.SLICE_COUNTS), ff.draw_sweep(ff.SLICE_SEED, ff.SLICE_COUNTS)
    assert a == b and len(a) == sum(n for _, n in ff.SLICE_COUNTS)
    assert sum(d["bwd"] for d in a) == len(a) // 2
    for d in a + ff.draw_sweep(ff.READBACK_SEED, ff.READBACK_COUNTS):
        assert d["rows"] in (0, 128, 256) and d["H"] % d["Hkv"] == 0 and 0 <= d["seed"] < 2 ** 64
        if d["mode"] == "dense":
            assert 1 <= d["B"] <= 3 and d["q_offset"] >= 0 and d["Nq"] >= 1 and d["Nkv"] >= 1
            assert d["Nq"] <= 1500 and d["Nkv"] <= (2100 if d["long"] else 1500)
        if d["mode"] == "packed":
            assert 1 <= len(d["lens_q"]) <= 8 and len(d["lens_q"]) == len(d["lens_k"])
            assert sum(n > 600 for n in d["lens_q"]) <= 1 and max(d["lens_q"] + d["lens_k"]) <= 1500


def test_slices_reach_what_they_are_there_for(ff):
    """(a) the draw alone, over the seeds and counts of the two slice tests, meets every coverage minimum."""
    cov = ff.coverage(ff.draw_sweep(ff.SLICE_SEED, ff.SLICE_COUNTS))
    cov.update(ff.coverage(ff.draw_sweep(ff.READBACK_SEED, ff.READBACK_COUNTS)))
    for name in sorted(cov):
        print("%4d  %s" % (cov[name], name))
    assert "dead rows, dense" in cov and "dead rows, packed" in cov and "readback dq packed" in cov and len(cov) >= 30
    assert not [n for n, c in cov.items() if c < 1]


# ---- (b) mutants of the emulation: wrong kernels the checker must flag.  Each returns what replaces a unit's band / keep / rs, or None where it changes nothing.
def _rebanded(ff, desc, t, b, **kw):
    nq, nk, left, right, off = ff.units_of(desc)[b]
    geo = dict(left=left, right=right, off=off)
    geo.update(kw)
    new = ff.band(nq, nk, geo["left"], geo["right"], geo["off"], False)
    return None if torch.equal(new, t["band"]) else dict(band=new)


def _rekeyed(ff, desc, t, b, **kw):
    nq, nk = ff.units_of(desc)[b][:2]
    if ff.threshold(desc["p"]) == 0:
        return None
    new = ff.keep_unit(desc["seed"], desc["p"], desc["H"], b, nq, nk, **kw)
    return None if torch.equal(new & t["band"], t["keep"] & t["band"]) else dict(keep=new)


def _mutants(ff):
    g = lambda d: d["H"] // d["Hkv"]         # noqa: E731
    return {
        "band's left edge off by one": lambda d, inp, b, t: _rebanded(ff, d, t, b, left=ff.units_of(d)[b][2] + 1) if ff.units_of(d)[b][2] >= 0 else None,
        "band's right edge off by one": lambda d, inp, b, t: _rebanded(ff, d, t, b, right=ff.units_of(d)[b][3] + 1) if ff.units_of(d)[b][3] >= 0 else None,
        "top-left where bottom-right was asked": lambda d, inp, b, t: _rebanded(ff, d, t, b, off=0) if d.get("bottom_right") else None,
        "mask keyed by the kv head": lambda d, inp, b, t: _rekeyed(ff, d, t, b, hmap=(d["Hkv"], lambda h: h // g(d))) if g(d) > 1 else None,
        "mask keyed by the packed row": lambda d, inp, b, t: _rekeyed(ff, d, t, b, i0=inp["units"][b]["q0"]) if inp["units"][b].get("q0") else None,
        "rs omitted": lambda d, inp, b, t: dict(rs=1.0) if ff.threshold(d["p"]) > 0 else None,
        "mask of row i + 1": lambda d, inp, b, t: _rekeyed(ff, d, t, b, i0=1),
    }


def test_checker_flags_mutant_outputs(ff):
    descs = [ff.shrink(d, CPU_NMAX) for d in ff.draw_sweep(ff.SLICE_SEED, ff.SLICE_COUNTS)]
    mutants = _mutants(ff)
    applies, caught = {m: 0 for m in mutants}, {m: 0 for m in mutants}
    gen = torch.Generator().manual_seed(ff.SLICE_SEED)
    for d in descs:
        inp = ff.build_inputs(d, gen)
        tr = ff.truths(d, inp)
        fails, _ = ff.check_units(d, inp, tr, ff.emulate(d, inp, tr))
        assert not fails, (d, fails)                                 # the emulation itself passes everywhere
        for name, fn in mutants.items():
            changed = {b: fn(d, inp, b, t) for b, t in enumerate(tr) if t is not None}
            changed = {b: m for b, m in changed.items() if m is not None}
            if not changed:
                continue
            applies[name] += 1
            fails, _ = ff.check_units(d, inp, tr, ff.emulate(d, inp, tr, mutate=lambda b, t: changed.get(b, {})))
            caught[name] += bool(fails)
    for name in mutants:
        print("%-40s applies to %3d of %d cases, caught on %3d (%.0f %%)" % (name, applies[name], len(descs), caught[name],
                                                                           100.0 * caught[name] / max(applies[name], 1)))
    assert all(caught[m] >= 1 for m in mutants), caught


# ---- (c) the readback decode on the emulation's outputs
def _flip_target(ff, desc, b, h, kind):
    """An element (b, h, i, j) inside the block a readback call reads, visible under its band: the block's last one, one in the keys' last partial tile
    or one beyond key 1024; None where the block holds no such element."""
    nq, nk, left, right, off = ff.units_of(desc)[b]
    s0, span = desc["start"], ff.BITS * desc["D"]
    if desc["pass_"] == "dkv":
        i, j = min(s0 + span, nq) - 1, nk - 1
        ok = i >= s0 and (kind == "last" or (kind == "partial" and nk % 64) or (kind == "beyond" and j > 1024))
        return (b, h, i, j) if ok else None
    vis = ff.band(nq, nk, left, right, off, False)[:, s0:s0 + span].nonzero()
    if kind == "partial":
        vis = vis[vis[:, 1] + s0 >= nk - nk % 64]
    if kind == "beyond":
        vis = vis[vis[:, 1] + s0 > 1024]
    return (b, h, int(vis[-1, 0]), int(vis[-1, 1]) + s0) if len(vis) else None


def test_readback_round_trip_and_single_bit_mutants(ff):
    gen = torch.Generator().manual_seed(ff.READBACK_SEED)
    worst, flips = {}, {"last": [0, 0], "partial": [0, 0], "beyond": [0, 0]}
    for d in ff.draw_sweep(ff.READBACK_SEED, ff.READBACK_COUNTS):
        units = ff.readback_inputs(d, gen)
        wrong, total, frac = ff.readback_decode(d, units, ff.readback_emulate(d, units))
        key = (d["dtype"], d["pass_"])
        worst[key] = max(worst.get(key, 0.0), frac)
        assert wrong == 0 and total > 0 and frac <= 0.25, (d, wrong, total, frac)
        lens = [u[0] * u[1] for u in ff.units_of(d)]
        b = lens.index(max(lens))                                     # the unit the block was drawn for
        for kind in flips:
            tgt = _flip_target(ff, d, b, d["member"], kind)           # (head `member` is a coded head of the dK / dV pass and a head like any other elsewhere)
            if tgt is None:
                continue
            flips[kind][0] += 1
            wrong = ff.readback_decode(d, units, ff.readback_emulate(d, units, flip=tgt))[0]
            flips[kind][1] += wrong == 1
            assert wrong == 1, (d, kind, tgt, wrong)                  # exactly the flipped bit
    for (dt, ps), f in sorted(worst.items()):
        print("readback %s %s pass: largest distance of a decoded count from an integer %.4f" % (dt, ps, f))
    print("single-bit mutants caught: %s" % {k: "%d of %d" % (v[1], v[0]) for k, v in flips.items()})
    assert all(v[0] >= 1 and v[0] == v[1] for v in flips.values()), flips
    assert len(worst) == 6, sorted(worst)
