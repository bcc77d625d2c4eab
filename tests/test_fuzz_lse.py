"""CPU tests of tools/fuzz_lse.py, the randomised sweep of the score-modifier, LSE-gradient, merge and chain calls: (a) the draw is pure and stays inside
the operator's limits, (b) the slices the `-m gpu` suite runs (tests/test_fuzz_lse_gpu.py) reach what they are there for and keep the quiet-case cap,
(c) the sweep's checker flags wrong kernels.  "The kernel's output" here is the same-contract emulation (fuzz_lse.emulate, fuzz_lse.merge_emulate) on
shapes capped for the CPU; the plan items of the coverage and the dropout keep mask come from the built library's host functions, which need no GPU."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
CPU_NMAX = 96            # every length of a checker case is capped here
LN2 = 0.6931471805599453


def _tool(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fl():
    return _tool("fuzz_lse")


def _slice(fl, fam):
    return fl.draw_sweep(*fl.SLICES[fam])


# ---- (a) the draw
def test_draw_is_pure_and_inside_the_operators_limits(fl):
    for fam in fl.MODES:
        a, b = _slice(fl, fam), _slice(fl, fam)
        assert a == b and len(a) == sum(n for _, n in fl.SLICES[fam][1]) and all(d["fam"] == fam for d in a)
        assert sum(d["bwd"] for d in a) >= len(a) // 3
        for d in a:
            assert d["dtype"] in ("float16", "bfloat16") and d["D"] % 8 == 0 and 8 <= d["D"] <= 512
            if fam == "merge":
                assert 1 <= d["nparts"] <= (16 if d["via"] == "abi" else 40) and 1 <= d["Nq"] <= 512 and d["B"] <= 2 and d["H"] <= 8
                assert d["natural"] or d["via"] == "abi"
                continue
            assert d["H"] <= 8 and d["H"] % d["Hkv"] == 0 and d["rows"] in (0, 128, 256) and d["softcap"] in fl.SOFTCAPS
            assert not (d["p"] > 0 and (d["softcap"] > 0 or d["slopes"] is not None)) and not (d["mask"] is not None and (d["p"] > 0 or d["softcap"] > 0 or d["slopes"] is not None))
            if fam == "scoremod":
                assert d["softcap"] > 0 or d["slopes"] is not None
            lens = d["lens_q"] + d["lens_k"] if d["mode"] == "packed" else [d["Nq"], d["Nkv"]]
            if d.get("kind") != "split":           # the slices' sizes: a few seconds per test
                assert max(lens) <= (300 if d["D"] > 256 else 700)
            else:
                assert d["B"] == 1 and d["H"] <= 2 and d["D"] == 64 and d["Nkv"] == fl.kv_split_nkv(d["H"], d["Nq"])
            if d["mode"] == "dense":
                assert 1 <= d["B"] <= 2 and d["q_offset"] >= 0 and min(lens) >= 1
            if d["mask"] is not None:
                assert d["D"] <= 256
            if fam == "chain":
                cuts = d["cuts"]
                assert 1 <= len(cuts) <= 5 and cuts == sorted(set(cuts)) and 0 < cuts[0] and cuts[-1] < d["Nkv"] and d["q_offset"] >= cuts[-1]
    assert sum(d.get("kind") == "split" for d in _slice(fl, "lse")) <= 2


# ---- (b) coverage and the quiet-case cap, from the draw and the references alone
def test_slices_reach_what_they_are_there_for(fl):
    names = 0
    for fam in fl.MODES:
        cov = fl.coverage(_slice(fl, fam))
        for name in sorted(cov):
            print("%-9s %4d  %s" % (fam, cov[name], name))
        assert not [n for n, c in cov.items() if c < 1], fam
        names += len(cov)
    cov = fl.coverage(_slice(fl, "lse"))
    assert "plan: KV-split parts take a dlse" in cov and "plan: the short dQ kernel takes a dlse" in cov and names >= 60


def _cpu_case(fl, d, gen):
    d = fl.shrink(d, CPU_NMAX)
    inp = fl.build_case(d, gen)
    refs, margin = fl.references(d, inp)
    if d["fam"] == "chain":
        refs = fl.chain_emulation(d, inp, refs)
    return d, inp, refs, margin


def test_quiet_cases_stay_under_the_cap_on_shrunk_shapes(fl):
    """The modifiers (scoremod) and u (lse) must move a float64 output by QUIET_BARS bars in three quarters of a slice's cases.  Here on the shapes
    capped for the CPU; the GPU slices assert the same on the drawn shapes, where distances (ALiBi) and row counts are larger."""
    for fam in ("scoremod", "lse"):
        gen = torch.Generator().manual_seed(fl.SLICES[fam][0])
        res = [dict(margin=_cpu_case(fl, d, gen)[3]) for d in _slice(fl, fam)]
        quiet, n = fl.quiet_share(res)
        print("%s: %d of %d cases with a margin are quiet" % (fam, quiet, n))
        assert n >= 20 and quiet <= fl.QUIET_CAP * n, (fam, quiet, n)


# ---- (c) mutants of the emulation: wrong kernels the checker must flag.  Each returns what replaces a unit's modifiers / u / flags, or None where it changes nothing.
def _differs(a, b):
    return a is not None and not torch.equal(a, b)


def _mutants(fl):
    ff = fl.ff
    g = lambda d: d["H"] // d["Hkv"]                                       # noqa: E731
    sl = lambda r: r["kw"]["slopes"]                                       # noqa: E731
    live_u = lambda d, r: d["bwd"] and r["u"] is not None                  # noqa: E731

    def by_kv_head(d, inp, b, r):
        if sl(r) is None or g(d) == 1:
            return None
        new = sl(r)[(torch.arange(d["H"]) // g(d))]
        return dict(slopes=new) if _differs(new, sl(r)) else None

    def of_batch_0(d, inp, b, r):
        if sl(r) is None or inp["slopes"].dim() == 1 or b == 0:
            return None
        return dict(slopes=inp["slopes"][0]) if _differs(inp["slopes"][0], sl(r)) else None

    def no_offset(packed):
        def fn(d, inp, b, r):
            if sl(r) is None or r["kw"]["off"] == 0 or (d["mode"] == "packed") != packed or not sl(r).any():
                return None
            return dict(off=0)
        return fn

    def dead_rows_alive(d, inp, b, r):
        return dict(mut=("cap_after_mask",)) if d["softcap"] > 0 and not r["allow"].all() else None

    def packed_u_without_offset(d, inp, b, r):
        q0, nq = inp["units"][b].get("q0", 0), r["q"].shape[1]
        if not live_u(d, r) or d["mode"] != "packed" or q0 == 0:
            return None
        return dict(u=torch.nan_to_num(inp["u"][:, :nq], nan=0.0))

    return {
        "slope taken by K / V head": by_kv_head,
        "slope of batch 0 for every batch": of_batch_0,
        "|pos - j| without q_offset": no_offset(False),
        "packed offset dropped from the slope distance": no_offset(True),
        "slope sign flipped": lambda d, inp, b, r: dict(slopes=-sl(r)) if sl(r) is not None and sl(r).any() else None,
        "cap applied after the mask": dead_rows_alive,
        "(1 - t^2) omitted from dX": lambda d, inp, b, r: dict(mut=("no_fac",)) if d["softcap"] > 0 and d["bwd"] else None,
        "dlse dropped": lambda d, inp, b, r: dict(u=None) if live_u(d, r) else None,
        "dlse scaled by ln 2": lambda d, inp, b, r: dict(u=r["u"] * LN2) if live_u(d, r) else None,
        "dlse applied to dead rows": lambda d, inp, b, r: dict(mut=("dlse_dead",)) if live_u(d, r) and torch.isnan(r["u"]).any() else None,
        "packed dlse without the sequence's row offset": packed_u_without_offset,
    }


def test_checker_flags_mutant_outputs(fl):
    mutants = _mutants(fl)
    applies, caught, total = {m: 0 for m in mutants}, {m: 0 for m in mutants}, 0
    for fam in ("scoremod", "lse"):
        gen = torch.Generator().manual_seed(fl.SLICES[fam][0])
        for d0 in _slice(fl, fam):
            d, inp, refs, _ = _cpu_case(fl, d0, gen)
            total += 1
            fails, _ = fl.check_units(d, refs, fl.emulated_outputs(d, inp))
            assert not fails, (d, fails)                                 # the emulation itself passes everywhere
            for name, fn in mutants.items():
                changed = {b: fn(d, inp, b, r) for b, r in enumerate(inp["refs"]) if r is not None}
                changed = {b: m for b, m in changed.items() if m is not None}
                if not changed:
                    continue
                applies[name] += 1
                fails, _ = fl.check_units(d, refs, fl.emulated_outputs(d, inp, mutate=lambda b, r: changed.get(b)))
                caught[name] += bool(fails)
    for name in mutants:
        print("%-48s applies to %3d of %d cases, caught on %3d (%.0f %%)" % (name, applies[name], total, caught[name], 100.0 * caught[name] / max(applies[name], 1)))
    assert all(applies[m] >= 1 and caught[m] >= 1 for m in mutants), (applies, caught)


MERGE_MUTANTS = {
    "merge weights from natural-log LSEs where log2 was flagged": ("natural_weights", lambda d: not d["natural"] and d["nparts"] > 1),
    "merge dlse_k without its dO.(O_k - O) term": ("no_dot_term", lambda d: d["nparts"] > 1),
    "merge reading part k + 1's LSE": ("next_lse", lambda d: d["nparts"] > 1),
}


def _merge_emulated(fl, d, mi, mut=()):
    dt = getattr(torch, d["dtype"])
    vo, _ = fl._views(d["layout"])
    out, lse, dos, dls = fl.merge_emulate([o["view"] for o in mi["outs"]], mi["lses"], vo(mi["dout"]), mi["dlse"] if d["dlse"] else None, d["natural"], dt, mut)
    return [out, lse, dos, dls] if d["bwd"] else [out, lse]


def test_merge_checker_passes_the_emulation_and_flags_its_mutants(fl):
    gen = torch.Generator().manual_seed(fl.SLICES["merge"][0])
    applies, caught = {m: 0 for m in MERGE_MUTANTS}, {m: 0 for m in MERGE_MUTANTS}
    descs = [fl.shrink(d, CPU_NMAX) for d in _slice(fl, "merge")]
    for d in descs:
        if d["nparts"] > 16:               # the folds are the operator's: the emulation is one kernel call
            continue
        mi = fl.merge_inputs(d, gen)
        fails, _ = fl.check_merge(d, mi, _merge_emulated(fl, d, mi))
        assert not fails, (d, fails)
        for name, (mut, cond) in MERGE_MUTANTS.items():
            if not cond(d):
                continue
            applies[name] += 1
            caught[name] += bool(fl.check_merge(d, mi, _merge_emulated(fl, d, mi, (mut,)))[0])
    for name in MERGE_MUTANTS:
        print("%-60s applies to %3d of %d cases, caught on %3d (%.0f %%)" % (name, applies[name], len(descs), caught[name], 100.0 * caught[name] / max(applies[name], 1)))
    assert all(caught[m] >= 1 for m in MERGE_MUTANTS), caught
    assert fl.merge_folds(16) == 1 and fl.merge_folds(17) == 2 and fl.merge_folds(31) == 2 and fl.merge_folds(32) == 3 and fl.merge_folds(40) == 3


def test_chain_emulation_passes_and_a_lost_part_is_flagged(fl):
    """The path emulation of a chain case (parts, merge, the gradient through both) stays inside the bars against float64 over the whole KV axis; the
    same emulation with the first live chunk left out of the merge does not."""
    gen = torch.Generator().manual_seed(fl.SLICES["chain"][0])
    caught = n = 0
    for d0 in _slice(fl, "chain"):
        d, inp, refs, _ = _cpu_case(fl, d0, gen)
        dt = getattr(torch, d["dtype"])
        got = [{k: (r["emu"][k].float() if k == "lse" else r["emu"][k].to(dt)) for k in fl.NAMES} for r in refs]
        fails, _ = fl.check_units(d, refs, got)
        assert not fails, (d, fails)
        ref0, c1 = inp["refs"][0], d["cuts"][0]
        if not ref0["allow"][:, :c1].any():               # (nobody sees the first chunk: losing it changes nothing)
            continue
        n += 1
        e = fl.emulate(ref0["q"], ref0["ke"][:, c1:], ref0["ve"][:, c1:], ref0["do"], None, ref0["allow"][:, c1:], fl.ff.scale_of(d), dt,
                       **dict(ref0["kw"], off=ref0["kw"]["off"] - c1))
        wrong = dict(got[0], O=e["O"].to(dt), lse=e["lse"].float())
        caught += bool(fl.check_units(d, refs[:1], [wrong])[0])
    print("a chain that loses its first chunk: flagged in %d of %d cases" % (caught, n))
    assert caught >= 1
