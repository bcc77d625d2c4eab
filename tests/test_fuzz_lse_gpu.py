"""Slices of tools/fuzz_lse.py, the randomised float64 sweep of the score-modifier, LSE-gradient, merge and chain calls, inside the driver-run suite
(`-m gpu`).  One test per family on the seeds and counts of fuzz_lse.SLICES, whose draw tests/test_fuzz_lse.py proves on the CPU to reach every
coverage item: no failing case, every coverage item reached, at most a quarter of the cases quiet (the modifiers, or u, move no float64 output by
five bars).  The slices draw at the smallest shapes that still reach the code: lengths up to 700 (300 above head dim 256), B <= 2, H <= 8; the two
KV-split cases sit at the smallest Nkv for which the library reports a split.  The committed long runs live in profiles/fuzz_runs.md.
Reduced calls of cases a sweep found failing stand below their family's slice."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fl():
    if not torch.cuda.is_available():
        pytest.fail("these tests need a ROCm device")
    return _tool("fuzz_lse")


def _family_slice(fl, fam):
    seed, counts = fl.SLICES[fam]
    gen = torch.Generator(device="cuda").manual_seed(seed)
    descs = fl.draw_sweep(seed, counts)
    out = [fl.run_case(d, gen) for d in descs]
    for k in ("o_ratio", "grad_ratio", "lse_ratio"):
        print("%s: worst %s %.3f" % (fam, k, max(r.get(k, 0.0) for r in out)))
    bad = [r for r in out if r["fails"]]
    assert not bad, bad[:3]
    missing = [name for name, n in fl.coverage(out).items() if n < 1]
    assert not missing, missing
    quiet, n = fl.quiet_share(out)
    print("%s: %d of %d cases with a margin are quiet" % (fam, quiet, n))
    assert fam not in ("scoremod", "lse") or quiet <= fl.QUIET_CAP * n, (quiet, n)          # (the cap is a condition on these two draws)
    return out


def test_score_modifier_sweep_slice(fl):
    out = _family_slice(fl, "scoremod")
    assert len(out) == 56 and sum(r["bwd"] for r in out) == 28 and all(r["margin"] is not None for r in out)


def test_lse_gradient_sweep_slice(fl):
    out = _family_slice(fl, "lse")
    assert len(out) == 72 and sum(r["bwd"] for r in out) >= 36
    # the plans the backward cases ran, as the library names them: the short dQ kernel, the D = 128 fallback, the KV-split parts
    plans = [r["plan"] for r in out if r.get("plan") is not None]
    assert any(p[0] == fl._fa2_lib.FA2_BWD_KERNEL_SHORT for p in plans) and sum(p[2] for p in plans) == 2, plans


def test_merge_sweep_slice(fl):
    out = _family_slice(fl, "merge")
    assert len(out) == 48 and {r["via"] for r in out} == {"abi", "op"}


def test_chain_sweep_slice(fl):
    out = _family_slice(fl, "chain")
    assert len(out) == 16 and any(r["dead_part"] for r in out)
