"""What the compiler makes of the shell around the hand-scheduled forward bodies (csrc/fa2_fwd_d128.hip.h; no GPU: tools/shell_cost.py compiles
csrc/fwd_asm.cpp to gfx950 assembly with the product build's flags and reads the result).

  * no instantiation of fwd_asm_kernel has a private segment: nothing is spilled to scratch around the statement;
  * the instructions of the persistent loop outside the generated body — entry and exit of the kernel config 2 runs — stay at most half of what they
    were before the shell located and described each item once and stored interior tiles without predicates.  A guard against the shell growing
    back, not a performance claim.
"""
import functools
import importlib.util
import os
import shutil

import pytest

from conftest import ROOT

# tools/shell_cost.py on commit db508bc (the shell before this change), fwd_asm_kernel<128, false, false, true, true, true>
PARENT_COMMIT = "db508bc"
PARENT_ENTRY = 633
PARENT_EXIT = 605
C2_KERNEL = (128, 0, 0, 1, 1, 1)          # HD, BF16, CAUSAL, FOLD, M16, LM


@functools.lru_cache(maxsize=1)
def _cost():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc") or os.environ.get("HIPCC")):
        pytest.fail("hipcc not found: the shell cannot be compiled")
    spec = importlib.util.spec_from_file_location("_shell_cost", os.path.join(ROOT, "tools", "shell_cost.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.measure()


def test_every_instantiation_is_found():
    res = _cost()
    insts = sorted(r["inst"] for r in res.values())
    assert len(insts) == len(set(insts)) == 40, insts          # fwd_asm.cpp: 16 of head dim 64, 24 of head dim 128
    assert C2_KERNEL in insts
    for r in res.values():
        assert r["private"] is not None and r["entry"] and r["exit"], r


def test_no_private_segment():
    bad = {r["inst"]: r["private"] for r in _cost().values() if r["private"] != 0}
    assert not bad, "fwd_asm_kernel instantiations with scratch (HD, BF16, CAUSAL, FOLD, M16, LM -> bytes per lane): %r" % bad


def test_shell_of_config_2_stays_half_of_what_it_was():
    r = next(r for r in _cost().values() if r["inst"] == C2_KERNEL)
    print("entry %d (was %d), exit %d (was %d at %s)" % (r["entry"], PARENT_ENTRY, r["exit"], PARENT_EXIT, PARENT_COMMIT))
    assert 2 * r["entry"] <= PARENT_ENTRY, (r["entry"], PARENT_ENTRY)
    assert 2 * r["exit"] <= PARENT_EXIT, (r["exit"], PARENT_EXIT)
