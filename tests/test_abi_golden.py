"""The host layer's answers, replayed from tests/golden/abi_golden.npz (tests/golden/make_abi_golden.py wrote it): every plan and workspace size over
grids that cross the planner's thresholds, and the error code of every single defect and every pair of defects of each launching entry point —
which check wins when two fail is part of the C-ABI's behaviour.  CPU only: no row reaches a launch."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from rocwmma_fattn import _fa2_lib

_spec = importlib.util.spec_from_file_location("make_abi_golden", os.path.join(GOLDEN_DIR, "make_abi_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

FIXTURE = np.load(gen.FIXTURE)
META = json.loads(str(FIXTURE["meta"]))
PLAN_FIELDS = ["rc"] + [n for n, _ in _fa2_lib.FwdPlan._fields_]


def _first_difference(grid, got, want, names):
    bad = np.flatnonzero((got != want).any(axis=1))
    if not len(bad):
        return None
    row = next(r for i, r in enumerate(gen.expand(grid)) if i == bad[0])
    return "%d of %d rows differ; first: %r\n  got  %r\n  want %r" % (len(bad), len(want), row, dict(zip(names, got[bad[0]].tolist())),
                                                                      dict(zip(names, want[bad[0]].tolist())))


@pytest.mark.parametrize("name", sorted(META["plan_grids"]))
def test_plans_are_the_recorded_ones(name):
    grid = META["plan_grids"][name]
    want = FIXTURE["plan_rows"][FIXTURE["plans/" + name]]
    got = gen.run_plan_grid(_fa2_lib.load(), grid)
    assert got.shape == want.shape
    assert _first_difference(grid, got, want, PLAN_FIELDS) is None, _first_difference(grid, got, want, PLAN_FIELDS)


@pytest.mark.parametrize("name", sorted(META["size_grids"]))
def test_workspace_sizes_are_the_recorded_ones(name):
    grid = META["size_grids"][name]
    want = FIXTURE["sizes/" + name]
    got = gen.run_size_grid(_fa2_lib.load(), grid)
    assert got.shape == want.shape
    names = ["fwd", "fwd_gqa", "bwd", "bwd_gqa", "bwd_bias"]
    assert _first_difference(grid, got, want, names) is None, _first_difference(grid, got, want, names)


def test_error_codes_and_their_precedence_are_the_recorded_ones():
    lib = _fa2_lib.load()
    rows, entries, dnames = FIXTURE["errors"], META["entries"], META["defects"]
    assert sorted(entries) == sorted(gen.ENTRIES) and len(rows) > 10000
    # the pointers of these calls are stand-ins: a row may only be replayed if the recorded call failed a check, i.e. never got to a launch
    assert (rows[:, 1] >= 0).all() and (rows[:, 3] < 0).all(), "the fixture holds a row of a launching entry point without an FA2_ERR_* code"
    wrong = []
    for row in rows.tolist():
        got = gen.replay_error_row(lib, entries, dnames, row)
        assert got < 0, "%s with %r got past the checks (code %d)" % (entries[row[0]], [dnames[i] for i in row[1:3] if i >= 0], got)     # stop at once
        if got != row[3]:
            wrong.append((entries[row[0]], dnames[row[1]], dnames[row[2]] if row[2] >= 0 else None, "got %d" % got, "want %d" % row[3]))
    assert not wrong, "%d of %d rows differ, e.g. %r" % (len(wrong), len(rows), wrong[:8])
