"""References shared by tests/test_lse_gpu.py and tests/test_merge_gpu.py (a helper module like far_layouts.py, not a test file).  The references
themselves live in tools/fuzz_lse.py, the randomised sweep of the same calls, and are re-exported here: one copy for the fixed-shape tests and the sweep.

truth64: dense float64 autograd of the contract with the LSE as a second output — loss = (O * dO).sum() + (lse_live * u).sum(), lse in natural-log
units, u the caller's weights; every route of flash_attention goes through the same few lines: scaled scores, soft-capping, ALiBi, an additive bias,
a keep mask (bool mask and band) as -inf, dropout applied to the probabilities (the LSE is that of the undropped ones).
emulate: the same contract as the kernels run it — f32 scores and sums, P rounded to the I/O dtype where it multiplies V and dO (O, dV), dS = P (dP - delta) (1 - t^2)
formed from the f32 P and rounded to the I/O dtype once, outputs rounded once — with the dQ pass's row term delta - u.  (The fp16 wave-pair dK / dV pass
hands P from one wave to the other in 16 bits, one relative rounding more than here; in fp16 as round16(2^14 P), which keeps that rounding relative
down to P = 2^-28 instead of losing the pair below 2^-25.)
Bars: the project's rule (tools/fuzz_features.py: error_and_bar; FLOOR / GRAD_TOL / LSE_TOL of conftest.py); the LSE is compared in log2 units."""
import importlib.util
import math
import os

import torch

from conftest import FLOOR, GRAD_TOL, LSE_TOL

LN2 = math.log(2.0)
NAMES = ("O", "lse", "dQ", "dK", "dV")

_spec = importlib.util.spec_from_file_location("_fuzz_lse", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "tools", "fuzz_lse.py"))
fl = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fl)
ff = fl.ff                                               # tools/fuzz_features.py: band, keep_unit, p_eff, error_and_bar
assert fl.LSE_TOL == LSE_TOL and all(fl.FLOOR[dt] == FLOOR[c] and fl.GRAD_TOL[dt] == GRAD_TOL[c] for c, dt in enumerate((torch.float16, torch.bfloat16)))
truth64, emulate, fold, bars_of, merge64, merge_check, MERGE_EPS = fl.truth64, fl.emulate, fl.fold, fl.bars_of, fl.merge64, fl.merge_check, fl.MERGE_EPS


def code(dt):
    return 0 if dt == torch.float16 else 1


def check(tag, got, true, bars, names=NAMES):
    """got: name -> tensor (lse in log2 units).  Prints every figure before it asserts."""
    for n in names:
        bar, e_emu = bars[n]
        x, t = got[n].double(), true[n]
        if n == "lse":
            dead = torch.isinf(t)
            assert torch.isneginf(got[n][dead]).all(), (tag, "rows that see no key: lse = -inf exactly")
            x, t = x[~dead], t[~dead]
        assert torch.isfinite(x).all(), (tag, n, "non-finite")
        err = (x - t).abs().max().item() if x.numel() else 0.0
        print("%s %s: err %.3g, emulation %.3g, bar %.3g" % (tag, n, err, e_emu, bar))
        assert err <= bar, (tag, n, err, bar)


def check_not_vacuous(tag, true, without_u, bars):
    """The u term must move the float64 dQ and dK by at least 5 bars (dV does not depend on dlse)."""
    for n in ("dQ", "dK"):
        mg = (true[n] - without_u[n]).abs().max().item() / bars[n][0]
        print("%s %s: the LSE term moves it by %.1f bars" % (tag, n, mg))
        assert mg >= 5.0, (tag, n, mg)
    assert (true["dV"] - without_u["dV"]).abs().max().item() <= 1e-9 * max(1.0, true["dV"].abs().max().item())
