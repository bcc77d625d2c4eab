"""Slices of the serving traces of the packed step and of the latent cache inside the driver-run suite (`-m gpu`): tools/fuzz_serving.py.

One fixed seed per family — continuous-batching steps of the fused flash_attention_prefill / flash_attention_prefill_fp8 on a paged pool whose pages
are recycled uncleared, and packed prompt appends plus fused flash_attention_decode_mla steps on a latent pool — every step against float64 over the
CPU's image of the pool, the image itself bit for bit at drawn steps, and the first trace of each slice also replayed from one captured step, bit for
bit against the eager trace.  tests/test_fuzz_serving.py proves on the CPU what these seeds reach and that the checker flags float64 mutants of the
contract by 5 bars.  The long runs are recorded in profiles/fuzz_runs.md."""
import importlib.util
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("_fuzz_serving", os.path.join(ROOT, "tools", "fuzz_serving.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _slice(fs, seed, counts):
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    t0 = time.time()
    descs = fs.draw_sweep(seed, counts)
    descs[0] = dict(descs[0], graph=True)          # (an mla trace is replayed when asked; every step trace is)
    out = [fs.run_case(d) for d in descs]
    bad = [d for d in out if d["fails"]]
    assert not bad, [(d["i"], d["fails"][:3]) for d in bad[:3]] + [bad[0]]
    missing = [name for name, n in fs.coverage(descs).items() if n < 1]
    assert not missing, missing
    assert all(d["steps_run"] == d["steps"] for d in out) and all(d["recycled"] >= 1 for d in out) and out[0]["graph"]
    return out, time.time() - t0


def test_step_traces_slice():
    fs = _tool()
    out, secs = _slice(fs, fs.STEP_SEED, fs.STEP_COUNTS)
    assert len(out) == 6 and sum(d["wrong"] for d in out) == 0
    assert all(d["graph"] and d["fill_checked"] == d["steps"] for d in out), "every step of every trace checked the rows of o at and beyond cu[B]"
    print("step traces: %d steps in %.1f s, worst O err / bar %.3f, worst LSE err %.3g; the unowned rows of o checked on %d steps"
          % (sum(d["steps"] for d in out), secs, max(d["o_ratio"] for d in out), max(d["lse_err"] for d in out), sum(d["fill_checked"] for d in out)))


def test_mla_traces_slice():
    fs = _tool()
    out, secs = _slice(fs, fs.MLA_SEED, fs.MLA_COUNTS)
    assert len(out) == 4 and sum(d["wrong"] for d in out) == 0
    print("mla traces: %d steps in %.1f s, worst O err / bar %.3f, worst LSE err %.3g"
          % (sum(d["steps"] for d in out), secs, max(d["o_ratio"] for d in out), max(d["lse_err"] for d in out)))
