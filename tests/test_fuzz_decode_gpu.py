"""Slices of the randomised sweep of the KV-cache serving path inside the driver-run suite (`-m gpu`): tools/fuzz_decode.py.

One fixed seed per family — a single fa2_fwd_decode_window call (plain, e4m3 and banded kernels; contiguous, paged and page-sharing caches), a single
kvcache_append call, and serving traces of append-then-decode steps on recycled, uncleared pages, one of them also replayed from a captured graph.
tests/test_fuzz_decode.py proves on the CPU what these seeds reach, that the checker flags float64 mutants of the contract by 5 bars, and that the
drawn windows, caps and slopes are not idle.  The long runs are recorded in profiles/fuzz_runs.md."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("_fuzz_decode", os.path.join(ROOT, "tools", "fuzz_decode.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _slice(fd, seed, counts, graph_first=False):
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    descs = fd.draw_sweep(seed, counts)
    if graph_first:
        descs[0] = dict(descs[0], graph=True)
    out = [fd.run_case(d) for d in descs]
    bad = [d for d in out if d["fails"]]
    assert not bad, [(d["i"], d["fails"][:3]) for d in bad[:3]] + [bad[0]]
    missing = [name for name, n in fd.coverage(descs).items() if n < 1]
    assert not missing, missing
    return out


def test_randomised_decode_sweep_slice():
    fd = _tool()
    out = _slice(fd, fd.DECODE_SEED, fd.DECODE_COUNTS)
    assert len(out) == 120 and sum(d["operator"] for d in out) == 30 and sum(d["twice"] for d in out) == 30
    print("decode: worst O err / bar %.3f, worst LSE err %.3g; splits run %s" % (max(d["o_ratio"] for d in out), max(d["lse_err"] for d in out),
                                                                              sorted({d["nsplit"] for d in out})))


def test_randomised_append_sweep_slice():
    fd = _tool()
    out = _slice(fd, fd.APPEND_SEED, fd.APPEND_COUNTS)
    assert len(out) == 60 and sum(d["written"] for d in out) > 0 and sum(d["wrong"] for d in out) == 0
    print("append: %d tokens written, 0 elements off the expected image; rotated K against float64 at most %.3f of its bar"
          % (sum(d["written"] for d in out), max(d["o_ratio"] for d in out)))


def test_serving_traces_slice():
    fd = _tool()
    out = _slice(fd, fd.TRACE_SEED, fd.TRACE_COUNTS, graph_first=True)
    assert len(out) == 6 and all(d["steps_run"] == d["steps"] for d in out) and all(d["recycled"] >= 1 for d in out) and out[0]["graph"]
    print("traces: %d steps, worst O err / bar %.3f, worst LSE err %.3g" % (sum(d["steps"] for d in out), max(d["o_ratio"] for d in out),
                                                                         max(d["lse_err"] for d in out)))
