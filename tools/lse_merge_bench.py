"""The differentiable LSE and the merge kernels on the GPU (developer tool; bench.py does not read it) — same box, interleaved rounds, median of
per-round event times (tools/varlen_bench.py practice).

    python tools/lse_merge_bench.py [--rounds R] [--iters I] [--parent PATH/libfa2_gfx950.so] [--skip merge,fallback,parent]

merge     first the two kernels alone through the C-ABI (2, 4, 8, 16 parts), then merge_attention forward and backward (fa2_merge_fwd / fa2_merge_bwd) at 2, 4 and 8 parts of B2 H16 N4096 D128 bf16 against the eager-torch
          composition of the same math (stack / logsumexp / exp / mul / sum, and its autograd): time, bytes moved / time, and the fraction of the
          6.3 TB/s a streaming kernel can reach on the MI355X.  Bytes: forward = the parts' O and LSE read once + the merged pair written; backward = the parts
          and dO read once + the parts' gradients written.
fallback  the backward of config 2 (B2 H16 N4096 D128 fp16 non-causal) through fa2_bwd_lse without a dlse (the hand-scheduled passes) and with one (the
          compiler-scheduled passes): the price of the fallback, i.e. what teaching the generators would buy.
parent    c2 / c3 / c4 backward (fa2_bwd), c2 forward (fa2_fwd) and two head-dim-64 backwards (the compiler-scheduled dQ pass) of this build against
          another build of the library (the parent commit's), interleaved: both numbers and the run-to-run spread (min .. max over the rounds) of each.
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from rocwmma_fattn import _fa2_lib  # noqa: E402
from rocwmma_fattn.FlashAttn import merge_attention  # noqa: E402

PEAK_TBS = 6.3
CFGS = {"c2": (2, 16, 4096, 128, torch.float16, False), "c3": (2, 16, 4096, 128, torch.bfloat16, True), "c4": (1, 32, 8192, 128, torch.float16, True),
        "d64": (2, 16, 4096, 64, torch.float16, False), "d64c": (2, 16, 4096, 64, torch.bfloat16, True)}      # (head dim 64: the compiler-scheduled dQ pass this change touches)


def rounds_of(fns, rounds, iters):
    """{name: [ms per call, one per round]} of the callables, timed round-robin."""
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(rounds):
        for n, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) / iters)
    return times


def eager_merge(outs, lses):
    L = torch.stack(lses)
    lse = torch.logsumexp(L, 0)
    w = torch.exp(L - lse)
    return (w.unsqueeze(-1) * torch.stack(outs).float()).sum(0).to(outs[0].dtype), lse


def bench_merge(rounds, iters, B=2, H=16, N=4096, D=128, dt=torch.bfloat16):
    dev = torch.device("cuda", 0)
    for n in (2, 4, 8):
        outs = [torch.randn((B, H, N, D), device=dev, dtype=dt) for _ in range(n)]
        lses = [torch.randn((B, H, N), device=dev) * 3.0 for _ in range(n)]
        do, dl = torch.randn((B, H, N, D), device=dev, dtype=dt), torch.randn((B, H, N), device=dev)
        go = [t.clone().requires_grad_(True) for t in outs]
        gl = [t.clone().requires_grad_(True) for t in lses]

        def fb(fn):
            def run():
                o, l = fn(go, gl)
                torch.autograd.backward([o, l], [do, dl])
                for t in go + gl:
                    t.grad = None
            return run
        with torch.no_grad():
            tf = rounds_of({"hip": lambda: merge_attention(outs, lses), "eager": lambda: eager_merge(outs, lses)}, rounds, iters)
        tb = rounds_of({"hip": fb(merge_attention), "eager": fb(eager_merge)}, rounds, iters)
        rows = B * H * N
        fwd_bytes = rows * (n * (2 * D + 4) + 2 * D + 4)
        bwd_bytes = rows * (n * (2 * D + 4) + 2 * D + 8 + n * (2 * D + 4))
        f_h, f_e = statistics.median(tf["hip"]), statistics.median(tf["eager"])
        b_h, b_e = statistics.median(tb["hip"]) - f_h, statistics.median(tb["eager"]) - f_e
        print("merge %d parts B%d H%d N%d D%d %s: fwd hip %7.1f us (%.2f TB/s, %.0f %% of %.1f) eager %7.1f us (%.1fx)   bwd (fwd+bwd minus fwd) hip %7.1f us "
              "(%.2f TB/s, %.0f %%) eager %7.1f us (%.1fx)" % (n, B, H, N, D, str(dt)[6:], f_h * 1e3, fwd_bytes / f_h / 1e9, 100 * fwd_bytes / f_h / 1e9 / PEAK_TBS,
                                                             PEAK_TBS, f_e * 1e3, f_e / f_h, b_h * 1e3, bwd_bytes / b_h / 1e9,
                                                             100 * bwd_bytes / b_h / 1e9 / PEAK_TBS, b_e * 1e3, b_e / b_h), flush=True)


def bench_merge_kernels(rounds, iters, B=2, H=16, N=4096, D=128, dt=torch.bfloat16):
    """The two kernels alone, straight through the C-ABI (pointer arrays built once, outputs allocated once): what the launches cost without the operator."""
    dev = torch.device("cuda", 0)
    lib = _fa2_lib.load()
    code = 0 if dt == torch.float16 else 1
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n in (2, 4, 8, 16):
        outs = [torch.randn((B, H, N, D), device=dev, dtype=dt) for _ in range(n)]
        lses = [torch.randn((B, H, N), device=dev) * 3.0 for _ in range(n)]
        do, dl = torch.randn((B, H, N, D), device=dev, dtype=dt), torch.randn((B, H, N), device=dev)
        o, l = torch.empty_like(outs[0]), torch.empty_like(lses[0])
        dos, dls = [torch.empty_like(t) for t in outs], [torch.empty_like(t) for t in lses]
        arr = lambda ts: (ctypes.c_void_p * n)(*(t.data_ptr() for t in ts))      # noqa: E731
        ao, al, ado, adl = arr(outs), arr(lses), arr(dos), arr(dls)
        s3, s2 = _s3(o), _fa2_lib.strides2(l.stride(0), l.stride(1))
        fl = _fa2_lib.FA2_MERGE_NATURAL_LSE
        fwd = lambda: _fa2_lib.check(lib.fa2_merge_fwd(code, n, ao, al, o.data_ptr(), l.data_ptr(), B, H, N, D, s3, s2, s3, s2, fl, st))      # noqa: E731
        bwd = lambda: _fa2_lib.check(lib.fa2_merge_bwd(code, n, ao, al, l.data_ptr(), do.data_ptr(), dl.data_ptr(), ado, adl, B, H, N, D, s3, s2, s2, s3, s2,      # noqa: E731
                                                       s3, s2, fl, st))
        fwd()
        tm = rounds_of({"fwd": fwd, "bwd": bwd}, rounds, iters)
        rows = B * H * N
        fwd_bytes = rows * (n * (2 * D + 4) + 2 * D + 4)
        bwd_bytes = rows * (n * (2 * D + 4) + 2 * D + 8 + n * (2 * D + 4))
        tf, tb = statistics.median(tm["fwd"]), statistics.median(tm["bwd"])
        print("merge kernels %2d parts B%d H%d N%d D%d %s: fwd %7.1f us  %6.1f MB  %.2f TB/s (%.0f %% of %.1f)   bwd %7.1f us  %6.1f MB  %.2f TB/s (%.0f %%)"
              % (n, B, H, N, D, str(dt)[6:], tf * 1e3, fwd_bytes / 1e6, fwd_bytes / tf / 1e9, 100 * fwd_bytes / tf / 1e9 / PEAK_TBS, PEAK_TBS,
                 tb * 1e3, bwd_bytes / 1e6, bwd_bytes / tb / 1e9, 100 * bwd_bytes / tb / 1e9 / PEAK_TBS), flush=True)


def _tensors(cfg):
    B, H, N, D, dt, causal = CFGS[cfg]
    dev = torch.device("cuda", 0)
    q, k, v, do = (torch.randn((B, H, N, D), device=dev, dtype=dt) for _ in range(4))
    o = torch.empty_like(q)
    lse = torch.empty((B, H, N), dtype=torch.float32, device=dev)
    return q, k, v, do, o, lse, torch.empty_like(lse), [torch.empty_like(q) for _ in range(3)]


def _s3(t):
    return _fa2_lib.strides3(t.stride(0), t.stride(1), t.stride(2))


def _fwd(lib, cfg, t, flags=0):
    B, H, N, D, dt, causal = CFGS[cfg]
    q, k, v, do, o, lse, delta, g = t
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _fa2_lib.check(lib.fa2_fwd(0 if dt == torch.float16 else 1, q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, N, N, D, _s3(q), _s3(k),
                               _s3(v), _s3(o), _fa2_lib.strides2(lse.stride(0), lse.stride(1)), float(D ** -0.5), int(causal) | flags, st))


def _bwd_args(cfg, t):
    B, H, N, D, dt, causal = CFGS[cfg]
    q, k, v, do, o, lse, delta, (dq, dk, dv) = t
    return (0 if dt == torch.float16 else 1, q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(),
            dv.data_ptr(), delta.data_ptr(), B, H, N, N, D, _s3(q), _s3(k), _s3(v), _s3(o), _s3(do), _s3(dq), _s3(dk), _s3(dv),
            _fa2_lib.strides2(lse.stride(0), lse.stride(1)), float(D ** -0.5), int(causal))


def bench_fallback(rounds, iters):
    lib = _fa2_lib.load()
    t = _tensors("c2")
    _fwd(lib, "c2", t, _fa2_lib.FA2_FLAG_EXACT_SCALE)
    args = _bwd_args("c2", t)
    dl = torch.zeros_like(t[5])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    tail = (None, 0, None, None, 0, st)
    s2 = _fa2_lib.strides2(dl.stride(0), dl.stride(1))
    tm = rounds_of({"no_dlse": lambda: _fa2_lib.check(lib.fa2_bwd_lse(*args, *tail, None, None)),
                    "dlse": lambda: _fa2_lib.check(lib.fa2_bwd_lse(*args, *tail, dl.data_ptr(), s2))}, rounds, iters)
    a, b = statistics.median(tm["no_dlse"]), statistics.median(tm["dlse"])
    print("fallback c2 backward (B2 H16 N4096 D128 fp16): without dlse (hand-scheduled) %.1f us, with dlse (compiler-scheduled) %.1f us, ratio %.3f"
          % (a * 1e3, b * 1e3, b / a), flush=True)


def bench_parent(path, rounds, iters):
    libs = {"this": _fa2_lib.load(), "parent": ctypes.CDLL(path)}
    for sym in ("fa2_fwd", "fa2_bwd"):
        fn = getattr(libs["parent"], sym)
        fn.restype, fn.argtypes = _fa2_lib.SYMBOLS[sym]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for cfg, what in (("c2", "bwd"), ("c3", "bwd"), ("c4", "bwd"), ("c2", "fwd"), ("d64", "bwd"), ("d64c", "bwd")):
        t = _tensors(cfg)
        _fwd(libs["this"], cfg, t)
        args = _bwd_args(cfg, t)
        if what == "bwd":
            fns = {n: (lambda lib=lib: _fa2_lib.check(lib.fa2_bwd(*args, st))) for n, lib in libs.items()}
        else:
            fns = {n: (lambda lib=lib: _fwd(lib, cfg, t)) for n, lib in libs.items()}
        tm = rounds_of(fns, rounds, iters)
        line = "parent %s %s:" % (cfg, what)
        for n in libs:
            line += "  %s median %.1f us (min %.1f .. max %.1f)" % (n, statistics.median(tm[n]) * 1e3, min(tm[n]) * 1e3, max(tm[n]) * 1e3)
        print(line + "  this/parent %.4f" % (statistics.median(tm["this"]) / statistics.median(tm["parent"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--parent", default="", help="another build of libfa2_gfx950.so to compare the existing calls with")
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    skip = set(a.skip.split(","))
    print(torch.cuda.get_device_name(0), "rounds", a.rounds, "iters", a.iters, flush=True)
    if "merge" not in skip:
        bench_merge_kernels(a.rounds, a.iters)
        bench_merge(a.rounds, a.iters)
    if "fallback" not in skip:
        bench_fallback(a.rounds, a.iters)
    if a.parent and "parent" not in skip:
        bench_parent(a.parent, a.rounds, a.iters)


if __name__ == "__main__":
    main()
