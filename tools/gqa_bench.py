"""Grouped-query attention: timing of the grouped call against the repeat_interleave workaround and torch SDPA (enable_gqa=True), same box,
interleaved rounds, median of per-round event times (tools/kbench.py practice).

    python tools/gqa_bench.py [--rounds R] [--iters I] [--ab PARENT.so]

Per row:  (a) the grouped call (FlashAttentionFunction.apply with k / v of Hkv heads);
          (b) this library's MHA call on K / V expanded to H heads: `mha` with the expanded tensors prepared outside the timed region, `mha+exp`
              with repeat_interleave (and, in the backward, the sum of dK / dV over each group that autograd does through it) inside;
          (c) torch.nn.functional.scaled_dot_product_attention(..., enable_gqa=True).
`fwd+bwd` rows time one forward and one backward through autograd.  The D = 128 backward is also timed pass by pass through the C-ABI
(option "bwd_parts": the dQ pass, then the dK / dV pass alone) for the grouped call and for the MHA call on expanded K / V.
--ab PARENT.so: the MHA forward of c2 / c3 / c4 and the c2 backward, this library against another build of it (C-ABI, interleaved).
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from rocwmma_fattn import _fa2_lib  # noqa: E402
from rocwmma_fattn.FlashAttn import FlashAttentionFunction  # noqa: E402

ROWS = [  # (label, B, H, Hkv, Nq, Nkv, D, dtype, causal, with backward)
    ("llama8b_bf16_c", 1, 32, 8, 4096, 4096, 128, torch.bfloat16, True, True),
    ("llama8b_f16_nc", 1, 32, 8, 4096, 4096, 128, torch.float16, False, True),
    ("d64_bf16_c", 2, 16, 4, 4096, 4096, 64, torch.bfloat16, True, True),
    ("mqa_bf16_c", 1, 32, 1, 4096, 4096, 128, torch.bfloat16, True, True),
    ("decode_hkv8", 1, 32, 8, 1, 8192, 128, torch.float16, False, False),
    ("decode_hkv4", 1, 32, 4, 1, 8192, 128, torch.float16, False, False),
    ("decode_hkv1", 1, 32, 1, 1, 8192, 128, torch.float16, False, False),
]


def interleaved(fns, rounds, iters):
    """{name: median ms per call} of the callables in `fns`, timed round-robin (one event pair per (round, callable))."""
    for f in fns.values():
        for _ in range(3):
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
    return {n: statistics.median(t) for n, t in times.items()}


def row(label, B, H, Hkv, Nq, Nkv, D, dt, causal, bwd, rounds, iters):
    dev = torch.device("cuda", 0)
    g = H // Hkv
    q = torch.randn((B, H, Nq, D), device=dev, dtype=dt)
    k = torch.randn((B, Hkv, Nkv, D), device=dev, dtype=dt)
    v = torch.randn((B, Hkv, Nkv, D), device=dev, dtype=dt)
    ke, ve = k.repeat_interleave(g, 1).contiguous(), v.repeat_interleave(g, 1).contiguous()
    do = torch.randn_like(q)
    out = []
    fwd = {
        "gqa": lambda: FlashAttentionFunction.apply(q, k, v, None, causal),
        "mha": lambda: FlashAttentionFunction.apply(q, ke, ve, None, causal),
        "mha+exp": lambda: FlashAttentionFunction.apply(q, k.repeat_interleave(g, 1), v.repeat_interleave(g, 1), None, causal),
        "sdpa": lambda: F.scaled_dot_product_attention(q, k, v, is_causal=causal, enable_gqa=True),
    }
    with torch.no_grad():
        t = interleaved(fwd, rounds, iters)
    out.append((label, "fwd", t))
    if bwd:
        qg, kg, vg = (x.clone().requires_grad_(True) for x in (q, k, v))
        kge, vge = ke.clone().requires_grad_(True), ve.clone().requires_grad_(True)

        def step(fn):
            def run():
                fn().backward(do)
            return run
        fb = {
            "gqa": step(lambda: FlashAttentionFunction.apply(qg, kg, vg, None, causal)),
            "mha": step(lambda: FlashAttentionFunction.apply(qg, kge, vge, None, causal)),
            "mha+exp": step(lambda: FlashAttentionFunction.apply(qg, kg.repeat_interleave(g, 1), vg.repeat_interleave(g, 1), None, causal)),
            "sdpa": step(lambda: F.scaled_dot_product_attention(qg, kg, vg, is_causal=causal, enable_gqa=True)),
        }
        out.append((label, "fwd+bwd", interleaved(fb, rounds, max(1, iters // 2))))
        if D == 128:
            out.append((label, "bwd passes", bwd_passes(q, k, v, ke, ve, do, H, Hkv, causal, rounds, iters)))
    return out


def bwd_passes(q, k, v, ke, ve, do, H, Hkv, causal, rounds, iters):
    """Backward through the C-ABI, pass by pass (option bwd_parts 1: the dQ pass, 2: the dK / dV pass on the delta an earlier full call left)."""
    lib = _fa2_lib.load()
    B, _, Nq, D = q.shape
    Nkv = k.shape[2]
    dt = _fa2_lib.FA2_DTYPE_F16 if q.dtype == torch.float16 else _fa2_lib.FA2_DTYPE_BF16
    s3 = lambda t: _fa2_lib.strides3(t.stride(0), t.stride(1), t.stride(2))  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = torch.empty_like(q)
    lse = torch.empty((B, H, Nq), device=q.device, dtype=torch.float32)
    s2 = _fa2_lib.strides2(H * Nq, Nq)
    _fa2_lib.check(lib.fa2_fwd(dt, q.data_ptr(), ke.data_ptr(), ve.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, Nq, Nkv, D, s3(q), s3(ke), s3(ve),
                               s3(o), s2, D ** -0.5, int(causal) | _fa2_lib.FA2_FLAG_EXACT_SCALE, None))
    dq, delta_g, delta_m = torch.empty_like(q), torch.empty_like(lse), torch.empty_like(lse)     # (one delta each: its sign depends on the dQ pass)
    dkg, dvg, dke, dve = torch.empty_like(k), torch.empty_like(v), torch.empty_like(ke), torch.empty_like(ve)
    common = lambda kk, vv, dk, dv: (q.data_ptr(), kk.data_ptr(), vv.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(),  # noqa: E731
                                     dk.data_ptr(), dv.data_ptr(), (delta_g if kk is k else delta_m).data_ptr())
    st = lambda kk, vv, dk, dv: (s3(q), s3(kk), s3(vv), s3(o), s3(do), s3(dq), s3(dk), s3(dv), s2)  # noqa: E731
    fns = {
        "gqa": lambda: _fa2_lib.check(lib.fa2_bwd_gqa(dt, *common(k, v, dkg, dvg), B, H, Hkv, Nq, Nkv, D, *st(k, v, dkg, dvg), D ** -0.5, int(causal),
                                                      None, 0, stream)),
        "mha": lambda: _fa2_lib.check(lib.fa2_bwd(dt, *common(ke, ve, dke, dve), B, H, Nq, Nkv, D, *st(ke, ve, dke, dve), D ** -0.5, int(causal), stream)),
    }
    res = {}
    for parts, tag in ((3, "whole"), (1, "dQ"), (2, "dKdV")):
        for f in fns.values():
            f()                      # (a full call first: the dK / dV pass alone reads the delta it left)
        with _fa2_lib.options(bwd_parts=parts):
            t = interleaved(fns, rounds, iters)
        for n, ms in t.items():
            res["%s %s" % (n, tag)] = ms
    return res


def ab(parent, rounds, iters):
    """MHA calls: this library against another build (C-ABI, interleaved): c2 / c3 / c4 forward, c2 backward."""
    i64p = ctypes.POINTER(ctypes.c_int64)
    libs = {"this": ctypes.CDLL(_fa2_lib.LIB_PATH), "parent": ctypes.CDLL(parent)}
    for lib in libs.values():
        lib.fa2_fwd.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 5 + [i64p] * 5 + [ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
        lib.fa2_bwd.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 10 + [ctypes.c_int] * 5 + [i64p] * 9 + [ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    dev = torch.device("cuda", 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    s3 = lambda t: _fa2_lib.strides3(t.stride(0), t.stride(1), t.stride(2))  # noqa: E731
    out = []
    for name, (B, H, N, D, dt, causal, bwd) in (("c2 fwd", (2, 16, 4096, 128, torch.float16, False, False)),
                                                ("c3 fwd", (2, 16, 4096, 128, torch.bfloat16, True, False)),
                                                ("c4 fwd", (1, 32, 8192, 128, torch.float16, True, False)),
                                                ("c2 bwd", (2, 16, 4096, 128, torch.float16, False, True))):
        q, k, v, do = (torch.rand((B, H, N, D), device=dev).to(dt) for _ in range(4))
        o, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
        lse, delta = (torch.empty((B, H, N), device=dev, dtype=torch.float32) for _ in range(2))
        code = 0 if dt == torch.float16 else 1
        s2 = _fa2_lib.strides2(H * N, N)

        def mk(lib):
            if not bwd:
                return lambda: lib.fa2_fwd(code, q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, N, N, D, s3(q), s3(k),
                                           s3(v), s3(o), s2, D ** -0.5, int(causal), stream)
            return lambda: lib.fa2_bwd(code, q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                                       dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), B, H, N, N, D, s3(q), s3(k), s3(v), s3(o), s3(do), s3(dq), s3(dk),
                                       s3(dv), s2, D ** -0.5, int(causal), stream)
        if bwd:
            libs["this"].fa2_fwd(code, q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, N, N, D, s3(q), s3(k), s3(v),
                                 s3(o), s2, D ** -0.5, int(causal) | 2, stream)
        out.append(("mha A/B", name, interleaved({n: mk(lib) for n, lib in libs.items()}, rounds, iters)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--ab", default=None, help="another build of libfa2_gfx950.so: MHA A/B of c2 / c3 / c4 forward and c2 backward")
    ap.add_argument("--ab-only", action="store_true", help="only the MHA A/B of --ab")
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0), "rounds", a.rounds, "iters", a.iters)
    results = []
    for r in ROWS if not a.ab_only else []:
        results += row(*r, a.rounds, a.iters)
    if a.ab:
        results += ab(a.ab, a.rounds, a.iters)
    for label, what, t in results:
        base = t.get("mha")
        print("%-16s %-10s " % (label, what) + "  ".join("%s %8.1f us%s" % (n, ms * 1e3, " (%.3fx mha)" % (ms / base) if base and n != "mha" else "")
                                                         for n, ms in t.items()))


if __name__ == "__main__":
    main()
