"""Packed (variable-length) attention: timing of flash_attention_varlen against what a caller had before it — the padded batch under a key-padding
mask, and a Python loop over the sequences — same box, interleaved rounds, median of per-round event times (tools/window_bench.py practice).

    python tools/varlen_bench.py [--rounds R] [--iters I] [--quick] [--dims 128,64] [--sets doc,ramp,near,uniform]

Per row (bf16; H16, and H32 with 8 K / V heads; D 128 and 64; causal and not; self-attention, Nq_s = Nkv_s):
    (a)  varlen  flash_attention_varlen(q, k, v, cu, cu, max, max)                  the packed kernels: sum(len^2) scores
    (b)  pad     flash_attention(qp, kp, vp, mask=key padding [B, 1, 1, max])        every sequence padded to the longest: B * max^2 scores through the
                                                                                    masked kernels, grouped K / V expanded
    (b') nomask  FlashAttentionFunction.apply(qp, kp, vp, None, causal)              the padded batch with NO mask on the default kernels: its answer is wrong
                                                                                    for padded keys — the fastest a padding approach could be
    (c)  loop    one FlashAttentionFunction.apply per sequence                       B launches (2 - 3 more each in the backward) on small grids
    (d)  bnhd    uniform lengths only: the batched [B, N, H, D] call on the same memory with option asm = 0 (the compiler-scheduled kernels): the per-tile
                 yardstick — (a) visits the same tiles there, so a/d is the time per visited tile of (a) over (d)
`fwd` rows time the forward alone (no_grad), `fwd+bwd` rows one forward and one backward through autograd.
ratio = B * max^2 / sum(len^2), from the lengths themselves: the work the padded batch does over the work there is.
Length sets: doc 8192 .. 128 (ratio 6.0), ramp 256 .. 4096 in steps of 256 (2.74), near 8 lengths in 3584 .. 4096 (~1.15), uniform 8 x 4096 (1).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))

import torch  # noqa: E402

from rocwmma_fattn import _fa2_lib  # noqa: E402
from rocwmma_fattn.FlashAttn import FlashAttentionFunction, flash_attention, flash_attention_varlen  # noqa: E402

LENGTH_SETS = {
    "doc": [8192, 4096, 2048, 1024, 512, 256, 128, 128],
    "ramp": [256 * i for i in range(1, 17)],
    "near": [4096, 3584, 3968, 3712, 4032, 3840, 3648, 3904],
    "uniform": [4096] * 8,
}


def interleaved(fns, rounds, iters):
    """{name: median ms per call} of the callables in `fns`, timed round-robin (one event pair per (round, callable))."""
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
    return {n: statistics.median(t) for n, t in times.items()}


def with_asm_off(fn):
    def run():
        with _fa2_lib.options(asm=0):
            fn()
    return run


def row(lens, H, Hkv, D, causal, rounds, iters):
    dev, dt = torch.device("cuda", 0), torch.bfloat16
    B, mx, total = len(lens), max(lens), sum(lens)
    cu = torch.tensor([0] + [sum(lens[:i + 1]) for i in range(B)], dtype=torch.int32, device=dev)
    q = torch.randn((total, H, D), device=dev, dtype=dt)
    k, v = (torch.randn((total, Hkv, D), device=dev, dtype=dt) for _ in range(2))
    do = torch.randn_like(q)
    # the padded batch, [B, max, heads, D] (BNHD), and its key-padding mask
    qp, dop = (torch.zeros((B, mx, H, D), device=dev, dtype=dt) for _ in range(2))
    kp, vp = (torch.zeros((B, mx, Hkv, D), device=dev, dtype=dt) for _ in range(2))
    for s, n in enumerate(lens):
        a = int(cu[s])
        qp[s, :n], dop[s, :n], kp[s, :n], vp[s, :n] = q[a:a + n], do[a:a + n], k[a:a + n], v[a:a + n]
    pad_mask = (torch.arange(mx, device=dev)[None, :] < torch.tensor(lens, device=dev)[:, None]).view(B, 1, 1, mx)
    bounds = [(int(cu[s]), int(cu[s + 1])) for s in range(B)]
    uniform = len(set(lens)) == 1

    def make(q, k, v, qp, kp, vp, back):
        def done(o, g):
            if back:
                o.backward(g)

        def loop():
            for a, b in bounds:
                done(FlashAttentionFunction.apply(q[a:b].unsqueeze(0), k[a:b].unsqueeze(0), v[a:b].unsqueeze(0), None, causal, None, True), do[a:b].unsqueeze(0))
        fns = {
            "varlen": lambda: done(flash_attention_varlen(q, k, v, cu, cu, mx, mx, causal=causal), do),
            "pad": lambda: done(flash_attention(qp, kp, vp, mask=pad_mask, causal=causal, BNHD_fmt=True), dop),
            "nomask": lambda: done(FlashAttentionFunction.apply(qp, kp, vp, None, causal, None, True), dop),
            "loop": loop,
        }
        if uniform:
            fns["bnhd"] = with_asm_off(lambda: done(FlashAttentionFunction.apply(q.view(B, mx, H, D), k.view(B, mx, Hkv, D), v.view(B, mx, Hkv, D), None, causal,
                                                                                 None, True), do.view(B, mx, H, D)))
        return fns
    out = []
    with torch.no_grad():
        out.append(("fwd", interleaved(make(q, k, v, qp, kp, vp, False), rounds, iters)))
    grads = [x.clone().requires_grad_(True) for x in (q, k, v, qp, kp, vp)]
    out.append(("fwd+bwd", interleaved(make(*grads, True), rounds, max(1, iters // 2))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="H16 only")
    ap.add_argument("--dims", default="128,64")
    ap.add_argument("--sets", default="doc,ramp,near,uniform")
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0), "rounds", a.rounds, "iters", a.iters, "bf16, self-attention, times in us", flush=True)
    heads = ((16, 16),) if a.quick else ((16, 16), (32, 8))
    for D in (int(x) for x in a.dims.split(",")):
        for H, Hkv in heads:
            for name in a.sets.split(","):
                lens = LENGTH_SETS[name]
                ratio = len(lens) * max(lens) ** 2 / sum(n * n for n in lens)
                for causal in (False, True):
                    for what, t in row(lens, H, Hkv, D, causal, a.rounds, a.iters):
                        line = "D%-3d H%d/%d %-7s %-6s %-7s ratio %.2f  " % (D, H, Hkv, name, "causal" if causal else "full", what, ratio)
                        line += "  ".join("%s %9.1f" % (n, ms * 1e3) for n, ms in t.items())
                        line += "  a/b %.3f  a/b' %.3f  a/c %.3f" % (t["varlen"] / t["pad"], t["varlen"] / t["nomask"], t["varlen"] / t["loop"])
                        if "bnhd" in t:
                            line += "  a/d (per visited tile) %.3f" % (t["varlen"] / t["bnhd"])
                        conds = []
                        if ratio >= 2:
                            conds.append("a<b %s" % ("ok" if t["varlen"] < t["pad"] else "MISSED"))
                        if ratio >= 4:
                            conds.append("a<b' %s" % ("ok" if t["varlen"] < t["nomask"] else "MISSED"))
                        print(line + ("  [" + ", ".join(conds) + "]" if conds else ""), flush=True)


if __name__ == "__main__":
    main()
