"""Sliding-window attention: timing of the windowed call against the dense band mask and the full causal call, same box, interleaved rounds,
median of per-round event times (tools/gqa_bench.py practice).

    python tools/window_bench.py [--rounds R] [--iters I] [--quick] [--decode]

Per row (bf16, B2, causal window of W keys ending at the query's own: window=(W - 1, 0), Nq = Nkv = N):
    (a) win   flash_attention(q, k, v, causal=True, window=(W - 1, 0))            the windowed kernels
    (b) mask  flash_attention(q, k, v, mask=band)                                  the only way without them: a bool [N, N] band, every KV tile swept
    (c) full  FlashAttentionFunction.apply(q, k, v, None, True)                    the full causal call (more work; hand-scheduled at D = 128)
    (d) hip   the same full causal call with option asm = 0 (the compiler-scheduled kernel of the head dim): the per-tile yardstick
`fwd` rows time the forward alone (no_grad), `fwd+bwd` rows one forward and one backward through autograd.
Derived columns: tiles = KV tiles a 256-row block visits, window / full causal (the work ratio the sweep should approach); a/b, a/c = time ratios;
frac = (c / a) / (tile ratio): the achieved share of the derived ratio; tile = time per visited tile of (a) over that of (d), against the
allowance (W + rows + tile) / W for the extra edge tile per block.
--decode: one query row against a KV cache (Nq = 1, q_offset = Nkv - 1), window 512 .. 4096, against the unwindowed decode call.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))

import torch  # noqa: E402

from rocwmma_fattn import _fa2_lib  # noqa: E402
from rocwmma_fattn.FlashAttn import FlashAttentionFunction, flash_attention  # noqa: E402

ROWS_PER_BLOCK, TILE = 256, 64


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


def visited_tiles(N, W):
    """KV tiles the 256-row blocks of one head visit: (windowed, full causal), from the library's own range function."""
    win = full = 0
    for row0 in range(0, N, ROWS_PER_BLOCK):
        win += _fa2_lib.window_tile_range(N, N, W - 1, 0, 0, True, row0, ROWS_PER_BLOCK, TILE)[1]
        full += _fa2_lib.window_tile_range(N, N, -1, 0, 0, True, row0, ROWS_PER_BLOCK, TILE)[1]
    return win, full


def with_asm_off(fn):
    def run():
        with _fa2_lib.options(asm=0):
            fn()
    return run


def row(B, H, Hkv, N, D, W, rounds, iters, bwd):
    dev, dt = torch.device("cuda", 0), torch.bfloat16
    q = torch.randn((B, H, N, D), device=dev, dtype=dt)
    k, v = (torch.randn((B, Hkv, N, D), device=dev, dtype=dt) for _ in range(2))
    do = torch.randn_like(q)
    i = torch.arange(N, device=dev)
    band = (i[None, :] <= i[:, None]) & (i[None, :] >= i[:, None] - (W - 1))       # bool [N, N], broadcast over B and H
    out = []
    fwd = {
        "win": lambda: flash_attention(q, k, v, causal=True, window=(W - 1, 0)),
        "mask": lambda: flash_attention(q, k, v, mask=band),
        "full": lambda: FlashAttentionFunction.apply(q, k, v, None, True),
        "hip": with_asm_off(lambda: FlashAttentionFunction.apply(q, k, v, None, True)),
    }
    with torch.no_grad():
        out.append(("fwd", interleaved(fwd, rounds, iters)))
    if bwd:
        qg, kg, vg = (x.clone().requires_grad_(True) for x in (q, k, v))
        fb = {
            "win": lambda: flash_attention(qg, kg, vg, causal=True, window=(W - 1, 0)).backward(do),
            "mask": lambda: flash_attention(qg, kg, vg, mask=band).backward(do),
            "full": lambda: FlashAttentionFunction.apply(qg, kg, vg, None, True).backward(do),
            "hip": with_asm_off(lambda: FlashAttentionFunction.apply(qg, kg, vg, None, True).backward(do)),
        }
        out.append(("fwd+bwd", interleaved(fb, rounds, max(1, iters // 2))))
    return out


def decode(rounds, iters):
    dev, dt = torch.device("cuda", 0), torch.bfloat16
    for H, Hkv, Nkv, D in ((32, 8, 8192, 128), (32, 8, 32768, 128), (16, 16, 8192, 64)):
        q = torch.randn((1, H, 1, D), device=dev, dtype=dt)
        k, v = (torch.randn((1, Hkv, Nkv, D), device=dev, dtype=dt) for _ in range(2))
        fns = {"all keys": lambda: FlashAttentionFunction.apply(q, k, v, None, False)}
        for W in (512, 1024, 4096):
            fns["W%d" % W] = (lambda W=W: flash_attention(q, k, v, window=(W - 1, 0), q_offset=Nkv - 1))
        with torch.no_grad():
            t = interleaved(fns, rounds, iters)
        print("decode H%d/Hkv%d Nkv%d D%d  " % (H, Hkv, Nkv, D) + "  ".join("%s %.1f us" % (n, ms * 1e3) for n, ms in t.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="H16 only, N 4096 and 8192, no N = 16384 mask rows")
    ap.add_argument("--decode", action="store_true", help="only the decode rows")
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0), "rounds", a.rounds, "iters", a.iters, "bf16 B2, causal window of W keys")
    if a.decode:
        return decode(a.rounds, a.iters)
    heads = ((16, 16),) if a.quick else ((16, 16), (32, 8))
    for D in (64, 128):
        for H, Hkv in heads:
            for N in ((4096, 8192) if a.quick else (4096, 8192, 16384)):
                for W in (256, 1024, 4096):
                    if W >= N:
                        continue
                    tw, tf = visited_tiles(N, W)
                    for what, t in row(2, H, Hkv, N, D, W, a.rounds, a.iters, True):
                        ratio = tf / tw
                        per_tile = (t["win"] / tw) / (t["hip"] / tf)
                        print("D%-3d H%d/%d N%-5d W%-4d %-7s tiles %5d/%5d (%.2fx)  " % (D, H, Hkv, N, W, what, tw, tf, ratio) +
                              "  ".join("%s %8.1f us" % (n, ms * 1e3) for n, ms in t.items()) +
                              "  a/b %.3f  a/c %.3f  frac %.2f  tile %.2f (allow %.2f)" % (t["win"] / t["mask"], t["win"] / t["full"], (t["full"] / t["win"]) / ratio,
                                                                                         per_tile, (W + ROWS_PER_BLOCK + TILE) / W), flush=True)
    decode(a.rounds, a.iters)


if __name__ == "__main__":
    main()
