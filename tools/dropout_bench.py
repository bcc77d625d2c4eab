"""Attention dropout: what the in-kernel Philox mask costs — same box, interleaved rounds, median of per-round event times (tools/varlen_bench.py practice).

    python tools/dropout_bench.py [--rounds R] [--iters I] [--p 0.1] [--quick]

Dense rows (B2 H16 N4096 D128: bf16 causal, fp16 full; --quick: the first only), forward alone (no_grad) and forward + backward through autograd:
    (a)  drop    flash_attention(q, k, v, causal, window=W, dropout_p=p)           the FA2_DROP kernels
    (b)  window  flash_attention(q, k, v, causal, window=W)                        the same kernel family without dropout: the windowed kernels
    (c)  plain   flash_attention(q, k, v, causal)                                  the default call (hand-scheduled kernels where they exist)
    (d)  sdpa    torch.nn.functional.scaled_dot_product_attention(dropout_p=p)     what a caller had before
W is the widest window that is not full — it masks ONE score of the whole matrix ((N, N - 2) full, (N - 2, 0) causal) — because a window that masks
nothing is handed to the default kernels by fa2_fwd_window, and (b) has to be the twin of (a): same tiles, same launch shapes, no dropout.
The cost of dropout is a/b.
Packed row (the `doc` lengths of tools/varlen_bench.py, H16 D128 bf16 causal): (a) flash_attention_varlen(dropout_p=p), (b) the same call without.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from rocwmma_fattn.FlashAttn import flash_attention, flash_attention_varlen  # noqa: E402
from varlen_bench import LENGTH_SETS, interleaved  # noqa: E402


def show(tag, what, t, names):
    line = "%-44s %-7s " % (tag, what) + "  ".join("%s %9.1f" % (n, t[n] * 1e3) for n in names if n in t)
    line += "  a/b %.3f" % (t["drop"] / t["window"])
    if "plain" in t:
        line += "  a/c %.3f" % (t["drop"] / t["plain"])
    if "sdpa" in t:
        line += "  a/d %.3f" % (t["drop"] / t["sdpa"])
    print(line, flush=True)


def dense(dt, causal, p, rounds, iters, B=2, H=16, N=4096, D=128):
    dev = torch.device("cuda", 0)
    q, k, v, do = (torch.randn((B, H, N, D), device=dev, dtype=dt) for _ in range(4))
    W = (N - 2, 0) if causal else (N, N - 2)
    seed = [1]

    def make(q, k, v, back):
        def done(o):
            if back:
                o.backward(do)

        def drop():
            seed[0] += 1                         # a new mask per call, as in training
            done(flash_attention(q, k, v, causal=causal, window=W, dropout_p=p, dropout_seed=seed[0]))
        fns = {
            "drop": drop,
            "window": lambda: done(flash_attention(q, k, v, causal=causal, window=W)),
            "plain": lambda: done(flash_attention(q, k, v, causal=causal)),
            "sdpa": lambda: done(torch.nn.functional.scaled_dot_product_attention(q, k, v, dropout_p=p, is_causal=causal)),
        }
        try:
            fns["sdpa"]()
            torch.cuda.synchronize()
        except Exception as e:   # noqa: BLE001 - a torch build without a fused dropout path for this shape
            print("  (sdpa not timed: %s)" % str(e)[:120])
            del fns["sdpa"]
        return fns
    tag = "dense B%d H%d N%d D%d %s %s p=%g" % (B, H, N, D, str(dt)[6:], "causal" if causal else "full", p)
    with torch.no_grad():
        show(tag, "fwd", interleaved(make(q, k, v, False), rounds, iters), ("drop", "window", "plain", "sdpa"))
    g = [x.clone().requires_grad_(True) for x in (q, k, v)]
    show(tag, "fwd+bwd", interleaved(make(*g, True), rounds, max(1, iters // 2)), ("drop", "window", "plain", "sdpa"))


def packed(p, rounds, iters, H=16, D=128):
    dev, dt, lens = torch.device("cuda", 0), torch.bfloat16, LENGTH_SETS["doc"]
    total, mx = sum(lens), max(lens)
    cu = torch.tensor([0] + [sum(lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32, device=dev)
    q, k, v, do = (torch.randn((total, H, D), device=dev, dtype=dt) for _ in range(4))
    seed = [1]

    def make(q, k, v, back):
        def done(o):
            if back:
                o.backward(do)

        def drop():
            seed[0] += 1
            done(flash_attention_varlen(q, k, v, cu, cu, mx, mx, causal=True, dropout_p=p, dropout_seed=seed[0]))
        return {"drop": drop, "window": lambda: done(flash_attention_varlen(q, k, v, cu, cu, mx, mx, causal=True))}
    tag = "packed doc H%d D%d bf16 causal p=%g" % (H, D, p)
    with torch.no_grad():
        show(tag, "fwd", interleaved(make(q, k, v, False), rounds, iters), ("drop", "window"))
    g = [x.clone().requires_grad_(True) for x in (q, k, v)]
    show(tag, "fwd+bwd", interleaved(make(*g, True), rounds, max(1, iters // 2)), ("drop", "window"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--quick", action="store_true", help="the bf16 causal dense row only")
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0), "rounds", a.rounds, "iters", a.iters, "times in us; drop = (a), window = (b), plain = (c), sdpa = (d)", flush=True)
    dense(torch.bfloat16, True, a.p, a.rounds, a.iters)
    if not a.quick:
        dense(torch.float16, False, a.p, a.rounds, a.iters)
        packed(a.p, a.rounds, a.iters)


if __name__ == "__main__":
    main()
