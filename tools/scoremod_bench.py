"""Score modifiers: what logit soft-capping and ALiBi slopes cost in-kernel — same box, interleaved rounds, median of per-round event times
(tools/varlen_bench.py practice).

    python tools/scoremod_bench.py [--rounds R] [--iters I] [--softcap 30] [--quick]

Dense rows (B2 H16 N4096 D128: bf16 causal, fp16 full; --quick: the first only), forward alone (no_grad) and forward + backward through autograd:
    (a1) cap     flash_attention(q, k, v, causal, window=W, softcap=c)                     the FA2_SMOD kernels, soft-capping alone
    (a2) alibi   flash_attention(q, k, v, causal, window=W, alibi_slopes=s)                ... ALiBi alone
    (a3) both    flash_attention(q, k, v, causal, window=W, softcap=c, alibi_slopes=s)     ... both
    (b)  window  flash_attention(q, k, v, causal, window=W)                                the same kernel family without them: the windowed kernels
    (c)  plain   flash_attention(q, k, v, causal)                                          the default call (hand-scheduled kernels where they exist)
    (d)  bias    flash_attention(q, k, v, mask=the ALiBi bias [H, N, N] (+ the causal band))  what an ALiBi caller had before (forward + backward only to D 256)
W is the widest window that is not full — it masks ONE score of the whole matrix ((N, N - 2) full, (N - 2, 0) causal) — because a window that masks
nothing is handed to the default kernels by fa2_fwd_window, and (b) has to be the twin of (a): same tiles, same launch shapes, no transform.
The cost of the feature is a/b.
Packed row (the `doc` lengths of tools/varlen_bench.py, H16 D128 bf16 causal): (a3) flash_attention_varlen(softcap=c, alibi_slopes=s), (b) the same call without.
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

ORDER = ("cap", "alibi", "both", "window", "plain", "bias")


def slopes_of(H, dev):
    return torch.tensor([2.0 ** (-8.0 * (h + 1) / H) for h in range(H)], dtype=torch.float32, device=dev)


def show(tag, what, t):
    line = "%-44s %-7s " % (tag, what) + "  ".join("%s %9.1f" % (n, t[n] * 1e3) for n in ORDER if n in t)
    line += "  a/b " + " ".join("%s %.3f" % (n, t[n] / t["window"]) for n in ("cap", "alibi", "both") if n in t)
    if "bias" in t and "alibi" in t:
        line += "  alibi/bias %.3f" % (t["alibi"] / t["bias"])
    print(line, flush=True)


def dense(dt, causal, cap, rounds, iters, B=2, H=16, N=4096, D=128):
    dev = torch.device("cuda", 0)
    q, k, v, do = (torch.randn((B, H, N, D), device=dev, dtype=dt) for _ in range(4))
    W = (N - 2, 0) if causal else (N, N - 2)
    sl = slopes_of(H, dev)
    i = torch.arange(N, device=dev)
    bias = (-sl[:, None, None] * (i[:, None] - i[None, :]).abs()).to(dt)            # [H, N, N]: the tensor the keyword spares
    if causal:
        bias = bias.masked_fill(i[None, :] > i[:, None], float("-inf"))

    def make(q, k, v, back):
        def done(o):
            if back:
                o.backward(do)
        return {
            "cap": lambda: done(flash_attention(q, k, v, causal=causal, window=W, softcap=cap)),
            "alibi": lambda: done(flash_attention(q, k, v, causal=causal, window=W, alibi_slopes=sl)),
            "both": lambda: done(flash_attention(q, k, v, causal=causal, window=W, softcap=cap, alibi_slopes=sl)),
            "window": lambda: done(flash_attention(q, k, v, causal=causal, window=W)),
            "plain": lambda: done(flash_attention(q, k, v, causal=causal)),
            "bias": lambda: done(flash_attention(q, k, v, mask=bias)),
        }
    tag = "dense B%d H%d N%d D%d %s %s cap=%g" % (B, H, N, D, str(dt)[6:], "causal" if causal else "full", cap)
    with torch.no_grad():
        show(tag, "fwd", interleaved(make(q, k, v, False), rounds, iters))
    g = [x.clone().requires_grad_(True) for x in (q, k, v)]
    show(tag, "fwd+bwd", interleaved(make(*g, True), rounds, max(1, iters // 2)))


def packed(cap, rounds, iters, H=16, D=128):
    dev, dt, lens = torch.device("cuda", 0), torch.bfloat16, LENGTH_SETS["doc"]
    total, mx = sum(lens), max(lens)
    cu = torch.tensor([0] + [sum(lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32, device=dev)
    q, k, v, do = (torch.randn((total, H, D), device=dev, dtype=dt) for _ in range(4))
    sl = slopes_of(H, dev)

    def make(q, k, v, back):
        def done(o):
            if back:
                o.backward(do)
        return {"both": lambda: done(flash_attention_varlen(q, k, v, cu, cu, mx, mx, causal=True, softcap=cap, alibi_slopes=sl)),
                "window": lambda: done(flash_attention_varlen(q, k, v, cu, cu, mx, mx, causal=True))}
    tag = "packed doc H%d D%d bf16 causal cap=%g" % (H, D, cap)
    with torch.no_grad():
        show(tag, "fwd", interleaved(make(q, k, v, False), rounds, iters))
    g = [x.clone().requires_grad_(True) for x in (q, k, v)]
    show(tag, "fwd+bwd", interleaved(make(*g, True), rounds, max(1, iters // 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--softcap", type=float, default=30.0)
    ap.add_argument("--quick", action="store_true", help="the bf16 causal dense row only")
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0), "rounds", a.rounds, "iters", a.iters,
          "times in us; cap / alibi / both = (a1) / (a2) / (a3), window = (b), plain = (c), bias = (d)", flush=True)
    dense(torch.bfloat16, True, a.softcap, a.rounds, a.iters)
    if not a.quick:
        dense(torch.float16, False, a.softcap, a.rounds, a.iters)
        packed(a.softcap, a.rounds, a.iters)


if __name__ == "__main__":
    main()
