"""The non-absorbed MLA prefill — packed, causal attention with q / k 192 wide and v 128 wide — through flash_attention_varlen's Dv route
(fa2_fwd_varlen_dv) against what a user had before it, same process, interleaved rounds, median of per-round event times with the spread of the rounds
beside it (tools/mla_append_bench.py's protocol: 9 rounds of 20 calls, spread = (max - min) / median; a gap counts only beyond the sum of the two
spreads).  bf16, D 192 / Dv 128.

    python tools/mla_prefill_bench.py [--rounds R] [--iters I] [--rows prefill|chunk|all]

Columns of a row:
    dv          flash_attention_varlen(q, k, v [total_k, H, 128]): one 128-column slab, 12 Q.K^T k-steps
    pad_out     the route before, V zero-padded to 192 OUTSIDE the timed region: flash_attention_varlen on the padded V, O sliced to 128 columns
                (the packed kernel of head dim 256: two 128-column slabs of 16 k-steps each)
    pad_in      the same with the pad (torch.nn.functional.pad of V) inside the timed region: what a serving loop that gets V from the up-projection pays
    dv_r128, dv_r256   dv under option "rows" = 128 / 256 (dv itself runs the plan's choice, printed first)
dv is first checked against pad_out on the timed inputs: the two must agree bit for bit.  TFLOPS count the real columns: 2 * (192 + 128) FLOPs per
visible (query, key) pair.
Prefill rows: B4 x 4096 tokens at H128 and H16, B1 x 16384 at H128 and H16, the eight packed documents 8192 .. 128 (16384 tokens) at H16; all causal.
Chunk row (a chunked-context / prefix-hit step): 2048 new tokens on 8192 up-projected context keys — the new queries against the context keys
(non-causal), against the new keys (causal), and merge_attention of the two; the padded route merges the sliced outputs."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))

import torch  # noqa: E402

from benchlib import interleaved  # noqa: E402
from rocwmma_fattn import _fa2_lib  # noqa: E402
from rocwmma_fattn.FlashAttn import flash_attention_varlen, merge_attention  # noqa: E402

D, DV = 192, 128
DOCS = [8192, 4096, 2048, 1024, 512, 256, 128, 128]
PREFILL_ROWS = [  # (label, H, lengths)
    ("b4_4k_h128", 128, [4096] * 4),
    ("b4_4k_h16", 16, [4096] * 4),
    ("b1_16k_h128", 128, [16384]),
    ("b1_16k_h16", 16, [16384]),
    ("docs_h16", 16, DOCS),
]
CHUNK_ROWS = [("chunk_h128", 128, 8192, 2048), ("chunk_h16", 16, 8192, 2048)]      # (label, H, context keys, new tokens)


def cu_of(lens, dev):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return torch.tensor(out, dtype=torch.int32, device=dev)


def line(name, t, flops, base=None):
    med, lo, hi = t[name]
    rel = ""
    if base is not None and name != base:
        b_med, b_lo, b_hi = t[base]
        real = abs(b_med - med) > (hi - lo) + (b_hi - b_lo)          # the project's rule: a difference beyond the sum of the two spreads
        rel = "  %+.1f us against %s, %.2fx %s (%s the sum of the spreads, %.1f us)" % ((med - b_med) * 1e3, base, max(b_med / med, med / b_med),
                                                                                       "faster" if med <= b_med else "slower", "beyond" if real else "WITHIN",
                                                                                       ((hi - lo) + (b_hi - b_lo)) * 1e3)
    return "    %-8s %9.1f us  (rounds %.1f .. %.1f, spread %.1f %%)  %6.1f TFLOPS on real columns%s" % (
        name, med * 1e3, lo * 1e3, hi * 1e3, 100.0 * (hi - lo) / med, flops / (med * 1e-3) / 1e12, rel)


def report(label, what, t, flops):
    print("%-12s %s" % (label, what))
    print(line("dv", t, flops, "pad_out"))
    print(line("dv", t, flops, "pad_in"))
    print(line("pad_out", t, flops))
    print(line("pad_in", t, flops, "pad_out"))
    print(line("dv_r128", t, flops, "dv"))
    print(line("dv_r256", t, flops, "dv"))
    sys.stdout.flush()


def forced(fn, rows):
    """fn under option "rows" = 128 | 256 (the option is process-wide: set and restored around every call)"""
    def run():
        with _fa2_lib.options(rows=rows):
            return fn()
    return run


def same_bits(label, a, b):
    for x, y in zip(a, b):
        if not torch.equal(x, y):
            raise SystemExit("mla_prefill_bench: %s: the Dv call and the padded route differ (max |diff| %.3g)" % (label, float((x.float() - y.float()).abs().max())))


def prefill_row(label, H, lens, rounds, iters):
    dev, dt = torch.device("cuda", 0), torch.bfloat16
    total, mx = sum(lens), max(lens)
    cu = cu_of(lens, dev)
    q, k = (torch.randn((total, H, D), device=dev, dtype=dt) for _ in range(2))
    v = torch.randn((total, H, DV), device=dev, dtype=dt)
    v_pad = torch.nn.functional.pad(v, (0, D - DV))

    def dv():
        return flash_attention_varlen(q, k, v, cu, cu, mx, mx, causal=True, return_lse=True)

    def pad_out():
        o, lse = flash_attention_varlen(q, k, v_pad, cu, cu, mx, mx, causal=True, return_lse=True)
        return o[..., :DV], lse

    def pad_in():
        o, lse = flash_attention_varlen(q, k, torch.nn.functional.pad(v, (0, D - DV)), cu, cu, mx, mx, causal=True, return_lse=True)
        return o[..., :DV], lse

    with torch.no_grad():
        same_bits(label, dv(), pad_out())
        t = interleaved({"dv": dv, "pad_out": pad_out, "pad_in": pad_in, "dv_r128": forced(dv, 128), "dv_r256": forced(dv, 256)}, rounds, iters)
    pairs = sum(n * (n + 1) // 2 for n in lens)
    report(label, "H%d, %d sequences, %d tokens (longest %d), causal, bf16 D %d / Dv %d" % (H, len(lens), total, mx, D, DV), t, 2.0 * (D + DV) * pairs * H)


def chunk_row(label, H, ctx, new, rounds, iters):
    dev, dt = torch.device("cuda", 0), torch.bfloat16
    cu_new, cu_ctx = cu_of([new], dev), cu_of([ctx], dev)
    q, k_new = (torch.randn((new, H, D), device=dev, dtype=dt) for _ in range(2))
    k_ctx = torch.randn((ctx, H, D), device=dev, dtype=dt)
    v_ctx, v_new = torch.randn((ctx, H, DV), device=dev, dtype=dt), torch.randn((new, H, DV), device=dev, dtype=dt)
    pad = lambda x: torch.nn.functional.pad(x, (0, D - DV))      # noqa: E731
    vp_ctx, vp_new = pad(v_ctx), pad(v_new)

    def two_pass(va, vb):
        oa, la = flash_attention_varlen(q, k_ctx, va, cu_new, cu_ctx, new, ctx, return_lse=True)
        ob, lb = flash_attention_varlen(q, k_new, vb, cu_new, cu_new, new, new, causal=True, return_lse=True)
        return merge_attention([oa[..., :DV], ob[..., :DV]], [la, lb])

    def dv():
        return two_pass(v_ctx, v_new)

    def pad_out():
        return two_pass(vp_ctx, vp_new)

    def pad_in():
        return two_pass(pad(v_ctx), pad(v_new))

    with torch.no_grad():
        same_bits(label, dv(), pad_out())
        t = interleaved({"dv": dv, "pad_out": pad_out, "pad_in": pad_in, "dv_r128": forced(dv, 128), "dv_r256": forced(dv, 256)}, rounds, iters)
    pairs = new * ctx + new * (new + 1) // 2
    report(label, "H%d, %d new tokens on %d context keys: non-causal pass + causal pass + merge, bf16 D %d / Dv %d" % (H, new, ctx, D, DV), t,
           2.0 * (D + DV) * pairs * H)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", default="all", choices=("prefill", "chunk", "all"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mla_prefill_bench: needs a ROCm GPU (a timing taken anywhere else says nothing)")
    print(torch.cuda.get_device_name(0), "rounds", a.rounds, "iters", a.iters, "|", _fa2_lib.load().fa2_version().decode())
    plan = _fa2_lib.FwdPlan()
    for H in (128, 16):
        _fa2_lib.check(_fa2_lib.load().fa2_fwd_varlen_dv_plan(_fa2_lib.FA2_DTYPE_BF16, 4, H, H, 4096, 4096, D, DV, None, None, D ** -0.5, _fa2_lib.FA2_FLAG_CAUSAL,
                                                              -1, -1, ctypes.byref(plan)))
        print("plan B4 H%d x 4096: kernel %d, rows %d, contract %d" % (H, plan.kernel, plan.rows, plan.contract))
    if a.rows in ("prefill", "all"):
        for r in PREFILL_ROWS:
            prefill_row(*r, a.rounds, a.iters)
    if a.rows in ("chunk", "all"):
        for r in CHUNK_ROWS:
            chunk_row(*r, a.rounds, a.iters)


if __name__ == "__main__":
    main()
