"""KV-cache decode attention: flash_attention_decode against the routes the library had before it, same box, interleaved rounds, median of
per-round event times with the spread of the rounds beside it (tools/gqa_bench.py practice).

    python tools/decode_bench.py [--rounds R] [--iters I] [--rows uniform|ragged|fp8|all]

Uniform rows (every sequence has the same length, so the older entry points can serve the call at all):
    decode  flash_attention_decode(q, k_cache, v_cache, cache_seqlens) on a [B, Nmax, Hkv, D] cache with Nmax above the length
    dense   flash_attention(q, k[:, :, :len], v[:, :, :len]) on [B, Hkv, Nmax, D] tensors, the layout that call prefers (Nq > 1: causal=True with
            q_offset = len - Nq, the same bottom-right mask) — the BASELINE: what a caller had to run before
Ragged rows (B sequences with lengths drawn from 256 .. 8192):
    decode / paged64 / paged256   the contiguous cache, and the same data in pages of 64 / 256 keys in shuffled physical order
    varlen        flash_attention_varlen(causal=True, bottom_right=True) on a packed copy of the valid keys made OUTSIDE the timed region
    varlen+copy   ... with the packing (one torch.cat of the per-sequence slices per tensor) inside it: what serving a cache through it costs per step
    padmask       flash_attention(mask = key padding [B, 1, 1, Nmax]) on the padded cache
FP8 rows (--rows fp8): the e4m3 cache with per (sequence, K / V head) descales beside the 16-bit call on the same shape and the
same (dequantised) values, in the same interleaved protocol:
    bf16 / fp16   flash_attention_decode on the 16-bit cache — the route the library had
    fp8           flash_attention_decode(k_descale=, v_descale=) on the e4m3 cache: half the bytes
    dequant+call  (one row) the whole e4m3 cache dequantised to the 16-bit dtype inside the timed region, then the 16-bit call: what a holder of
                  such a cache had to do per step before
Each route's TB/s is of ITS OWN valid bytes, and the floor is printed for both cache widths.
Every row prints the K + V bytes that are valid (what a perfect kernel has to read) and the time they take at 6.3 TB/s, the achievable HBM rate.
Each row first checks the routes against each other on the timed inputs (fp16 1e-3 + 2e-3 |x|, bf16 8e-3 + 1.6e-2 |x|): faster and different is not faster.
The same K / V are read in every iteration, so caches up to the 256 MB of Infinity Cache are served from it in every route alike.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))

import torch  # noqa: E402

from benchlib import close, interleaved, paged_pool  # noqa: E402
from rocwmma_fattn import _fa2_lib  # noqa: E402
from rocwmma_fattn.FlashAttn import flash_attention, flash_attention_decode, flash_attention_varlen  # noqa: E402

HBM_TBS = 6.3
UNIFORM = [  # (label, B, H, Hkv, Nq, keys, D, dtype)
    ("b1_hkv8", 1, 32, 8, 1, 8192, 128, torch.float16),
    ("b1_hkv1_mqa", 1, 32, 1, 1, 8192, 128, torch.float16),
    ("b1_hkv32_mha", 1, 32, 32, 1, 8192, 128, torch.float16),
    ("b32_hkv8_bf16", 32, 32, 8, 1, 4096, 128, torch.bfloat16),
    ("b4_h8_d64", 4, 8, 8, 1, 16384, 64, torch.float16),
    ("b8_hkv8_nq4", 8, 32, 8, 4, 8192, 128, torch.float16),
]
RAGGED = ("ragged_b32", 32, 32, 8, 1, 256, 8192, 128, torch.float16)      # label, B, H, Hkv, Nq, shortest, longest, D, dtype


def report(label, shape, t, valid_bytes, base):
    floor_us = valid_bytes / (HBM_TBS * 1e12) * 1e6
    print("%-14s %s  valid K+V %.1f MB = %.1f us at %.1f TB/s" % (label, shape, valid_bytes / 1e6, floor_us, HBM_TBS))
    b_med, b_lo, b_hi = t[base]
    for n, (med, lo, hi) in t.items():
        rel = "" if n == base else "  %.2fx faster than %s" % (b_med / med, base) if med <= b_med else "  %.2fx SLOWER than %s" % (med / b_med, base)
        print("    %-12s %9.1f us  (rounds %.1f .. %.1f, spread %.1f %%)  %5.2f TB/s of valid K+V%s"
              % (n, med * 1e3, lo * 1e3, hi * 1e3, 100.0 * (hi - lo) / med, valid_bytes / (med * 1e-3) / 1e12, rel))
    sys.stdout.flush()


def uniform_row(label, B, H, Hkv, Nq, keys, D, dt, rounds, iters):
    dev = torch.device("cuda", 0)
    nmax = keys + 256                                        # a cache with room to grow, as in serving
    q = torch.randn((B, Nq, H, D), device=dev, dtype=dt)
    kc, vc = (torch.randn((B, nmax, Hkv, D), device=dev, dtype=dt) for _ in range(2))
    lens = torch.full((B,), keys, dtype=torch.int32, device=dev)
    qh = q.transpose(1, 2).contiguous()                      # the dense call's layout: [B, H, N, D] and a [B, Hkv, Nmax, D] cache
    kh, vh = kc.transpose(1, 2).contiguous(), vc.transpose(1, 2).contiguous()
    if Nq == 1:
        dense = lambda: flash_attention(qh, kh[:, :, :keys], vh[:, :, :keys])  # noqa: E731
    else:
        dense = lambda: flash_attention(qh, kh[:, :, :keys], vh[:, :, :keys], causal=True, q_offset=keys - Nq)  # noqa: E731
    fns = {"decode": lambda: flash_attention_decode(q, kc, vc, lens), "dense": dense}
    with torch.no_grad():
        close("decode_bench", fns["decode"]().transpose(1, 2), fns["dense"](), dt, label + ": decode and dense")
        t = interleaved(fns, rounds, iters)
    plan = _fa2_lib.decode_plan(0 if dt == torch.float16 else 1, B, H, Hkv, Nq, D, nmax)
    shape = "B%d H%d Hkv%d Nq%d keys %d D%d %s (split %d, %d row tile%s)" % (B, H, Hkv, Nq, keys, D, "fp16" if dt == torch.float16 else "bf16", plan.nsplit,
                                                                              plan.row_tiles, "" if plan.row_tiles == 1 else "s")
    report(label, shape, t, 2 * B * Hkv * keys * D * 2, "dense")


FP8_UNIFORM = [r for r in UNIFORM if r[0] in ("b32_hkv8_bf16", "b8_hkv8_nq4", "b1_hkv8")]
FP8_DEQUANT_ROW = "b32_hkv8_bf16"


def report_fp8(label, shape, t, bytes16, base):
    """rows of an fp8 comparison: every route against `base` (the 16-bit call), TB/s of the route's own valid bytes (fp8: half)"""
    print("%-14s %s  valid K+V %.1f MB = %.1f us (16-bit) / %.1f MB = %.1f us (e4m3) at %.1f TB/s"
          % (label, shape, bytes16 / 1e6, bytes16 / (HBM_TBS * 1e12) * 1e6, bytes16 / 2e6, bytes16 / 2 / (HBM_TBS * 1e12) * 1e6, HBM_TBS))
    b_med, b_lo, b_hi = t[base]
    for n, (med, lo, hi) in t.items():
        own = bytes16 // 2 if n.startswith("fp8") else bytes16
        rel = ""
        if n != base:
            real = abs(b_med - med) > (hi - lo) + (b_hi - b_lo)          # the project's rule: a difference beyond the sum of the two spreads
            rel = "  %.2fx %s than %s (%s the sum of the spreads, %.1f us)" % (max(b_med / med, med / b_med), "faster" if med <= b_med else "SLOWER", base,
                                                                              "beyond" if real else "WITHIN", ((hi - lo) + (b_hi - b_lo)) * 1e3)
        print("    %-12s %9.1f us  (rounds %.1f .. %.1f, spread %.1f %%)  %5.2f TB/s of its valid K+V%s"
              % (n, med * 1e3, lo * 1e3, hi * 1e3, 100.0 * (hi - lo) / med, own / (med * 1e-3) / 1e12, rel))
    sys.stdout.flush()


def quantise(x, g):
    """unit-scale x [B, N, Hkv, D] -> (e4m3 cache, descale [B, Hkv] of powers of two, the dequantised values in x's dtype — exact)"""
    B, Hkv = x.shape[0], x.shape[2]
    d = (2.0 ** -torch.randint(5, 8, (B, Hkv), generator=g).float()).to(x.device)
    x8 = (x.float() / d[:, None, :, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return x8, d, (x8.float() * d[:, None, :, None]).to(x.dtype)


def fp8_uniform_row(label, B, H, Hkv, Nq, keys, D, dt, rounds, iters):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(2)
    nmax = keys + 256
    name16 = "fp16" if dt == torch.float16 else "bf16"
    q = torch.randn((B, Nq, H, D), device=dev, dtype=dt)
    (k8, kd, kc), (v8, vd, vc) = (quantise(torch.randn((B, nmax, Hkv, D), device=dev, dtype=dt), g) for _ in range(2))
    lens = torch.full((B,), keys, dtype=torch.int32, device=dev)
    fns = {name16: lambda: flash_attention_decode(q, kc, vc, lens),
           "fp8": lambda: flash_attention_decode(q, k8, v8, lens, k_descale=kd, v_descale=vd)}
    if label == FP8_DEQUANT_ROW:
        dq = lambda x8, d: x8.to(dt) * d[:, None, :, None].to(dt)  # noqa: E731
        fns["dequant+call"] = lambda: flash_attention_decode(q, dq(k8, kd), dq(v8, vd), lens)
    with torch.no_grad():
        for n in fns:
            close("decode_bench", fns[n](), fns[name16](), dt, label + ": %s and %s" % (n, name16))
        t = interleaved(fns, rounds, iters)
    plan = _fa2_lib.decode_fp8_plan(0 if dt == torch.float16 else 1, B, H, Hkv, Nq, D, nmax)
    shape = "B%d H%d Hkv%d Nq%d keys %d D%d %s (split %d, key tile %d)" % (B, H, Hkv, Nq, keys, D, name16, plan.nsplit, plan.key_tile)
    report_fp8(label + "_fp8", shape, t, 2 * B * Hkv * keys * D * 2, name16)


def fp8_ragged_row(label, B, H, Hkv, Nq, lo, hi, D, dt, rounds, iters):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(1)
    lens_h = torch.randint(lo, hi + 1, (B,), generator=g).tolist()
    name16 = "fp16" if dt == torch.float16 else "bf16"
    q = torch.randn((B, Nq, H, D), device=dev, dtype=dt)
    (k8, kd, kc), (v8, vd, vc) = (quantise(torch.randn((B, hi, Hkv, D), device=dev, dtype=dt), g) for _ in range(2))
    lens = torch.tensor(lens_h, dtype=torch.int32, device=dev)
    p16 = paged_pool(kc, vc, 64, torch.Generator(device="cpu").manual_seed(3), lens=lens_h)
    p8 = paged_pool(k8.view(torch.uint8), v8.view(torch.uint8), 64, torch.Generator(device="cpu").manual_seed(3), lens=lens_h)
    pk8, pv8 = p8[0].view(torch.float8_e4m3fn), p8[1].view(torch.float8_e4m3fn)
    fns = {name16: lambda: flash_attention_decode(q, kc, vc, lens),
           "fp8": lambda: flash_attention_decode(q, k8, v8, lens, k_descale=kd, v_descale=vd),
           name16 + "_pg64": lambda: flash_attention_decode(q, p16[0], p16[1], lens, block_table=p16[2]),
           "fp8_pg64": lambda: flash_attention_decode(q, pk8, pv8, lens, block_table=p8[2], k_descale=kd, v_descale=vd)}
    with torch.no_grad():
        for n in fns:
            close("decode_bench", fns[n](), fns[name16](), dt, label + ": %s and %s" % (n, name16))
        t = interleaved(fns, rounds, max(1, iters // 2))
    plan = _fa2_lib.decode_fp8_plan(0 if dt == torch.float16 else 1, B, H, Hkv, Nq, D, hi)
    shape = "B%d H%d Hkv%d Nq%d keys %d .. %d (mean %d) D%d %s (split %d, key tile %d)" % (B, H, Hkv, Nq, min(lens_h), max(lens_h), sum(lens_h) // B, D, name16,
                                                                                          plan.nsplit, plan.key_tile)
    bytes16 = 2 * Hkv * sum(lens_h) * D * 2
    report_fp8(label + "_fp8", shape, {n: t[n] for n in (name16, "fp8")}, bytes16, name16)
    report_fp8(label + "_fp8_pg64", shape, {n: t[n] for n in (name16 + "_pg64", "fp8_pg64")}, bytes16, name16 + "_pg64")


def ragged_row(label, B, H, Hkv, Nq, lo, hi, D, dt, rounds, iters):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(1)
    lens_h = torch.randint(lo, hi + 1, (B,), generator=g).tolist()
    nmax = hi
    q = torch.randn((B, Nq, H, D), device=dev, dtype=dt)
    kc, vc = (torch.randn((B, nmax, Hkv, D), device=dev, dtype=dt) for _ in range(2))
    lens = torch.tensor(lens_h, dtype=torch.int32, device=dev)
    cu_q = torch.arange(0, (B + 1) * Nq, Nq, dtype=torch.int32, device=dev)
    cu_k = torch.tensor([0] + list(torch.tensor(lens_h).cumsum(0)), dtype=torch.int32, device=dev)
    qp = q.reshape(B * Nq, H, D)
    pack = lambda t: torch.cat([t[b, :n] for b, n in enumerate(lens_h)])  # noqa: E731
    kp, vp = pack(kc), pack(vc)
    qh, kh, vh = q.transpose(1, 2).contiguous(), kc.transpose(1, 2).contiguous(), vc.transpose(1, 2).contiguous()
    keep = (torch.arange(nmax, device=dev)[None, :] < lens[:, None]).view(B, 1, 1, nmax)
    p64, p256 = paged_pool(kc, vc, 64, g, lens=lens_h), paged_pool(kc, vc, 256, g, lens=lens_h)
    fns = {
        "decode": lambda: flash_attention_decode(q, kc, vc, lens),
        "paged64": lambda: flash_attention_decode(q, p64[0], p64[1], lens, block_table=p64[2]),
        "paged256": lambda: flash_attention_decode(q, p256[0], p256[1], lens, block_table=p256[2]),
        "varlen": lambda: flash_attention_varlen(qp, kp, vp, cu_q, cu_k, Nq, hi, causal=True, bottom_right=True),
        "varlen+copy": lambda: flash_attention_varlen(qp, pack(kc), pack(vc), cu_q, cu_k, Nq, hi, causal=True, bottom_right=True),
        "padmask": lambda: flash_attention(qh, kh, vh, mask=keep),
    }
    with torch.no_grad():
        want = fns["varlen"]().reshape(B, Nq, H, D)
        for n in ("decode", "paged64", "paged256"):
            close("decode_bench", fns[n](), want, dt, label + ": %s and varlen" % n)
        close("decode_bench", fns["padmask"]().transpose(1, 2), want, dt, label + ": padmask and varlen")
        t = interleaved(fns, rounds, max(1, iters // 2))
    plan = _fa2_lib.decode_plan(0 if dt == torch.float16 else 1, B, H, Hkv, Nq, D, nmax)
    shape = "B%d H%d Hkv%d Nq%d keys %d .. %d (mean %d) D%d %s (split %d)" % (B, H, Hkv, Nq, min(lens_h), max(lens_h), sum(lens_h) // B, D,
                                                                             "fp16" if dt == torch.float16 else "bf16", plan.nsplit)
    report(label, shape, t, 2 * Hkv * sum(lens_h) * D * 2, "varlen")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", default="all", choices=("uniform", "ragged", "fp8", "all"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench: needs a ROCm GPU (a timing taken anywhere else says nothing)")
    print(torch.cuda.get_device_name(0), "rounds", a.rounds, "iters", a.iters, "|", _fa2_lib.load().fa2_version().decode())
    if a.rows in ("uniform", "all"):
        for r in UNIFORM:
            uniform_row(*r, a.rounds, a.iters)
    if a.rows in ("ragged", "all"):
        ragged_row(*RAGGED, a.rounds, a.iters)
    if a.rows in ("fp8", "all"):
        for r in FP8_UNIFORM:
            fp8_uniform_row(*r, a.rounds, a.iters)
        fp8_ragged_row(*RAGGED, a.rounds, a.iters)


if __name__ == "__main__":
    main()
