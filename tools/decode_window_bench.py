"""Decode attention with a sliding window, soft-capping and ALiBi slopes: tools/decode_bench.py's protocol — same box, interleaved
rounds, median of per-round event times with the spread of the rounds beside it.

    python tools/decode_window_bench.py [--rounds R] [--iters I] [--rows window|scoremod|plain|all] [--parent-lib PATH]

Window rows (B32 H32 Hkv8 Nq1 D128 bf16 and B1 H32 Hkv8 Nq1 D128 fp16; caches of 32 768 valid keys, contiguous and in pages of 64; window 1023, 4095):
    window     flash_attention_decode(window=W) on the full cache
    reference  the plain call on the same cache with lengths W + Nq: the kernel the library had, doing the same useful work — under the plan IT gets,
               which is the plan of the capacity (B1: 16 parts)
    ref@split  the plain call again, forced to the split the windowed plan chose: separates what the plan does from what the kernel does
    window@ref the windowed call on the reference's own lengths (its window starts at key 0): the windowed kernel on the reference's keys, which
               separates what the kernel's code costs from where in the cache its keys lie
    full       the plain call over all 32 768 keys: what the window saves
  "within" = |window - reference| <= the sum of the two rows' spreads, the project's criterion.
Score-modifier rows (the same shapes at 4 096 keys, 16-bit and e4m3 caches): softcap = 30 with [H] slopes against the plain call on the same shape.
Plain rows (--parent-lib: a libfa2_gfx950.so built from the parent commit): fa2_fwd_decode / fa2_fwd_decode_fp8 of both libraries on the shapes of
tools/decode_bench.py's uniform rows, interleaved in one process (tools/kbench.py's method); each row must be within the sum of its spreads.
Each row first checks its routes against each other on the timed inputs."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))

import torch  # noqa: E402

import decode_abi as dc  # noqa: E402 - the one copy of the C argument lists
from benchlib import close, interleaved, paged_pool  # noqa: E402
from rocwmma_fattn import _fa2_lib  # noqa: E402
from rocwmma_fattn.FlashAttn import flash_attention_decode  # noqa: E402

SHAPES = [("b32_hkv8_bf16", 32, 32, 8, 1, 128, torch.bfloat16), ("b1_hkv8_fp16", 1, 32, 8, 1, 128, torch.float16)]     # label, B, H, Hkv, Nq, D, dtype
PLAIN = [("b1_hkv8", 1, 32, 8, 1, 8192, 128, torch.float16), ("b1_hkv1_mqa", 1, 32, 1, 1, 8192, 128, torch.float16),
         ("b1_hkv32_mha", 1, 32, 32, 1, 8192, 128, torch.float16), ("b32_hkv8_bf16", 32, 32, 8, 1, 4096, 128, torch.bfloat16),
         ("b4_h8_d64", 4, 8, 8, 1, 16384, 64, torch.float16), ("b8_hkv8_nq4", 8, 32, 8, 4, 8192, 128, torch.float16)]       # tools/decode_bench.py's UNIFORM
KEYS = 32768


def report(label, shape, t, base, compare=()):
    """every route with its spread; the routes in `compare` against `base` under the sum-of-spreads rule"""
    print("%-22s %s" % (label, shape))
    b_med, b_lo, b_hi = t[base]
    for n, (med, lo, hi) in t.items():
        rel = ""
        if n in compare:
            s = (hi - lo) + (b_hi - b_lo)
            rel = "  %.2fx %s than %s: %s the sum of the spreads (%.1f us against %.1f us)" % (
                max(b_med / med, med / b_med), "faster" if med <= b_med else "SLOWER", base, "WITHIN" if abs(med - b_med) <= s else "beyond",
                abs(med - b_med) * 1e3, s * 1e3)
        elif n != base:
            rel = "  %.2fx of %s" % (med / b_med, base)
        print("    %-12s %9.1f us  (rounds %.1f .. %.1f, spread %.1f %%)%s" % (n, med * 1e3, lo * 1e3, hi * 1e3, 100.0 * (hi - lo) / med, rel))
    sys.stdout.flush()


def window_rows(label, B, H, Hkv, Nq, D, dt, rounds, iters):
    dev = torch.device("cuda", 0)
    code = 0 if dt == torch.float16 else 1
    q = torch.randn((B, Nq, H, D), device=dev, dtype=dt)
    kc, vc = (torch.randn((B, KEYS, Hkv, D), device=dev, dtype=dt) for _ in range(2))
    pk, pv, bt = paged_pool(kc, vc, 64, torch.Generator(device="cpu").manual_seed(5), spare=0)
    full = torch.full((B,), KEYS, dtype=torch.int32, device=dev)
    for layout, (k, v, kw) in (("contiguous", (kc, vc, {})), ("pages of 64", (pk, pv, dict(block_table=bt)))):
        for W in (1023, 4095):
            short = torch.full((B,), W + Nq, dtype=torch.int32, device=dev)
            ns = _fa2_lib.decode_window_plan(code, B, H, Hkv, Nq, D, KEYS if not kw else KEYS // 64, 64 if kw else 0, 0, W).nsplit
            ns0 = _fa2_lib.decode_plan(code, B, H, Hkv, Nq, D, KEYS if not kw else KEYS // 64, 64 if kw else 0).nsplit
            fns = {"reference": lambda: flash_attention_decode(q, k, v, short, **kw),
                   "window": lambda: flash_attention_decode(q, k, v, full, window=W, **kw),
                   "ref@split": lambda: flash_attention_decode(q, k, v, short, num_splits=ns, **kw),
                   "window@ref": lambda: flash_attention_decode(q, k, v, short, window=W, **kw),
                   "full": lambda: flash_attention_decode(q, k, v, full, **kw)}
            with torch.no_grad():
                lo = KEYS - Nq - W           # the window of a full cache is the plain call on that slice of it
                close("decode_window_bench", flash_attention_decode(q, kc, vc, full, window=W), flash_attention_decode(q, kc[:, lo:], vc[:, lo:], short), dt,
                      label + ": window and slice")
                close("decode_window_bench", fns["window"](), flash_attention_decode(q, kc, vc, full, window=W), dt, label + ": the layouts")
                t = interleaved(fns, rounds, iters)
            shape = "B%d H%d Hkv%d Nq%d D%d %s, %d valid keys, %s, window %d (split %d; reference and full: split %d)" % (
                B, H, Hkv, Nq, D, "fp16" if dt == torch.float16 else "bf16", KEYS, layout, W, ns, ns0)
            report(label + "_w%d" % W, shape, t, "reference", compare=("window",))


def scoremod_rows(label, B, H, Hkv, Nq, D, dt, rounds, iters):
    dev = torch.device("cuda", 0)
    keys, nmax = 4096, 4096 + 256
    q = torch.randn((B, Nq, H, D), device=dev, dtype=dt)
    kc, vc = (torch.randn((B, nmax, Hkv, D), device=dev, dtype=dt) for _ in range(2))
    lens = torch.full((B,), keys, dtype=torch.int32, device=dev)
    sl = torch.tensor([2.0 ** (-8.0 * (i + 1) / H) for i in range(H)], dtype=torch.float32, device=dev)
    d = torch.full((B, Hkv), 2.0 ** -6, device=dev)
    k8, v8 = ((t.float() / 2.0 ** -6).clamp(-448.0, 448.0).to(torch.float8_e4m3fn) for t in (kc, vc))
    fns = {"plain": lambda: flash_attention_decode(q, kc, vc, lens),
           "cap+alibi": lambda: flash_attention_decode(q, kc, vc, lens, softcap=30.0, alibi_slopes=sl),
           "plain_e4m3": lambda: flash_attention_decode(q, k8, v8, lens, k_descale=d, v_descale=d),
           "cap+alibi_e4m3": lambda: flash_attention_decode(q, k8, v8, lens, k_descale=d, v_descale=d, softcap=30.0, alibi_slopes=sl)}
    with torch.no_grad():
        zero = torch.zeros_like(sl)
        close("decode_window_bench", flash_attention_decode(q, kc, vc, lens, alibi_slopes=zero), fns["plain"](), dt,
              label + ": the banded kernel with zero slopes and plain")
        t = interleaved(fns, rounds, iters)
    shape = "B%d H%d Hkv%d Nq%d D%d %s, %d keys, softcap 30 and [H] slopes" % (B, H, Hkv, Nq, D, "fp16" if dt == torch.float16 else "bf16", keys)
    report(label + "_smod", shape, {n: t[n] for n in ("plain", "cap+alibi")}, "plain")
    report(label + "_smod_e4m3", shape, {n: t[n] for n in ("plain_e4m3", "cap+alibi_e4m3")}, "plain_e4m3")


def plain_rows(parent_path, rounds, iters):
    """fa2_fwd_decode / fa2_fwd_decode_fp8 of this library and of the parent's, the same tensors, interleaved"""
    dev = torch.device("cuda", 0)
    libs = {"this": _fa2_lib.load(), "parent": ctypes.CDLL(parent_path)}
    names = ("fa2_fwd_decode", "fa2_fwd_decode_fp8", "fa2_fwd_decode_workspace_bytes")
    for n in names:
        getattr(libs["parent"], n).restype, getattr(libs["parent"], n).argtypes = _fa2_lib.SYMBOLS[n]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (label, B, H, Hkv, Nq, keys, D, dt) in PLAIN:
        code = 0 if dt == torch.float16 else 1
        nmax = keys + 256
        q = torch.randn((B, Nq, H, D), device=dev, dtype=dt)
        kc, vc = (torch.randn((B, nmax, Hkv, D), device=dev, dtype=dt) for _ in range(2))
        k8, v8 = ((t.float() * 64.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn) for t in (kc, vc))
        d = torch.full((B, Hkv), 2.0 ** -6, device=dev)
        lens = torch.full((B,), keys, dtype=torch.int32, device=dev)
        need = libs["this"].fa2_fwd_decode_workspace_bytes(code, B, H, Hkv, Nq, D, nmax, 0, 0)
        assert need == libs["parent"].fa2_fwd_decode_workspace_bytes(code, B, H, Hkv, Nq, D, nmax, 0, 0)
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        outs = {}

        def make(lib, fp8, key):
            o = torch.empty((B, Nq, H, D), device=dev, dtype=dt)
            lse = torch.empty((B, H, Nq), device=dev, dtype=torch.float32)
            outs[key] = (o, lse)
            k, v, dd = (k8, v8, d) if fp8 else (kc, vc, None)
            entry = "fp8" if fp8 else "plain"
            args = dc.c_args(entry, **dc.tensor_kw(q, k, v, o, lse, lens, kd=dd, vd=dd), ns=0, ws=ws.data_ptr() if need else None, wsb=need, stream=stream)
            return lambda: _fa2_lib.check(getattr(lib, dc.ENTRIES[entry][0])(*args))

        for fp8 in (False, True):
            fns = {n: make(lib, fp8, (n, fp8)) for n, lib in libs.items()}
            for f in fns.values():
                f()
            torch.cuda.synchronize()
            same = all(torch.equal(a, b) for a, b in zip(outs[("this", fp8)], outs[("parent", fp8)]))
            t = interleaved(fns, rounds, iters)
            shape = "B%d H%d Hkv%d Nq%d keys %d D%d %s %s cache, C-ABI call; outputs %s" % (
                B, H, Hkv, Nq, keys, D, "fp16" if dt == torch.float16 else "bf16", "e4m3" if fp8 else "16-bit", "bit-identical" if same else "DIFFER")
            report(label + ("_e4m3" if fp8 else ""), shape, t, "parent", compare=("this",))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", default="all", choices=("window", "scoremod", "plain", "all"))
    ap.add_argument("--parent-lib", default=None, help="a libfa2_gfx950.so built from the parent commit (the plain rows)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_window_bench: needs a ROCm GPU (a timing taken anywhere else says nothing)")
    print(torch.cuda.get_device_name(0), "rounds", a.rounds, "iters", a.iters, "|", _fa2_lib.load().fa2_version().decode())
    if a.rows in ("window", "all"):
        for s in SHAPES:
            window_rows(*s, a.rounds, a.iters)
    if a.rows in ("scoremod", "all"):
        for s in SHAPES:
            scoremod_rows(*s, a.rounds, a.iters)
    if a.rows in ("plain", "all"):
        if not a.parent_lib:
            print("plain rows skipped: no --parent-lib")
        else:
            plain_rows(a.parent_lib, a.rounds, a.iters)


if __name__ == "__main__":
    main()
