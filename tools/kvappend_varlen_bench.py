"""The packed (ragged) KV-cache append against what a caller had before it, same box, interleaved rounds, median of per-round event times with the spread
of the rounds beside it (tools/kvappend_bench.py's protocol: 9 rounds of 20 calls, spread = (max - min) / median).  H32 Hkv8 D128 bf16, 16-bit caches
unless a row says e4m3; every call rotates k (GPT-J pairing, f32 tables).

    python tools/kvappend_varlen_bench.py [--rounds R] [--iters I] [--rows uniform|step|fused|single|all]

Rows:
    uniform   B4 x 2 048-token chunk, kvcache_append_varlen against kvcache_append on the SAME tokens (16-bit and e4m3): the same useful work, so the
              difference prices the search and the cu_seqlens loads.  The uniform call's time, measured in the same run, is the reference.
    step      the ragged serving step of tools/prefill_bench.py — 24 decode rows + 4 x 384 — kvcache_append_varlen (one launch) against the loop of 28
              per-sequence kvcache_append calls on sliced views, which is what a caller does today and needs the lengths on the host.
    fused     the same step: flash_attention_prefill(k=, v=, rotary_*) against torch-op positions + rotation + index_put_ + flash_attention_prefill
              (no host read in either), each eagerly and as one replayed graph ("/g").  The two routes' outputs are checked against each other first.
    single    B256 single-token rows, packed against uniform: nine probes of cu_seqlens per token.
Every line: median us, the rounds' range, the spread; a comparison says whether the gap exceeds the sum of the two spreads."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))

import torch  # noqa: E402

from benchlib import close, graphed, interleaved  # noqa: E402
from rocwmma_fattn import _fa2_lib  # noqa: E402
from rocwmma_fattn.FlashAttn import flash_attention_prefill, kvcache_append, kvcache_append_varlen  # noqa: E402

E4M3 = torch.float8_e4m3fn
H, HKV, D, DT = 32, 8, 128, torch.bfloat16
STEP_LENS = [592 + (7947 - 592) * i // 27 for i in range(28)]       # the lengths AFTER the append
STEP_NQS = [384 if i % 7 == 3 else 1 for i in range(28)]


def line(name, t, base=None):
    med, lo, hi = t[name]
    rel = ""
    if base is not None and name != base:
        b_med, b_lo, b_hi = t[base]
        real = abs(b_med - med) > (hi - lo) + (b_hi - b_lo)          # the project's rule: a difference beyond the sum of the two spreads
        rel = "  %.2fx %s than %s (%+.1f us; %s the sum of the spreads, %.1f us)" % (max(b_med / med, med / b_med), "faster" if med <= b_med else "SLOWER", base,
                                                                                  (med - b_med) * 1e3, "beyond" if real else "WITHIN",
                                                                                  ((hi - lo) + (b_hi - b_lo)) * 1e3)
    return "    %-10s %9.1f us  (rounds %.1f .. %.1f, spread %.1f %%)%s" % (name, med * 1e3, lo * 1e3, hi * 1e3, 100.0 * (hi - lo) / med, rel)


def tables(n, dev):
    inv = 10000.0 ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
    ang = torch.arange(n, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().float().to(dev), ang.sin().float().to(dev)


def caches(B, nmax, fp8, dev, n=2):
    return tuple(torch.zeros((B, nmax, HKV, D), device=dev, dtype=torch.float16).to(E4M3 if fp8 else DT) for _ in range(n))


def equal_counts_row(label, B, N, fp8, rounds, iters):
    """packed against uniform on the same tokens"""
    dev = torch.device("cuda", 0)
    nmax = N + 256
    k, v = (torch.randn((B * N, HKV, D), device=dev, dtype=DT) for _ in range(2))
    kd = vd = None
    if fp8:
        kd, vd = (torch.full((B, HKV), 2.0 ** -5, device=dev) for _ in range(2))
    kc, vc, kc2, vc2 = caches(B, nmax, fp8, dev, 4)
    lens = torch.full((B,), N, dtype=torch.int32, device=dev)
    cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * N
    cos, sin = tables(nmax, dev)
    k4, v4 = k.view(B, N, HKV, D), v.view(B, N, HKV, D)
    fns = {"packed": lambda: kvcache_append_varlen(kc, vc, k, v, cu, lens, rotary_cos=cos, rotary_sin=sin, k_descale=kd, v_descale=vd),
           "uniform": lambda: kvcache_append(kc2, vc2, k4, v4, lens, rotary_cos=cos, rotary_sin=sin, k_descale=kd, v_descale=vd)}
    with torch.no_grad():
        fns["packed"]()
        fns["uniform"]()
        if not (torch.equal(kc.view(torch.uint8), kc2.view(torch.uint8)) and torch.equal(vc.view(torch.uint8), vc2.view(torch.uint8))):
            raise SystemExit("kvappend_varlen_bench: %s: the caches of the two calls differ" % label)
        fns.update({n + "/g": graphed(f) for n, f in list(fns.items())})
        t = interleaved(fns, rounds, iters)
    print("%-12s B%d x %d tokens Hkv%d D%d bf16 -> %s, k rotated" % (label, B, N, HKV, D, "e4m3" if fp8 else "16-bit"))
    for n, base in (("packed", "uniform"), ("uniform", None), ("packed/g", "uniform/g"), ("uniform/g", None)):
        print(line(n, t, base))
    sys.stdout.flush()


def rotate(x, cos, sin):
    """GPT-J pairing, f32 arithmetic: x [total, heads, D], cos / sin [total, D / 2] -> f32"""
    x = x.float()
    x1, x2 = x[..., 0::2], x[..., 1::2]
    c, s = cos[:, None, :], sin[:, None, :]
    return torch.stack((x1 * c - x2 * s, x1 * s + x2 * c), dim=-1).flatten(-2)


def torch_append(q, k, v, kc, vc, cu, lens, cos, sin):
    """The packed append as torch ops on device tensors, no host read: the sequence of every token by searchsorted, its position, rotation, index_put_.
    -> the rotated q"""
    t = torch.arange(k.shape[0], device=k.device)
    cul = cu.long()
    seq = torch.searchsorted(cul[1:], t, right=True).clamp(max=lens.numel() - 1)
    nnew = cul[seq + 1] - cul[seq]
    pos = lens.long()[seq] - nnew + (t - cul[seq])
    rows = pos.clamp(0, cos.shape[0] - 1)
    c, s = cos[rows], sin[rows]
    kc.index_put_((seq, pos), rotate(k, c, s).to(k.dtype))
    vc.index_put_((seq, pos), v)
    return rotate(q, c, s).to(q.dtype)


def step_rows(which, rounds, iters):
    dev = torch.device("cuda", 0)
    B, total, nmax = len(STEP_LENS), sum(STEP_NQS), 8192
    q, k, v = (torch.randn((total, h, D), device=dev, dtype=DT) for h in (H, HKV, HKV))
    cul = [0]
    for n in STEP_NQS:
        cul.append(cul[-1] + n)
    cu = torch.tensor(cul, dtype=torch.int32, device=dev)
    lens = torch.tensor(STEP_LENS, dtype=torch.int32, device=dev)
    kc, vc = (torch.randn((B, nmax, HKV, D), device=dev, dtype=DT) for _ in range(2))
    kc2, vc2 = kc.clone(), vc.clone()
    cos, sin = tables(nmax, dev)
    max_q = max(STEP_NQS)
    slices = [(kc2[s:s + 1], vc2[s:s + 1], k[cul[s]:cul[s + 1]][None], v[cul[s]:cul[s + 1]][None], lens[s:s + 1], q[cul[s]:cul[s + 1]][None]) for s in range(B)]

    def packed():
        return kvcache_append_varlen(kc, vc, k, v, cu, lens, rotary_cos=cos, rotary_sin=sin, q=q)

    def loop():
        return [kvcache_append(a, b, kk, vv, ll, rotary_cos=cos, rotary_sin=sin, q=qq) for (a, b, kk, vv, ll, qq) in slices]

    def fused():
        return flash_attention_prefill(q, kc, vc, cu, lens, max_seqlen_q=max_q, k=k, v=v, rotary_cos=cos, rotary_sin=sin)

    def torch_route():
        return flash_attention_prefill(torch_append(q, k, v, kc2, vc2, cu, lens, cos, sin), kc2, vc2, cu, lens, max_seqlen_q=max_q)

    print("ragged step  24 decode rows + 4 x 384 (%d tokens, B%d) H%d Hkv%d D%d bf16 contiguous 16-bit, lengths %d .. %d" % (total, B, H, HKV, D, min(STEP_LENS), max(STEP_LENS)))
    with torch.no_grad():
        if which in ("step", "all"):
            qa = packed()
            qb = torch.cat([x[0] for x in loop()])
            if not (torch.equal(qa.view(torch.int16), qb.view(torch.int16)) and torch.equal(kc.view(torch.int16), kc2.view(torch.int16))):
                raise SystemExit("kvappend_varlen_bench: the packed call and the loop differ")
            fns = {"packed": packed, "loop": loop}
            fns.update({n + "/g": graphed(f) for n, f in list(fns.items())})
            t = interleaved(fns, rounds, iters)
            print("  append alone (q rotated too): one packed launch against 28 uniform launches on sliced views")
            for n, base in (("packed", "loop"), ("loop", None), ("packed/g", "loop/g"), ("loop/g", None)):
                print(line(n, t, base))
        if which in ("fused", "all"):
            close("kvappend_varlen_bench", fused(), torch_route(), DT, "fused and torch outputs")
            close("kvappend_varlen_bench", kc.float(), kc2.float(), DT, "the K caches")
            if not torch.equal(vc.view(torch.int16), vc2.view(torch.int16)):
                raise SystemExit("kvappend_varlen_bench: the V caches of the two routes differ")
            fns = {"fused": fused, "torch": torch_route}
            fns.update({n + "/g": graphed(f) for n, f in list(fns.items())})
            t = interleaved(fns, rounds, iters)
            print("  append + rotate + attend: flash_attention_prefill(k=, v=, rotary_*) against torch ops + flash_attention_prefill")
            for n, base in (("fused", "torch"), ("torch", None), ("fused/g", "torch/g"), ("torch/g", None)):
                print(line(n, t, base))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", default="all", choices=("uniform", "step", "fused", "single", "all"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kvappend_varlen_bench: needs a ROCm GPU (a timing taken anywhere else says nothing)")
    print(torch.cuda.get_device_name(0), "rounds", a.rounds, "iters", a.iters, "|", _fa2_lib.load().fa2_version().decode())
    if a.rows in ("uniform", "all"):
        equal_counts_row("chunk_16bit", 4, 2048, False, a.rounds, a.iters)
        equal_counts_row("chunk_e4m3", 4, 2048, True, a.rounds, a.iters)
    if a.rows in ("step", "fused", "all"):
        step_rows(a.rows, a.rounds, a.iters)
    if a.rows in ("single", "all"):
        equal_counts_row("single_b256", 256, 1, False, a.rounds, a.iters)


if __name__ == "__main__":
    main()
