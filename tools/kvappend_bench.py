"""One serving step — append the new tokens' K / V, rotate q and k, quantise for an e4m3 cache, decode — through the library's append launch against the
route a caller had before it, same box, interleaved rounds, median of per-round event times with the spread of the rounds beside it
(tools/decode_bench.py's protocol: 9 rounds of 20 calls, spread = (max - min) / median).

    python tools/kvappend_bench.py [--rounds R] [--iters I] [--rows step|chunk|all]

Step rows (cache_seqlens counts the new tokens; every sequence has `keys` keys after the append):
    fused        flash_attention_decode(q, ..., k=, v=, rotary_cos=, rotary_sin=): the append launch, then the decode call on the rotated q
    torch        the route before: torch ops compute the positions (and page slots) from the device tensors, gather the table rows and rotate q and
                 k, divide-clamp-cast for an e4m3 cache, index_put_ into the cache, then flash_attention_decode — no host read either
    append       kvcache_append(..., q=q) alone: the price of keeping the decode kernels untouched
    decode       flash_attention_decode on an already appended cache alone
Each of the four is timed eagerly and, with a "/g" suffix, as a replayed graph.  fused and torch are first checked against each other on the timed
inputs (the caches bit for bit where nothing is rotated, within a rounding of the cache format where k is; the outputs fp16 1e-3 + 2e-3 |x|, bf16
8e-3 + 1.6e-2 |x|): faster and different is not faster.
Chunk rows: a standalone append of B4 x 2 048 tokens (a prefill chunk), 16-bit and e4m3, with the GB/s of its own bytes (k and v read once, the cache
rows written once) and the time those bytes take at 6.3 TB/s."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))

import torch  # noqa: E402

from benchlib import close, graphed, interleaved, paged_pool  # noqa: E402
from rocwmma_fattn import _fa2_lib  # noqa: E402
from rocwmma_fattn.FlashAttn import flash_attention_decode, kvcache_append  # noqa: E402

HBM_TBS = 6.3
E4M3 = torch.float8_e4m3fn
STEP_ROWS = [  # (label, B, H, Hkv, Nq, keys, D, dtype, page, fp8)
    ("b32_contig", 32, 32, 8, 1, 4096, 128, torch.bfloat16, 0, False),
    ("b32_pg64", 32, 32, 8, 1, 4096, 128, torch.bfloat16, 64, False),
    ("b32_e4m3", 32, 32, 8, 1, 4096, 128, torch.bfloat16, 0, True),
    ("b1_8k", 1, 32, 8, 1, 8192, 128, torch.bfloat16, 0, False),
    ("b8_nq4_8k", 8, 32, 8, 4, 8192, 128, torch.bfloat16, 0, False),
]
CHUNK_ROWS = [("chunk_16bit", 4, 2048, 8, 128, torch.bfloat16, False), ("chunk_e4m3", 4, 2048, 8, 128, torch.bfloat16, True)]


def rotate(x, cos, sin):
    """GPT-J pairing, f32 arithmetic: x [B, N, heads, D], cos / sin [B, N, D / 2] -> f32"""
    x = x.float()
    x1, x2 = x[..., 0::2], x[..., 1::2]
    c, s = cos[:, :, None, :], sin[:, :, None, :]
    return torch.stack((x1 * c - x2 * s, x1 * s + x2 * c), dim=-1).flatten(-2)


def torch_append(q, k, v, kc, vc, lens, bt, cos, sin, kd, vd):
    """The route before the append launch: positions, page slots, rotation, quantisation and the cache write as torch ops on device tensors.
    -> the rotated q (q None: a standalone append)"""
    B, N = k.shape[:2]
    pos = lens.long()[:, None] - N + torch.arange(N, device=k.device)[None, :]
    rows = pos.clamp(0, cos.shape[0] - 1)
    c, s = cos[rows], sin[rows]
    q_rot = None if q is None else rotate(q, c, s).to(q.dtype)
    kr, vr = rotate(k, c, s), v
    if kc.dtype == E4M3:
        kr = (kr / kd[:, None, :, None]).clamp(-448.0, 448.0).to(E4M3).view(torch.uint8)
        vr = (v.float() / vd[:, None, :, None]).clamp(-448.0, 448.0).to(E4M3).view(torch.uint8)
        kc, vc = kc.view(torch.uint8), vc.view(torch.uint8)
    else:
        kr = kr.to(k.dtype)
    if bt is None:
        idx = (torch.arange(B, device=k.device)[:, None].expand(B, N), pos)
    else:
        page = kc.shape[1]
        idx = (bt.gather(1, pos // page).long(), pos % page)
    kc.index_put_(idx, kr)
    vc.index_put_(idx, vr)
    return q_rot


def line(name, t, base=None):
    med, lo, hi = t[name]
    rel = ""
    if base is not None and name != base:
        b_med, b_lo, b_hi = t[base]
        real = abs(b_med - med) > (hi - lo) + (b_hi - b_lo)          # the project's rule: a difference beyond the sum of the two spreads
        rel = "  %.2fx %s than %s (%s the sum of the spreads, %.1f us)" % (max(b_med / med, med / b_med), "faster" if med <= b_med else "SLOWER", base,
                                                                          "beyond" if real else "WITHIN", ((hi - lo) + (b_hi - b_lo)) * 1e3)
    return "    %-10s %9.1f us  (rounds %.1f .. %.1f, spread %.1f %%)%s" % (name, med * 1e3, lo * 1e3, hi * 1e3, 100.0 * (hi - lo) / med, rel)


def step_row(label, B, H, Hkv, Nq, keys, D, dt, page, fp8, rounds, iters):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(4)
    nmax = keys + 256
    q, k, v = (torch.randn((B, Nq, h, D), device=dev, dtype=dt) for h in (H, Hkv, Hkv))
    kc, vc = (torch.randn((B, nmax, Hkv, D), device=dev, dtype=dt) for _ in range(2))
    kd = vd = None
    if fp8:
        kd, vd = ((2.0 ** -torch.randint(5, 8, (B, Hkv), generator=g).float()).to(dev) for _ in range(2))
        kc, vc = ((x.float() / d[:, None, :, None]).clamp(-448.0, 448.0).to(E4M3) for x, d in ((kc, kd), (vc, vd)))
    bt = None
    if page:
        kc, vc, bt = paged_pool(kc, vc, page, g)
    lens = torch.full((B,), keys, dtype=torch.int32, device=dev)
    inv = 10000.0 ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
    ang = torch.arange(nmax, dtype=torch.float64)[:, None] * inv[None, :]
    cos, sin = ang.cos().float().to(dev), ang.sin().float().to(dev)
    kc2, vc2 = kc.clone(), vc.clone()                                    # the torch route's own caches
    dec = dict(block_table=bt, k_descale=kd, v_descale=vd)

    def fused():
        return flash_attention_decode(q, kc, vc, lens, k=k, v=v, rotary_cos=cos, rotary_sin=sin, **dec)

    def torch_route():
        return flash_attention_decode(torch_append(q, k, v, kc2, vc2, lens, bt, cos, sin, kd, vd), kc2, vc2, lens, **dec)

    def append():
        return kvcache_append(kc, vc, k, v, lens, block_table=bt, rotary_cos=cos, rotary_sin=sin, k_descale=kd, v_descale=vd, q=q)

    def decode():
        return flash_attention_decode(q, kc, vc, lens, **dec)

    with torch.no_grad():
        close("kvappend_bench", fused(), torch_route(), dt, label + ": fused and torch outputs")
        a, b = kc.float(), kc2.float()
        if fp8:                                                          # at most one e4m3 step apart where the two f32 rotations round differently
            if bool(((a - b).abs() > 0.126 * b.abs() + 2.0 ** -9).any()):
                raise SystemExit("kvappend_bench: %s: the K caches of the two routes differ by more than one e4m3 step" % label)
        else:
            close("kvappend_bench", a, b, dt, label + ": the K caches")
        if not torch.equal(vc.view(torch.uint8), vc2.view(torch.uint8)):
            raise SystemExit("kvappend_bench: %s: the V caches of the two routes differ" % label)
        fns = {"fused": fused, "torch": torch_route, "append": append, "decode": decode}
        fns.update({n + "/g": graphed(f) for n, f in list(fns.items())})
        t = interleaved(fns, rounds, iters)
    print("%-12s B%d H%d Hkv%d Nq%d keys %d D%d %s %s %s" % (label, B, H, Hkv, Nq, keys, D, "fp16" if dt == torch.float16 else "bf16",
                                                             "pages of %d" % page if page else "contiguous", "e4m3" if fp8 else "16-bit"))
    for n in ("fused", "torch", "append", "decode"):
        print(line(n, t, "torch" if n == "fused" else None))
    for n in ("fused/g", "torch/g", "append/g", "decode/g"):
        print(line(n, t, "torch/g" if n == "fused/g" else None))
    sys.stdout.flush()


def chunk_row(label, B, N, Hkv, D, dt, fp8, rounds, iters):
    dev = torch.device("cuda", 0)
    nmax = N + 256
    k, v = (torch.randn((B, N, Hkv, D), device=dev, dtype=dt) for _ in range(2))
    kd = vd = None
    cdt = dt
    if fp8:
        kd, vd = (torch.full((B, Hkv), 2.0 ** -5, device=dev) for _ in range(2))
        cdt = E4M3
    kc, vc, kc2, vc2 = (torch.zeros((B, nmax, Hkv, D), device=dev, dtype=torch.float16).to(cdt) for _ in range(4))
    lens = torch.full((B,), N, dtype=torch.int32, device=dev)
    inv = 10000.0 ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
    ang = torch.arange(nmax, dtype=torch.float64)[:, None] * inv[None, :]
    cos, sin = ang.cos().float().to(dev), ang.sin().float().to(dev)
    fns = {"append": lambda: kvcache_append(kc, vc, k, v, lens, rotary_cos=cos, rotary_sin=sin, k_descale=kd, v_descale=vd),
           "torch": lambda: torch_append(None, k, v, kc2, vc2, lens, None, cos, sin, kd, vd)}
    with torch.no_grad():
        fns["append"]()
        fns["torch"]()
        if not torch.equal(vc.view(torch.uint8), vc2.view(torch.uint8)):
            raise SystemExit("kvappend_bench: %s: the V caches of the two routes differ" % label)
        fns.update({n + "/g": graphed(f) for n, f in list(fns.items())})
        t = interleaved(fns, rounds, iters)
    own = 2 * B * N * Hkv * D * 2 + 2 * B * N * Hkv * D * (1 if fp8 else 2)
    print("%-12s B%d x %d tokens Hkv%d D%d %s -> %s: %.1f MB of its own (k, v read, cache rows written) = %.1f us at %.1f TB/s"
          % (label, B, N, Hkv, D, "bf16", "e4m3" if fp8 else "16-bit", own / 1e6, own / (HBM_TBS * 1e12) * 1e6, HBM_TBS))
    for n, base in (("append", "torch"), ("torch", None), ("append/g", "torch/g"), ("torch/g", None)):
        print(line(n, t, base) + ("  %.0f GB/s of its own bytes" % (own / (t[n][0] * 1e-3) / 1e9) if n.startswith("append") else ""))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", default="all", choices=("step", "chunk", "all"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kvappend_bench: needs a ROCm GPU (a timing taken anywhere else says nothing)")
    print(torch.cuda.get_device_name(0), "rounds", a.rounds, "iters", a.iters, "|", _fa2_lib.load().fa2_version().decode())
    if a.rows in ("step", "all"):
        for r in STEP_ROWS:
            step_row(*r, a.rounds, a.iters)
    if a.rows in ("chunk", "all"):
        for r in CHUNK_ROWS:
            chunk_row(*r, a.rounds, a.iters)


if __name__ == "__main__":
    main()
