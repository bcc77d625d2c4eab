"""One MLA serving step — write the new tokens' latent rows (kv_c + rotated k_pe), rotate the tail of q, decode on the latent cache — through the
library's append launch against the route a caller had before it, same box, interleaved rounds, median of per-round event times with the spread of the
rounds beside it (tools/kvappend_bench.py's protocol: 9 rounds of 20 calls, spread = (max - min) / median; a gap counts only beyond the sum of the
two spreads).

    python tools/mla_append_bench.py [--rounds R] [--iters I] [--rows step|packed|all]

Step rows (cache_seqlens counts the new tokens; every sequence has `keys` keys after the append):
    fused        flash_attention_decode_mla(q, ..., kv_c=, k_pe=, rotary_cos=, rotary_sin=): the append launch, then the decode call on the rotated q
    torch        the route before: torch ops compute the positions (and page slots) from the device tensors, gather the table rows, rotate k_pe and
                 the tail of q, cat the row and index_put_ it into the cache, then flash_attention_decode_mla — no host read either
    append       kvcache_append_mla(..., q=q) alone
    decode       flash_attention_decode_mla on an already appended cache alone: fused - decode is what the append adds
Each of the four is timed eagerly and, with a "/g" suffix, as a replayed graph.  fused and torch are first checked against each other on the timed
inputs (caches and outputs within fp16 1e-3 + 2e-3 |x|, bf16 8e-3 + 1.6e-2 |x|).  The append lines carry the GB/s of the valid bytes: the latent rows
read and written, the q rows both ways, the table rows (1 GB/s is 1 000 bytes per microsecond).
Packed row: a continuous-batching step of 24 single-token rows and 4 chunks of 384 tokens: kvcache_append_mla_varlen (one launch) against a loop of
per-sequence kvcache_append_mla calls (28 launches), eager and replayed."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))

import torch  # noqa: E402

from benchlib import close, graphed, interleaved, paged_pool  # noqa: E402
from rocwmma_fattn import _fa2_lib  # noqa: E402
from rocwmma_fattn.FlashAttn import flash_attention_decode_mla, kvcache_append_mla, kvcache_append_mla_varlen  # noqa: E402

D, DV, ROT = 576, 512, 64
STEP_ROWS = [  # (label, B, H, Nq, keys, page)
    ("b32_h128", 32, 128, 1, 4096, 0),
    ("b32_h16", 32, 16, 1, 4096, 0),
    ("b1_h128_8k", 1, 128, 1, 8192, 0),
    ("b32_h128_pg64", 32, 128, 1, 4096, 64),
]
PACKED_COUNTS = [1] * 24 + [384] * 4


def tables(n, dev):
    inv = 10000.0 ** (-torch.arange(0, ROT, 2, dtype=torch.float64) / ROT)
    ang = torch.arange(n, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().float().to(dev), ang.sin().float().to(dev)


def rotate(x, cos, sin):
    """GPT-J pairing, f32 arithmetic: x [..., 64], cos / sin broadcastable [..., 32] -> f32"""
    x = x.float()
    x1, x2 = x[..., 0::2], x[..., 1::2]
    return torch.stack((x1 * cos - x2 * sin, x1 * sin + x2 * cos), dim=-1).flatten(-2)


def torch_append(q, kv_c, k_pe, cache, lens, bt, cos, sin):
    """The route before the append launch: positions, page slots, rotation, cat and the cache write as torch ops on device tensors -> the rotated q"""
    B, N = kv_c.shape[:2]
    pos = lens.long()[:, None] - N + torch.arange(N, device=kv_c.device)[None, :]
    rows = pos.clamp(0, cos.shape[0] - 1)
    c, s = cos[rows], sin[rows]
    row = torch.cat((kv_c, rotate(k_pe, c, s).to(kv_c.dtype)), dim=-1)
    q_rot = torch.cat((q[..., :DV], rotate(q[..., DV:], c[:, :, None, :], s[:, :, None, :]).to(q.dtype)), dim=-1)
    if bt is None:
        idx = (torch.arange(B, device=kv_c.device)[:, None].expand(B, N), pos)
    else:
        page = cache.shape[1]
        idx = (bt.gather(1, pos // page).long(), pos % page)
    cache.index_put_(idx, row)
    return q_rot


def line(name, t, base=None, extra=""):
    med, lo, hi = t[name]
    rel = ""
    if base is not None and name != base:
        b_med, b_lo, b_hi = t[base]
        real = abs(b_med - med) > (hi - lo) + (b_hi - b_lo)          # the project's rule: a difference beyond the sum of the two spreads
        rel = "  %+.1f us against %s, %.2fx %s (%s the sum of the spreads, %.1f us)" % ((med - b_med) * 1e3, base, max(b_med / med, med / b_med),
                                                                                       "faster" if med <= b_med else "slower", "beyond" if real else "WITHIN",
                                                                                       ((hi - lo) + (b_hi - b_lo)) * 1e3)
    return "    %-10s %9.1f us  (rounds %.1f .. %.1f, spread %.1f %%)%s%s" % (name, med * 1e3, lo * 1e3, hi * 1e3, 100.0 * (hi - lo) / med, rel, extra)


def step_row(label, B, H, Nq, keys, page, rounds, iters):
    dev, dt = torch.device("cuda", 0), torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(4)
    nmax = keys + 256
    q = torch.randn((B, Nq, H, D), device=dev, dtype=dt)
    proj = torch.randn((B, Nq, D), device=dev, dtype=dt)             # one projection output: kv_c and k_pe are its two slices, never copied
    kv_c, k_pe = proj[..., :DV], proj[..., DV:]
    cache = torch.randn((B, nmax, D), device=dev, dtype=dt)
    bt = None
    if page:
        pool, _, bt = paged_pool(cache.unsqueeze(2), cache.unsqueeze(2), page, g)
        cache = pool[:, :, 0]
    lens = torch.full((B,), keys, dtype=torch.int32, device=dev)
    cos, sin = tables(nmax, dev)
    cache2 = cache.clone()                                           # the torch route's own cache

    def fused():
        return flash_attention_decode_mla(q, cache, lens, block_table=bt, kv_c=kv_c, k_pe=k_pe, rotary_cos=cos, rotary_sin=sin)

    def torch_route():
        return flash_attention_decode_mla(torch_append(q, kv_c, k_pe, cache2, lens, bt, cos, sin), cache2, lens, block_table=bt)

    def append():
        return kvcache_append_mla(cache, kv_c, k_pe, lens, block_table=bt, rotary_cos=cos, rotary_sin=sin, q=q)

    def decode():
        return flash_attention_decode_mla(q, cache, lens, block_table=bt)

    with torch.no_grad():
        close("mla_append_bench", fused(), torch_route(), dt, label + ": fused and torch outputs")
        close("mla_append_bench", cache, cache2, dt, label + ": the caches")
        fns = {"fused": fused, "torch": torch_route, "append": append, "decode": decode}
        fns.update({n + "/g": graphed(f) for n, f in list(fns.items())})
        t = interleaved(fns, rounds, iters)
    own = B * Nq * (2 * D * 2 + 2 * H * D * 2 + 2 * (ROT // 2) * 4)
    print("%-14s B%d H%d Nq%d keys %d bf16 %s: %.2f MB valid bytes in the append (latent rows in and out, q rows both ways, table rows)"
          % (label, B, H, Nq, keys, "pages of %d" % page if page else "contiguous", own / 1e6))
    for sfx in ("", "/g"):
        print(line("fused" + sfx, t, "decode" + sfx))
        print(line("fused" + sfx, t, "torch" + sfx))
        print(line("torch" + sfx, t, "decode" + sfx))
        print(line("append" + sfx, t, None, "  %.0f GB/s of its valid bytes" % (own / (t["append" + sfx][0] * 1e-3) / 1e9)))
        print(line("decode" + sfx, t))
    sys.stdout.flush()


def packed_row(rounds, iters):
    dev, dt, H, keys = torch.device("cuda", 0), torch.bfloat16, 16, 4096
    counts = PACKED_COUNTS
    B, total, nmax = len(counts), sum(counts), keys + 256
    cu_host = [0]
    for c in counts:
        cu_host.append(cu_host[-1] + c)
    cu = torch.tensor(cu_host, dtype=torch.int32, device=dev)
    proj = torch.randn((total, D), device=dev, dtype=dt)
    kv_c, k_pe = proj[:, :DV], proj[:, DV:]
    q = torch.randn((total, H, D), device=dev, dtype=dt)
    cache, cache2 = (torch.zeros((B, nmax, D), device=dev, dtype=dt) for _ in range(2))
    lens = torch.tensor([keys if c == 1 else 2048 for c in counts], dtype=torch.int32, device=dev)
    cos, sin = tables(nmax, dev)
    parts = [(cache2[s:s + 1], kv_c[cu_host[s]:cu_host[s + 1]][None], k_pe[cu_host[s]:cu_host[s + 1]][None], lens[s:s + 1], q[cu_host[s]:cu_host[s + 1]][None])
             for s in range(B)]

    def packed():
        return kvcache_append_mla_varlen(cache, kv_c, k_pe, cu, lens, rotary_cos=cos, rotary_sin=sin, q=q)

    def loop():
        return [kvcache_append_mla(c, a, b, n, rotary_cos=cos, rotary_sin=sin, q=qq) for c, a, b, n, qq in parts]

    with torch.no_grad():
        qa, qb = packed(), torch.cat([x[0] for x in loop()])
        if not torch.equal(cache.view(torch.int16), cache2.view(torch.int16)) or not torch.equal(qa.view(torch.int16), qb.view(torch.int16)):
            raise SystemExit("mla_append_bench: the packed call and the loop of uniform calls differ")
        fns = {"packed": packed, "loop": loop}
        fns.update({n + "/g": graphed(f) for n, f in list(fns.items())})
        t = interleaved(fns, rounds, iters)
    own = total * (2 * D * 2 + 2 * H * D * 2 + 2 * (ROT // 2) * 4)
    print("%-14s 24 single-token rows + 4 chunks of 384 (%d tokens, %d sequences) H%d bf16 contiguous: %.2f MB valid bytes" % ("packed_step", total, B, H, own / 1e6))
    for sfx in ("", "/g"):
        print(line("packed" + sfx, t, "loop" + sfx, "  %.0f GB/s of its valid bytes" % (own / (t["packed" + sfx][0] * 1e-3) / 1e9)))
        print(line("loop" + sfx, t))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", default="all", choices=("step", "packed", "all"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mla_append_bench: needs a ROCm GPU (a timing taken anywhere else says nothing)")
    print(torch.cuda.get_device_name(0), "rounds", a.rounds, "iters", a.iters, "|", _fa2_lib.load().fa2_version().decode())
    if a.rows in ("step", "all"):
        for r in STEP_ROWS:
            step_row(*r, a.rounds, a.iters)
    if a.rows in ("packed", "all"):
        packed_row(a.rounds, a.iters)


if __name__ == "__main__":
    main()
