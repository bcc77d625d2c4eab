"""Sparse (top-k indexed) decode attention on a latent (MLA) KV cache: flash_attention_decode_mla(indices=) against the routes a holder of such a cache
had before, same box, interleaved rounds, median of per-round event times with the spread of the rounds beside it (tools/mla_decode_bench.py's method).

    python tools/mla_sparse_bench.py [--rounds R] [--iters I] [--out FILE] [--only LABEL-PREFIX] [--fp8]

Routes
    sparse        flash_attention_decode_mla(q, cache, lens, indices=idx): the selected rows read in place
    gather+dense  (a) index_select of the selected rows into a contiguous [B * Nq, topk, 576] copy (through the block table where the cache is paged),
                  then the dense call on the copy, the copy INSIDE the timed region: the same computation
    dense-all     (b) the dense call over the whole cache: a DIFFERENT computation (it attends every key), shown for scale only
Every row prints (c) the floor: B * Nq * topk * 1 152 bytes at 6.3 TB/s.  A route is called faster only where the gap exceeds the sum of the two
spreads.  Each row first checks sparse against gather+dense on the timed inputs.  The lists hold topk distinct positions of each sequence, drawn
uniformly and sorted, as an indexer's top-k is.
--fp8: the contiguous H128 / H16 rows at 4 K and 64 K keys on an e4m3 latent cache of 656-byte rows instead, three routes:
    sparse        (a) the 16-bit sparse call on the 16-bit cache of the same shape
    deq+sparse    (b) mla_cache_from_fp8 over the live rows, then the 16-bit sparse call: what a holder of an e4m3 cache ran before
    sparse_fp8    (c) the sparse call on the e4m3 cache itself (checked bit for bit against (b) first)
and the floor B * topk * 656 bytes at 6.3 TB/s.
--packed: the packed (prefill) call, flash_attention_prefill_mla, at topk 2 048 over 32 K keys, H128 / H16, bf16 and e4m3 caches:
    chunk         one sequence's chunk of 2 048 tokens;  ragged: 28 decode rows and 4 chunks of 505 tokens in one buffer of 2 048
    per-token     32 sequences of one token each: the shape of section 31's B32 row, for the time per (token, head block)
    packed        the one call;  host-loop: flash_attention_decode_mla(indices=, num_splits=0) per sequence in calls of Nq * H <= 512 rows, which
                  is what a caller had before (checked bit for bit against packed under num_splits=1 first)
A token's list is its sequence's 2 048 sorted random positions with the last min(i, 256) of them replaced by the newest positions below its own:
neighbouring tokens share most of their rows, as an indexer's lists do."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))

import torch  # noqa: E402

from benchlib import close, interleaved, paged_pool  # noqa: E402
from rocwmma_fattn import _fa2_lib  # noqa: E402
from rocwmma_fattn.FlashAttn import flash_attention_decode_mla, flash_attention_prefill_mla, mla_cache_from_fp8, mla_cache_to_fp8  # noqa: E402

HBM_TBS = 6.3
D, TOPK, BF16 = 576, 2048, torch.bfloat16
ROWS = [(("%d_b%d_h%d_%dk%s" % (n, B, H, keys // 1024, "_pg64" if paged else "")), B, H, keys, paged)      # (label, B, H, keys or (shortest, longest), paged)
        for n, (B, H) in enumerate(((32, 128), (32, 16)), 1) for keys in (4096, 32768, 65536) for paged in (False, True)]
ROWS.append(("3_ragged_b32_h128_pg64", 32, 128, (2048, 65536), True))


def row(out, label, B, H, keys, paged, rounds, iters):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(1)
    lens_h = torch.randint(keys[0], keys[1] + 1, (B,), generator=g).tolist() if isinstance(keys, tuple) else [keys] * B
    nmax = -(-max(lens_h) // 64) * 64
    q = torch.randn((B, 1, H, D), device=dev, dtype=BF16)
    kv = torch.randn((B, nmax, D), device=dev, dtype=BF16)
    lens = torch.tensor(lens_h, dtype=torch.int32, device=dev)
    idx = torch.stack([torch.randperm(n, generator=g)[:TOPK].sort().values for n in lens_h]).to(torch.int32).view(B, 1, TOPK).to(dev)
    full = torch.full((B,), TOPK, dtype=torch.int32, device=dev)
    if paged:
        pool, _, bt = paged_pool(kv.unsqueeze(2), kv.unsqueeze(2), 64, g, lens=lens_h)
        pool = pool[:, :, 0]
        flat = pool.view(-1, D)

        def rows_of():                                 # logical -> physical rows, then the copy
            j = idx.view(B, TOPK).long()
            return flat.index_select(0, (bt.long().gather(1, j // 64) * 64 + j % 64).view(-1)).view(B, TOPK, D)
        fns = {"sparse": lambda: flash_attention_decode_mla(q, pool, lens, block_table=bt, indices=idx),
               "gather+dense": lambda: flash_attention_decode_mla(q, rows_of(), full),
               "dense-all": lambda: flash_attention_decode_mla(q, pool, lens, block_table=bt)}
    else:
        flat = kv.view(-1, D)
        base = (torch.arange(B, device=dev) * nmax).view(B, 1)
        fns = {"sparse": lambda: flash_attention_decode_mla(q, kv, lens, indices=idx),
               "gather+dense": lambda: flash_attention_decode_mla(q, flat.index_select(0, (base + idx.view(B, TOPK)).view(-1)).view(B, TOPK, D), full),
               "dense-all": lambda: flash_attention_decode_mla(q, kv, lens)}
    with torch.no_grad():
        close("mla_sparse_bench", fns["sparse"](), fns["gather+dense"](), BF16, label + ": sparse and gather+dense")
        t = interleaved(fns, rounds, iters)
    plan = _fa2_lib.decode_mla_sparse_plan(1, B, H, 1, bt.shape[1] if paged else nmax, TOPK, 64 if paged else 0)
    floor_us = B * TOPK * D * 2 / (HBM_TBS * 1e12) * 1e6
    shape = "B%d H%d Nq1 topk %d of %s keys bf16%s (split %d)" % (
        B, H, TOPK, keys if not isinstance(keys, tuple) else "%d .. %d (mean %d)" % (min(lens_h), max(lens_h), sum(lens_h) // B), " pages of 64" if paged else "",
        plan.nsplit)
    lines = ["%-24s %s  floor %.1f us at %.1f TB/s" % (label, shape, floor_us, HBM_TBS)]
    s_med, s_lo, s_hi = t["sparse"]
    for n, (med, lo, hi) in t.items():
        rel = ""
        if n != "sparse":
            real = abs(med - s_med) > (hi - lo) + (s_hi - s_lo)
            rel = "  sparse %.2fx %s (%s the sum of the spreads, %.1f us)%s" % (
                max(med / s_med, s_med / med), "faster" if s_med <= med else "SLOWER", "beyond" if real else "WITHIN", ((hi - lo) + (s_hi - s_lo)) * 1e3,
                "  [a different computation: every key]" if n == "dense-all" else "")
        lines.append("    %-13s %9.1f us  (rounds %.1f .. %.1f, spread %.1f %%)  %.1f x the floor%s" % (n, med * 1e3, lo * 1e3, hi * 1e3, 100.0 * (hi - lo) / med,
                                                                                                   med * 1e3 / floor_us, rel))
    for line in lines:
        print(line)
        if out:
            out.write(line + "\n")
            out.flush()
    sys.stdout.flush()


def row_fp8(out, label, B, H, keys, rounds, iters):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(1)
    q = torch.randn((B, 1, H, D), device=dev, dtype=BF16)
    kv = torch.randn((B, keys, D), device=dev, dtype=BF16)
    lens = torch.full((B,), keys, dtype=torch.int32, device=dev)
    idx = torch.stack([torch.randperm(keys, generator=g)[:TOPK].sort().values for _ in range(B)]).to(torch.int32).view(B, 1, TOPK).to(dev)
    c8 = mla_cache_to_fp8(kv)
    fns = {"sparse": lambda: flash_attention_decode_mla(q, kv, lens, indices=idx),
           "deq+sparse": lambda: flash_attention_decode_mla(q, mla_cache_from_fp8(c8, BF16), lens, indices=idx),
           "sparse_fp8": lambda: flash_attention_decode_mla(q, c8, lens, indices=idx)}
    with torch.no_grad():
        assert torch.equal(fns["sparse_fp8"]().view(torch.int16), fns["deq+sparse"]().view(torch.int16)), label + ": the e4m3 call against the dequantised cache"
        t = interleaved(fns, rounds, iters)
    floor_us = B * TOPK * 656 / (HBM_TBS * 1e12) * 1e6
    lines = ["%-24s B%d H%d Nq1 topk %d of %d keys bf16, e4m3 cache  floor %.1f us at %.1f TB/s" % (label, B, H, TOPK, keys, floor_us, HBM_TBS)]
    c_med, c_lo, c_hi = t["sparse_fp8"]
    for n, (med, lo, hi) in t.items():
        rel = ""
        if n != "sparse_fp8":
            real = abs(med - c_med) > (hi - lo) + (c_hi - c_lo)
            rel = "  sparse_fp8 %.2fx %s (%s the sum of the spreads, %.1f us)" % (max(med / c_med, c_med / med), "faster" if c_med <= med else "SLOWER",
                                                                                 "beyond" if real else "WITHIN", ((hi - lo) + (c_hi - c_lo)) * 1e3)
        lines.append("    %-13s %9.1f us  (rounds %.1f .. %.1f, spread %.1f us)%s" % (n, med * 1e3, lo * 1e3, hi * 1e3, (hi - lo) * 1e3, rel))
    for line in lines:
        print(line)
        if out:
            out.write(line + "\n")
            out.flush()
    sys.stdout.flush()


PACKED = [("%s_h%d_%s" % (kind, H, "e4m3" if fp8 else "bf16"), kind, H, fp8) for kind in ("chunk", "ragged", "per-token") for H in (128, 16) for fp8 in (False, True)]


def row_packed(out, label, kind, H, fp8, rounds, iters):
    dev, keys = torch.device("cuda", 0), 32768
    g = torch.Generator(device="cpu").manual_seed(1)
    counts = {"chunk": [2048], "ragged": [1] * 28 + [505] * 4, "per-token": [1] * 32}[kind]
    B, total = len(counts), sum(counts)
    q = torch.randn((total, H, D), device=dev, dtype=BF16)
    kv = torch.randn((B, keys, D), device=dev, dtype=BF16)
    cache = mla_cache_to_fp8(kv) if fp8 else kv
    lens = torch.full((B,), keys, dtype=torch.int32, device=dev)
    cu_h = [sum(counts[:s]) for s in range(B + 1)]
    cu = torch.tensor(cu_h, dtype=torch.int32, device=dev)
    idx = torch.empty((total, TOPK), dtype=torch.int32)
    for s, n in enumerate(counts):
        base = torch.randperm(keys - n, generator=g)[:TOPK].sort().values
        for i in range(n):
            r, pos = min(i, 256), keys - n + i
            idx[cu_h[s] + i] = torch.cat([base[:TOPK - r], torch.arange(pos - r + 1, pos + 1)])
    idx = idx.to(dev)

    def host_loop(num_splits=0):
        outs = []
        for s, n in enumerate(counts):
            for a in range(0, n, 512 // H):
                b = min(n, a + 512 // H)
                outs.append(flash_attention_decode_mla(q[None, cu_h[s] + a:cu_h[s] + b], cache[s:s + 1], lens[s:s + 1] - (n - b), num_splits=num_splits,
                                                       indices=idx[None, cu_h[s] + a:cu_h[s] + b])[0])
        return torch.cat(outs)
    fns = {"packed": lambda: flash_attention_prefill_mla(q, cache, cu, lens, idx), "host-loop": host_loop}
    if kind == "per-token":                            # the decode call on the same 32 rows, under its own plan (it splits the list over idle CUs)
        fns["decode-b32"] = lambda: flash_attention_decode_mla(q.view(B, 1, H, D), cache, lens, indices=idx.view(B, 1, TOPK))
    with torch.no_grad():
        assert torch.equal(fns["packed"]().view(torch.int16), host_loop(1).view(torch.int16)), label + ": packed against the host loop, bit for bit"
        t = interleaved(fns, rounds, iters)
    blocks = total * -(-H // 64)
    lines = ["%-22s %d tokens in %d sequences, H%d, topk %d of %d keys, %s cache: %d (token, head block) items, %d calls in the host loop"
             % (label, total, B, H, TOPK, keys, "e4m3" if fp8 else "bf16", blocks, sum(-(-n // (512 // H)) for n in counts))]
    p_med, p_lo, p_hi = t["packed"]
    for n, (med, lo, hi) in t.items():
        rel = "  %.2f us per item" % (med * 1e3 / blocks)
        if n != "packed":
            rel += "  packed %.2fx %s (%s the sum of the spreads, %.1f us)" % (max(med / p_med, p_med / med), "faster" if p_med <= med else "SLOWER",
                                                                            "beyond" if abs(med - p_med) > (hi - lo) + (p_hi - p_lo) else "WITHIN",
                                                                            ((hi - lo) + (p_hi - p_lo)) * 1e3)
        lines.append("    %-13s %10.1f us  (rounds %.1f .. %.1f, spread %.1f us)%s" % (n, med * 1e3, lo * 1e3, hi * 1e3, (hi - lo) * 1e3, rel))
    for line in lines:
        print(line)
        if out:
            out.write(line + "\n")
            out.flush()
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--only", default="", help="rows whose label starts with this")
    ap.add_argument("--fp8", action="store_true", help="H128 / H16 at 4 K and 64 K keys on an e4m3 cache: 16-bit, dequantise-then-call and the e4m3 call")
    ap.add_argument("--packed", action="store_true", help="flash_attention_prefill_mla against the host loop of sparse decode calls: chunk, ragged, per-token")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mla_sparse_bench: needs a ROCm GPU (a timing taken anywhere else says nothing)")
    out = open(a.out, "w") if a.out else None
    head = "%s (%d CUs) rounds %d iters %d | %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, a.rounds, a.iters,
                                                   _fa2_lib.load().fa2_version().decode())
    print(head)
    if out:
        out.write(head + "\n")
    for r in PACKED if a.packed else ():
        if r[0].startswith(a.only):
            row_packed(out, *r, a.rounds, a.iters)
    for r in () if a.packed else ROWS:
        if a.fp8:
            if not r[4] and r[3] in (4096, 65536) and r[0].startswith(a.only):
                row_fp8(out, *r[:4], a.rounds, a.iters)
        elif r[0].startswith(a.only):
            row(out, *r, a.rounds, a.iters)


if __name__ == "__main__":
    main()
