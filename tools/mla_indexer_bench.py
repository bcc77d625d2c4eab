"""The lightning indexer of sparse MLA decode: mla_indexer_topk against what a user of flash_attention_decode_mla(indices=) wrote before it existed, same
box, interleaved rounds, median of per-round event times with the spread of the rounds beside it (tools/mla_sparse_bench.py's method).

    python tools/mla_indexer_bench.py [--rounds R] [--iters I] [--out FILE] [--only LABEL-PREFIX] [--fp8]

Routes
    indexer       mla_indexer_topk(q_idx, k_idx_cache, weights, lens, topk=2048): two launches
    indexer graph the same call captured once and replayed
    logits        mla_indexer_logits alone; its achieved bytes per second counts the VALID key bytes (sum of lens * 256) over its time
    select        topk_indices alone on those logits
    torch         the baseline: (a pool: gather the pages of each sequence through the block table) -> matmul -> relu -> weighted head sum -> length
                  mask built on the device -> torch.topk -> sort -> -1 fill.  It materialises [B, H_idx, Nkeys] scores.
A route is called faster only where the gap exceeds the sum of the two spreads.  Each row first checks the library's logits of sequence 0 against
float32 torch and its lists against torch.topk on the same logits (random logits have no tie at the threshold), and reports the overlap with the
baseline's lists, whose bf16 matmul rounds the scores."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))

import torch  # noqa: E402

from benchlib import graphed, interleaved, paged_pool  # noqa: E402
from rocwmma_fattn import _fa2_lib  # noqa: E402
from rocwmma_fattn.FlashAttn import (kvcache_append_mla_index, mla_index_cache_from_fp8, mla_index_cache_to_fp8, mla_indexer_logits,  # noqa: E402
                                     mla_indexer_topk, topk_indices)

H, D, TOPK, BF16 = 64, 128, 2048, torch.bfloat16
ROWS = [("%d_b%d_%dk%s" % (n, B, keys // 1024, "_pg64" if paged else ""), B, keys, paged)
        for n, B in enumerate((32, 1), 1) for keys in (4096, 32768, 65536) for paged in (False, True)]


def row(out, label, B, keys, paged, rounds, iters):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(1)
    q = torch.randn((B, 1, H, D), device=dev, dtype=BF16)
    k = torch.randn((B, keys, D), device=dev, dtype=BF16)
    w = torch.randn((B, 1, H), device=dev) * H ** -0.5
    lens = torch.full((B,), keys, dtype=torch.int32, device=dev)
    bt, cache = None, k
    if paged:
        cache, _, bt = paged_pool(k.unsqueeze(2), k.unsqueeze(2), 64, g)
        cache = cache[:, :, 0]
    pos = torch.arange(keys, device=dev).view(1, 1, keys)

    def baseline():
        kk = cache if bt is None else cache[bt.long()].view(B, keys, D)                    # the gathered copy a pool needs
        s = torch.relu(torch.matmul(q[:, 0], kk.transpose(1, 2)).float())                # [B, H, keys]
        logits = (s * w[:, 0, :, None]).sum(1, keepdim=True)
        logits = logits.masked_fill(pos >= lens.view(B, 1, 1), float("-inf"))
        top = torch.topk(logits, TOPK, dim=-1)
        idx = top.indices.masked_fill(top.values == float("-inf"), keys).sort(-1).values
        return idx.masked_fill(idx == keys, -1).to(torch.int32)

    logits = mla_indexer_logits(q, cache, w, lens, block_table=bt)
    fns = {"indexer": lambda: mla_indexer_topk(q, cache, w, lens, block_table=bt, topk=TOPK),
           "indexer graph": graphed(lambda: mla_indexer_topk(q, cache, w, lens, block_table=bt, topk=TOPK)),
           "logits": lambda: mla_indexer_logits(q, cache, w, lens, block_table=bt),
           "select": lambda: topk_indices(logits, lens, TOPK),
           "torch": baseline}
    with torch.no_grad():
        got, want = fns["indexer"](), baseline()
        ref0 = (torch.relu(q[0, 0].float() @ k[0].float().t()) * w[0, 0, :, None]).sum(0)
        if float((logits[0, 0] - ref0).abs().max()) > 1e-3:
            raise SystemExit("mla_indexer_bench: %s: the logits disagree with float32 torch (max |diff| %.3g)" % (label, float((logits[0, 0] - ref0).abs().max())))
        if not torch.equal(got.long(), torch.topk(logits, TOPK, dim=-1).indices.sort(-1).values):
            raise SystemExit("mla_indexer_bench: %s: the lists disagree with torch.topk on the same logits" % label)
        overlap = min(len(set(got[b, 0].tolist()) & set(want[b, 0].tolist())) for b in range(B))
        t = interleaved(fns, rounds, iters)
    lines = ["%-16s B%d Nq1 H_idx %d topk %d of %d keys bf16%s  (lists: torch.topk's on the same logits; least overlap with the bf16 baseline's %d of %d)"
             % (label, B, H, TOPK, keys, " pages of 64" if paged else "", overlap, TOPK)]
    i_med, i_lo, i_hi = t["indexer"]
    for n, (med, lo, hi) in t.items():
        rel = ""
        if n == "torch":
            real = abs(med - i_med) > (hi - lo) + (i_hi - i_lo)
            rel = "  indexer %.2fx %s (%s the sum of the spreads, %.1f us)" % (max(med / i_med, i_med / med), "faster" if i_med <= med else "SLOWER",
                                                                              "beyond" if real else "WITHIN", ((hi - lo) + (i_hi - i_lo)) * 1e3)
        if n == "logits":
            rel = "  %.2f TB/s of valid key bytes (%d MB)" % (B * keys * D * 2 / (med * 1e-3) / 1e12, B * keys * D * 2 >> 20)
        lines.append("    %-13s %9.1f us  (rounds %.1f .. %.1f, spread %.1f %%)%s" % (n, med * 1e3, lo * 1e3, hi * 1e3, 100.0 * (hi - lo) / med, rel))
    for line in lines:
        print(line)
        if out:
            out.write(line + "\n")
            out.flush()
    sys.stdout.flush()


def row8(out, label, B, keys, paged, rounds, iters):
    if paged:                                          # (the three layouts are one row here)
        return
    dev = torch.device("cuda", 0)
    q = torch.randn((B, 1, H, D), device=dev, dtype=BF16)
    k = torch.randn((B, keys, D), device=dev, dtype=BF16)
    w = torch.randn((B, 1, H), device=dev) * H ** -0.5
    lens = torch.full((B,), keys, dtype=torch.int32, device=dev)
    rows = mla_index_cache_to_fp8(k)
    pages = B * keys // 64
    perm = torch.randperm(pages, device=dev)
    pool = torch.empty((pages, 64, 132), dtype=torch.uint8, device=dev)
    pool[perm] = rows.view(pages, 64, 132)
    bt = perm.view(B, keys // 64).int()
    buf = torch.cat([pool[:, :, :128].reshape(pages, -1), pool[:, :, 128:].reshape(pages, -1)], 1).contiguous()
    blocks = (buf[:, :64 * 128].view(pages, 64, 128), buf[:, 64 * 128:].view(torch.float32))
    new, at = torch.randn((B, 1, D), device=dev, dtype=BF16), (torch.arange(B, device=dev), lens.long() - 1)
    caches = {"16-bit": (k, None), "e4m3 rows": (rows, None), "e4m3 rows pg64": (pool, bt), "e4m3 blocks pg64": (blocks, bt)}
    fns = {}
    for n, (c, t) in caches.items():
        fns[n] = lambda c=c, t=t: mla_indexer_topk(q, c, w, lens, block_table=t, topk=TOPK)
        fns[n + " logits"] = lambda c=c, t=t: mla_indexer_logits(q, c, w, lens, block_table=t)
    fns["dequant + 16-bit"] = lambda: mla_indexer_topk(q, mla_index_cache_from_fp8(rows, BF16), w, lens, topk=TOPK)
    fns["append"] = lambda: kvcache_append_mla_index(rows, new, lens)
    fns["append torch"] = lambda: rows.index_put_(at, mla_index_cache_to_fp8(new[:, 0]))
    with torch.no_grad():
        a = fns["e4m3 rows logits"]()
        if not all(torch.equal(a, fns[n + " logits"]()) for n in ("e4m3 rows pg64", "e4m3 blocks pg64")):
            raise SystemExit("mla_indexer_bench: %s: the e4m3 layouts disagree" % label)
        t = interleaved(fns, rounds, iters)
    lines = ["%-12s B%d Nq1 H_idx %d topk %d of %d keys, bf16 q" % (label, B, H, TOPK, keys)]
    for n, (med, lo, hi) in t.items():
        rel = ""
        base = t.get("16-bit logits" if n.endswith("logits") else "16-bit")
        if n.endswith("logits"):
            per = 256 if n.startswith("16") else 132
            rel = "  %.2f TB/s of valid key bytes (%d MB)" % (B * keys * per / (med * 1e-3) / 1e12, B * keys * per >> 20)
        if n.startswith("e4m3") or n.startswith("dequant"):
            real = abs(med - base[0]) > (hi - lo) + (base[2] - base[1])
            rel += "  %.2fx the 16-bit time (%s the sum of the spreads)" % (med / base[0], "beyond" if real else "WITHIN")
        lines.append("    %-24s %9.1f us  (rounds %.1f .. %.1f, spread %.1f %%)%s" % (n, med * 1e3, lo * 1e3, hi * 1e3, 100.0 * (hi - lo) / med, rel))
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
    ap.add_argument("--fp8", action="store_true", help="the e4m3 index-key cache rows (section 35) instead of the 16-bit ones")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mla_indexer_bench: needs a ROCm GPU (a timing taken anywhere else says nothing)")
    out = open(a.out, "w") if a.out else None
    head = "%s (%d CUs) rounds %d iters %d | %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, a.rounds, a.iters,
                                                   _fa2_lib.load().fa2_version().decode())
    print(head)
    if out:
        out.write(head + "\n")
    for r in ROWS:
        if r[0].startswith(a.only):
            (row8 if a.fp8 else row)(out, *r, a.rounds, a.iters)


if __name__ == "__main__":
    main()
