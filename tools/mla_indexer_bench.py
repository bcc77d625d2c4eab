"""The lightning indexer of sparse MLA decode: mla_indexer_topk against what a user of flash_attention_decode_mla(indices=) wrote before it existed, same
box, interleaved rounds, median of per-round event times with the spread of the rounds beside it (tools/mla_sparse_bench.py's method).

    python tools/mla_indexer_bench.py [--rounds R] [--iters I] [--out FILE] [--only LABEL-PREFIX] [--fp8 | --prefill]

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
                                     mla_indexer_logits_varlen, mla_indexer_q_to_fp8, mla_indexer_topk, mla_indexer_topk_varlen, topk_indices)

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


# --prefill (section 36): (label, token counts per sequence, keys per sequence).  The packed operators against what a caller does without them: one
# uniform call with Nq = the chunk where the batch is uniform, the host loop over sequences where it is ragged.
PREFILL = [("1_b1_2048_8k", (2048,), 8192), ("2_b1_2048_32k", (2048,), 32768), ("3_b1_2048_64k", (2048,), 65536), ("4_b4_512_32k", (512,) * 4, 32768),
           ("5_ragged_24x1_4x384_32k", (1,) * 24 + (384,) * 4, 32768)]
CLOCK_GHZ, MFMA_CYCLES, HBM_TBS = 2.4, 32, 8.0      # the floors' assumptions: peak clock, 8 passes of 4 cycles per 16x16x128 FP8 MFMA, peak HBM rate


def row_prefill(out, label, counts, keys, rounds, iters):
    dev, B, total = torch.device("cuda", 0), len(counts), sum(counts)
    uniform = len(set(counts)) == 1
    q = torch.randn((total, H, D), device=dev, dtype=BF16)
    w = torch.randn((total, H), device=dev) * H ** -0.5
    q8, w8 = (t[0] for t in mla_indexer_q_to_fp8(q[None], w[None]))
    rows = mla_index_cache_to_fp8(torch.randn((B, keys, D), device=dev, dtype=BF16))
    lens = torch.full((B,), keys, dtype=torch.int32, device=dev)
    cu_host = [0]
    for c in counts:
        cu_host.append(cu_host[-1] + c)
    cu = torch.tensor(cu_host, dtype=torch.int32, device=dev)
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def parent(qq, ww, f):
        if uniform:
            return [f(qq.view(B, counts[0], H, D), rows, ww.view(B, counts[0], H), lens)]
        return [f(qq[a:b][None], rows[s:s + 1], ww[a:b][None], lens[s:s + 1]) for s, (a, b) in enumerate(zip(cu_host, cu_host[1:]))]

    fns = {}
    for n, (qq, ww) in (("bf16 q", (q, w)), ("e4m3 q", (q8, w8))):
        fns[n + " logits packed"] = lambda qq=qq, ww=ww: mla_indexer_logits_varlen(qq, rows, ww, cu, lens)
        fns[n + " logits parent"] = lambda qq=qq, ww=ww: parent(qq, ww, mla_indexer_logits)
        fns[n + " step packed"] = lambda qq=qq, ww=ww: mla_indexer_topk_varlen(qq, rows, ww, cu, lens, topk=TOPK)
        fns[n + " step parent"] = lambda qq=qq, ww=ww: parent(qq, ww, lambda *a: mla_indexer_topk(*a, topk=TOPK))
    with torch.no_grad():
        for n in ("bf16 q", "e4m3 q"):
            a, b = fns[n + " logits packed"](), torch.cat([t.flatten(0, 1) for t in fns[n + " logits parent"]()])
            c, d = fns[n + " step packed"](), torch.cat([t.flatten(0, 1) for t in fns[n + " step parent"]()])
            if not torch.equal(a.view(torch.int32), b.view(torch.int32)) or not torch.equal(c, d):
                raise SystemExit("mla_indexer_bench: %s: %s: the packed call disagrees with the parent's calls" % (label, n))
        t = interleaved(fns, rounds, iters)
    # the causal triangle: token i of a chunk of c sees keys - c + i + 1 keys; an MFMA serves 16 heads x 16 keys
    mfmas = sum(sum(-(-(keys - c + i + 1) // 16) for i in range(c)) for c in counts) * (H // 16)
    f_mfma, f_write = mfmas * MFMA_CYCLES / (cus * 4) / (CLOCK_GHZ * 1e3), total * keys * 4 / (HBM_TBS * 1e6)      # us
    lines = ["%-24s B%d, %d packed tokens, %d keys per sequence, H_idx %d topk %d, e4m3 rows; packed == parent bit for bit" % (label, B, total, keys, H, TOPK),
             "    floors for the logits: MFMA issue %.1f us (%d MFMAs, %d cycles each, %d SIMDs, %.1f GHz), output write %.1f us (%d MB at %.0f TB/s)"
             % (f_mfma, mfmas, MFMA_CYCLES, cus * 4, CLOCK_GHZ, f_write, total * keys * 4 >> 20, HBM_TBS)]
    for n, (med, lo, hi) in t.items():
        rel = ""
        if n.endswith("packed"):
            base = t[n[:-6] + "parent"]
            real = abs(med - base[0]) > (hi - lo) + (base[2] - base[1])
            rel = "  %.2fx the parent's time (%s the sum of the spreads)" % (med / base[0], "beyond" if real else "WITHIN")
            if "logits" in n:
                rel += "; %.2f of the MFMA floor's rate, %.2f of the write floor's" % (f_mfma / (med * 1e3), f_write / (med * 1e3))
        lines.append("    %-22s %10.1f us  (rounds %.1f .. %.1f, spread %.1f %%)%s" % (n, med * 1e3, lo * 1e3, hi * 1e3, 100.0 * (hi - lo) / med, rel))
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
    ap.add_argument("--prefill", action="store_true", help="the packed (prefill) indexer against the parent's calls (section 36)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mla_indexer_bench: needs a ROCm GPU (a timing taken anywhere else says nothing)")
    out = open(a.out, "w") if a.out else None
    head = "%s (%d CUs) rounds %d iters %d | %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, a.rounds, a.iters,
                                                   _fa2_lib.load().fa2_version().decode())
    print(head)
    if out:
        out.write(head + "\n")
    for r in PREFILL if a.prefill else ROWS:
        if r[0].startswith(a.only):
            (row_prefill if a.prefill else row8 if a.fp8 else row)(out, *r, a.rounds, a.iters)


if __name__ == "__main__":
    main()
