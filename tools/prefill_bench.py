"""Chunked prefill against a KV cache (flash_attention_prefill) against what a user had to do before it existed.

    python tools/prefill_bench.py [--rounds 9] [--iters 10] [--out profiles/rNN_prefill_bench.txt]

Per row three routes, timed round-robin on one device (tools/benchlib.py: interleaved rounds, median, spread = (max - min) / median):
    prefill          flash_attention_prefill on the cache as it lies (contiguous, or pages under a shuffled block table)
    varlen           flash_attention_varlen(causal=True, bottom_right=True) on a PRE-gathered packed copy of the keys: the same useful work, so the
                     difference prices the paging itself (one scalar load and one descriptor per 64-key tile)
    gather+varlen    index_select of the valid rows out of the cache (the row index built beforehand, on the host, from lengths and table — which is
                     what breaks graph capture) and then that call: what a user does today
Shapes: H32 Hkv8 D128 bf16 (the first row also fp16).  The outputs of the three routes are compared before anything is timed."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchlib  # noqa: E402
from rocwmma_fattn.FlashAttn import flash_attention_prefill, flash_attention_varlen  # noqa: E402

H, HKV, D = 32, 8, 128


def case(name, lens, nqs, page, dtype, window, g, dev):
    B, nmax = len(lens), -(-max(lens) // 256) * 256
    kc = torch.randn((B, nmax, HKV, D), generator=g).to(dtype).to(dev)
    vc = torch.randn((B, nmax, HKV, D), generator=g).to(dtype).to(dev)
    q = torch.randn((sum(nqs), H, D), generator=g).to(dtype).to(dev)
    cu_q = torch.tensor([0] + torch.tensor(nqs).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    cu_k = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    if page:
        pk, pv, bt = benchlib.paged_pool(kc, vc, page, g, lens=lens)
        btc = bt.cpu().long()
        rows = torch.cat([btc[b][torch.arange(n) // page] * page + torch.arange(n) % page for b, n in enumerate(lens)]).to(dev)
    else:
        pk, pv, bt = kc, vc, None
        rows = torch.cat([b * nmax + torch.arange(n) for b, n in enumerate(lens)]).to(dev)
    flat_k, flat_v = pk.view(-1, HKV, D), pv.view(-1, HKV, D)
    kp, vp = flat_k.index_select(0, rows), flat_v.index_select(0, rows)
    mq, mk, w = max(nqs), max(lens), (window, 0) if window >= 0 else None

    def prefill():
        return flash_attention_prefill(q, pk, pv, cu_q, lens_d, bt, max_seqlen_q=mq, window=w)

    def varlen():
        return flash_attention_varlen(q, kp, vp, cu_q, cu_k, mq, mk, causal=True, bottom_right=True, window=w)

    def gather_varlen():
        return flash_attention_varlen(q, flat_k.index_select(0, rows), flat_v.index_select(0, rows), cu_q, cu_k, mq, mk, causal=True, bottom_right=True, window=w)

    with torch.no_grad():
        a, b, c = prefill(), varlen(), gather_varlen()
    if not (torch.equal(a, b) and torch.equal(a, c)):
        benchlib.close("prefill_bench", a, b, dtype, name)
    return name, {"prefill": prefill, "varlen": varlen, "gather+varlen": gather_varlen}, bool(torch.equal(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    bf, f16 = torch.bfloat16, torch.float16
    ragged_lens = [592 + (7947 - 592) * i // 27 for i in range(28)]
    ragged_nqs = [384 if i % 7 == 3 else 1 for i in range(28)]
    specs = []
    for dt in (bf, f16):
        for page in (0, 64, 256):
            specs.append(("chunk 512 on 8192 keys B4 %s %s" % ("contiguous" if not page else "pages of %d" % page, str(dt)[6:]), [8192] * 4, [512] * 4, page, dt, -1))
    for page in (0, 64):
        specs.append(("prefix hit 3072 + 1024 new B8 %s bf16" % ("contiguous" if not page else "pages of %d" % page), [4096] * 8, [1024] * 8, page, bf, -1))
    for page in (0, 64, 256):
        specs.append(("ragged step 24 decode rows + 4 x 384 %s bf16" % ("contiguous" if not page else "pages of %d" % page), ragged_lens, ragged_nqs, page, bf, -1))
    for page in (0, 64, 256):
        specs.append(("chunk 512 on 8192 keys B4 window 1023 %s bf16" % ("contiguous" if not page else "pages of %d" % page), [8192] * 4, [512] * 4, page, bf, 1023))
    lines = ["prefill_bench: H%d Hkv%d D%d, %d rounds of %d calls, us per call: median (spread = (max - min) / median)" % (H, HKV, D, a.rounds, a.iters),
             "%-62s %18s %18s %18s  %s" % ("row", "prefill", "varlen (packed)", "gather + varlen", "bit-equal")]
    print("\n".join(lines), flush=True)
    with torch.no_grad():
        for spec in specs:
            name, fns, same = case(*spec, g, dev)
            t = benchlib.interleaved(fns, a.rounds, a.iters)
            cell = lambda n: "%8.1f (%4.1f %%)" % (t[n][0] * 1e3, 100.0 * (t[n][2] - t[n][1]) / t[n][0])       # noqa: E731
            lines.append("%-62s %18s %18s %18s  %s" % (name, cell("prefill"), cell("varlen"), cell("gather+varlen"), same))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
