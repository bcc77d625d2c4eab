"""Chunked prefill on an e4m3 KV cache (flash_attention_prefill_fp8) against the 16-bit call and against what a user had to do before it existed.

    python tools/prefill_fp8_bench.py [--rounds 9] [--iters 10] [--out profiles/rNN_prefill_fp8_bench.txt]

Per row three routes, timed round-robin on one device (tools/benchlib.py: interleaved rounds, median, spread = (max - min) / median):
    fp8              flash_attention_prefill_fp8 on the e4m3 cache as it lies (contiguous, or pages under a shuffled block table), descales [B, Hkv]
    16-bit           flash_attention_prefill on a 16-bit cache of the same shape that holds the dequantised values: the same useful work on twice the
                     cache bytes, so the difference prices the conversion and the register staging (head dim 128 gives up the LDS-DMA form)
    dequant+16-bit   cache.to(dtype) * descale over the live pages — a paged pool: every page a sequence uses, with a per-page descale gathered beforehand on
                     the host from the block table; a contiguous cache: the [B, Nmax] slab — and then the 16-bit call: what a user does today
Shapes: H32 Hkv8 D128 bf16.  The descales are powers of two, so the three routes are compared bit for bit before anything is timed."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchlib  # noqa: E402
from rocwmma_fattn.FlashAttn import flash_attention_prefill, flash_attention_prefill_fp8  # noqa: E402

H, HKV, D = 32, 8, 128
E4M3 = torch.float8_e4m3fn


def case(name, lens, nqs, page, dtype, g, dev):
    B, nmax = len(lens), -(-max(lens) // 256) * 256
    kd = (2.0 ** torch.randint(-3, 4, (B, HKV), generator=g).float()).to(dev)
    vd = (2.0 ** torch.randint(-3, 4, (B, HKV), generator=g).float()).to(dev)
    # the e4m3 codes as exact 16-bit values, and the dequantised 16-bit caches (exact under power-of-two descales)
    kcode = (torch.randn((B, nmax, HKV, D), generator=g).to(dev) / kd[:, None, :, None]).to(E4M3).to(dtype)
    vcode = (torch.randn((B, nmax, HKV, D), generator=g).to(dev) / vd[:, None, :, None]).to(E4M3).to(dtype)
    q = torch.randn((sum(nqs), H, D), generator=g).to(dtype).to(dev)
    cu_q = torch.tensor([0] + torch.tensor(nqs).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    if page:
        pk, pv, bt = benchlib.paged_pool(kcode, vcode, page, g, lens=lens)
        owner = torch.zeros(pk.shape[0], dtype=torch.long)                    # the sequence that owns a page (spare pages: sequence 0, they hold zeros)
        btc = bt.cpu().long()
        for b, n in enumerate(lens):
            owner[btc[b, :-(-n // page)]] = b
        kdp, vdp = kd[owner.to(dev)][:, None, :, None].to(dtype), vd[owner.to(dev)][:, None, :, None].to(dtype)
    else:
        pk, pv, bt = kcode, vcode, None
        kdp, vdp = kd[:, None, :, None].to(dtype), vd[:, None, :, None].to(dtype)
    k8, v8 = pk.to(E4M3), pv.to(E4M3)
    k16, v16 = pk * kdp, pv * vdp
    mq = max(nqs)

    def fp8():
        return flash_attention_prefill_fp8(q, k8, v8, cu_q, lens_d, bt, max_seqlen_q=mq, k_descale=kd, v_descale=vd)

    def wide():
        return flash_attention_prefill(q, k16, v16, cu_q, lens_d, bt, max_seqlen_q=mq)

    def dequant_wide():
        return flash_attention_prefill(q, k8.to(dtype) * kdp, v8.to(dtype) * vdp, cu_q, lens_d, bt, max_seqlen_q=mq)

    with torch.no_grad():
        a, b, c = fp8(), wide(), dequant_wide()
    if not (torch.equal(a, b) and torch.equal(a, c)):
        benchlib.close("prefill_fp8_bench", a, b, dtype, name)
    return name, {"fp8": fp8, "16-bit": wide, "dequant+16-bit": dequant_wide}, bool(torch.equal(a, b) and torch.equal(a, c))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    bf = torch.bfloat16
    ragged_lens = [592 + (7947 - 592) * i // 27 for i in range(28)]
    ragged_nqs = [384 if i % 7 == 3 else 1 for i in range(28)]
    layout = lambda page: "contiguous" if not page else "pages of %d" % page       # noqa: E731
    specs = []
    for page in (0, 256, 64):
        specs.append(("chunk 512 on 8192 keys B4 %s bf16" % layout(page), [8192] * 4, [512] * 4, page, bf))
    for page in (0, 256, 64):
        specs.append(("prefix hit 3072 + 1024 new B8 %s bf16" % layout(page), [4096] * 8, [1024] * 8, page, bf))
    for page in (0, 256, 64):
        specs.append(("ragged step 24 decode rows + 4 x 384 %s bf16" % layout(page), ragged_lens, ragged_nqs, page, bf))
    lines = ["prefill_fp8_bench: H%d Hkv%d D%d, %d rounds of %d calls, us per call: median (spread = (max - min) / median)" % (H, HKV, D, a.rounds, a.iters),
             "%-58s %18s %18s %18s  %9s %9s  %s" % ("row", "fp8", "16-bit", "dequant + 16-bit", "fp8/16", "fp8/deq", "bit-equal")]
    print("\n".join(lines), flush=True)
    with torch.no_grad():
        for spec in specs:
            name, fns, same = case(*spec, g, dev)
            t = benchlib.interleaved(fns, a.rounds, a.iters)
            cell = lambda n: "%8.1f (%4.1f %%)" % (t[n][0] * 1e3, 100.0 * (t[n][2] - t[n][1]) / t[n][0])       # noqa: E731
            lines.append("%-58s %18s %18s %18s  %9.3f %9.3f  %s" % (name, cell("fp8"), cell("16-bit"), cell("dequant+16-bit"), t["fp8"][0] / t["16-bit"][0],
                                                                      t["fp8"][0] / t["dequant+16-bit"][0], same))
            print(lines[-1], flush=True)
            del fns
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
