"""Decode attention on a latent (MLA) KV cache: flash_attention_decode_mla against what a holder of such a cache ran before the library had the call,
same box, interleaved rounds, median of per-round event times with the spread of the rounds beside it (tools/decode_bench.py's method).

    python tools/mla_decode_bench.py [--rounds R] [--iters I] [--out FILE] [--only LABEL-PREFIX] [--routes mla,torch]

Routes
    mla          flash_attention_decode_mla(q, kv_cache, cache_seqlens) on a [B, Nmax, 576] cache (paged rows: [num_pages, 64, 576] under a block table)
    torch        the BASELINE — there is no other route in the library: torch matmul -> f32 masked softmax -> matmul on kv[:, :len] (ragged rows: on
                 kv[:, :max len] under a length mask), which materialises [B, Nq * H, N] scores and reads the cache twice.  Its K and V operands are
                 contiguous tensors of their own, cut out of the cache OUTSIDE the timed region: the baseline at its best
    torch+gather (paged rows) the same with the gather of the pages into a contiguous tensor inside the timed region: what serving a pool costs per step
Every row prints the valid cache bytes (1 152 per key, once: what a perfect kernel has to read), the time they take at 6.3 TB/s (the achievable HBM rate
DESIGN section 20 uses) and each route's achieved bytes/s.  A route is called faster only where the gap exceeds the sum of the two spreads.  Each row
first checks the routes against each other on the timed inputs (fp16 1e-3 + 2e-3 |x|, bf16 8e-3 + 1.6e-2 |x|).  The same cache is read in every
iteration, so caches up to the 256 MB of Infinity Cache are served from it in every route alike."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd"))

import torch  # noqa: E402

from benchlib import close, interleaved, paged_pool  # noqa: E402
from rocwmma_fattn import _fa2_lib  # noqa: E402
from rocwmma_fattn.FlashAttn import flash_attention_decode_mla  # noqa: E402

HBM_TBS = 6.3
D, DV, SCALE = 576, 512, 576 ** -0.5
BF16, F16 = torch.bfloat16, torch.float16
# Row 4 has no baseline: torch.matmul on [8, 256, 576] x [8, 576, 8192] bf16 ended in an illegal memory access on the measuring machine, in this tool and
# again alone in a fresh process that never loaded the library (profiles/r49_mla_decode_bench.txt), so the tool does not run it.
NO_TORCH = ("4_b8_h128_nq2",)
ROWS = [  # (label, B, H, Nq, keys or (shortest, longest), dtype, paged)
    ("1_b1_h128", 1, 128, 1, 8192, BF16, False),
    ("2_b32_h128", 32, 128, 1, 4096, BF16, False),
    ("3_b32_h16_tp8", 32, 16, 1, 4096, BF16, False),
    ("4_b8_h128_nq2", 8, 128, 2, 8192, BF16, False),
    ("5_ragged_b32_h128", 32, 128, 1, (256, 8192), BF16, False),
    ("6a_b32_h128_pg64", 32, 128, 1, 4096, BF16, True),
    ("6b_ragged_pg64", 32, 128, 1, (256, 8192), BF16, True),
    ("7_b32_h128_fp16", 32, 128, 1, 4096, F16, False),
]


def torch_route(q, k, v, lens):
    """softmax(scale q k^T) v for k [B, N, 576] and v [B, N, 512], both contiguous, under the length and causal masks; scores and softmax in f32"""
    B, Nq, H, _ = q.shape
    nmax_used = k.shape[1]
    s = torch.matmul(q.reshape(B, Nq * H, D), k.transpose(1, 2)).float() * SCALE                       # [B, Nq * H, N]
    pos = (lens.view(B, 1) - Nq + torch.arange(Nq, device=q.device).view(1, Nq)).repeat_interleave(H, dim=1)      # row r = i * H + h
    s = s.masked_fill(torch.arange(nmax_used, device=q.device).view(1, 1, -1) > pos.unsqueeze(-1), float("-inf"))
    p = torch.softmax(s, dim=-1).to(q.dtype)
    return torch.matmul(p, v).view(B, Nq, H, DV)


def latent(kv, used):
    """kv[:, :used] as the baseline's operands: K [B, used, 576] and V [B, used, 512], each a contiguous tensor of its own"""
    return kv[:, :used].contiguous(), kv[:, :used, :DV].contiguous()


def row(out, label, B, H, Nq, keys, dt, paged, rounds, iters, routes):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(1)
    if isinstance(keys, tuple):
        lens_h = torch.randint(keys[0], keys[1] + 1, (B,), generator=g).tolist()      # decode_bench's ragged row: the same seed, the same draw
        nmax = keys[1]
    else:
        lens_h, nmax = [keys] * B, keys + 256                                         # a cache with room to grow, as in serving
    q = torch.randn((B, Nq, H, D), device=dev, dtype=dt)
    kv = torch.randn((B, nmax, D), device=dev, dtype=dt)
    lens = torch.tensor(lens_h, dtype=torch.int32, device=dev)
    used = max(lens_h)
    fns = {}
    if paged:
        pool, _, bt = paged_pool(kv.unsqueeze(2), kv.unsqueeze(2), 64, g, lens=lens_h)
        pool = pool[:, :, 0]
        fns["mla"] = lambda: flash_attention_decode_mla(q, pool, lens, block_table=bt)
        fns["torch+gather"] = lambda: torch_route(q, *latent(pool[bt.long()].view(B, -1, D), used), lens)
    else:
        fns["mla"] = lambda: flash_attention_decode_mla(q, kv, lens)
    if label not in NO_TORCH:
        kc, vc = latent(kv, used)                                                     # made once, outside the timed region
        fns["torch"] = lambda: torch_route(q, kc, vc, lens)
    if routes:                                                                        # (a developer's look at one route: no comparison, no table)
        fns = {n: f for n, f in fns.items() if n in routes}
        with torch.no_grad():
            print(label, {n: "%.1f us" % (v[0] * 1e3) for n, v in interleaved(fns, rounds, iters).items()})
        return
    with torch.no_grad():
        for n in fns:
            close("mla_decode_bench", fns["mla"](), fns[n](), dt, label + ": mla and " + n)
        t = interleaved(fns, rounds, iters)
    plan = _fa2_lib.decode_mla_plan(0 if dt == F16 else 1, B, H, Nq, bt.shape[1] if paged else nmax, 64 if paged else 0)
    valid = sum(lens_h) * D * 2
    floor_us = valid / (HBM_TBS * 1e12) * 1e6
    shape = "B%d H%d Nq%d keys %s %s%s (split %d, %d row block%s)" % (
        B, H, Nq, keys if not isinstance(keys, tuple) else "%d .. %d (mean %d)" % (min(lens_h), max(lens_h), sum(lens_h) // B), "fp16" if dt == F16 else "bf16",
        " pages of 64" if paged else "", plan.nsplit, plan.row_blocks, "" if plan.row_blocks == 1 else "s")
    lines = ["%-20s %s  valid cache %.1f MB = %.1f us at %.1f TB/s" % (label, shape, valid / 1e6, floor_us, HBM_TBS)]
    m_med, m_lo, m_hi = t["mla"]
    for n, (med, lo, hi) in t.items():
        rel = ""
        if n != "mla":
            real = abs(med - m_med) > (hi - lo) + (m_hi - m_lo)
            rel = "  mla %.2fx %s (%s the sum of the spreads, %.1f us)" % (max(med / m_med, m_med / med), "faster" if m_med <= med else "SLOWER",
                                                                          "beyond" if real else "WITHIN", ((hi - lo) + (m_hi - m_lo)) * 1e3)
        lines.append("    %-12s %9.1f us  (rounds %.1f .. %.1f, spread %.1f %%)  %5.2f TB/s of the valid cache, %.1f x the floor%s"
                     % (n, med * 1e3, lo * 1e3, hi * 1e3, 100.0 * (hi - lo) / med, valid / (med * 1e-3) / 1e12, med * 1e3 / floor_us, rel))
    if label in NO_TORCH:
        lines.append("    torch        not measured: torch.matmul faults at this shape on the measuring machine (see NO_TORCH)")
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
    ap.add_argument("--routes", default="", help="comma-separated routes to time alone (no comparison, no table)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mla_decode_bench: needs a ROCm GPU (a timing taken anywhere else says nothing)")
    out = open(a.out, "w") if a.out else None
    head = "%s (%d CUs) rounds %d iters %d | %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, a.rounds, a.iters,
                                                   _fa2_lib.load().fa2_version().decode())
    print(head)
    if out:
        out.write(head + "\n")
    for r in ROWS:
        if r[0].startswith(a.only):
            row(out, *r, a.rounds, a.iters, [n for n in a.routes.split(",") if n])


if __name__ == "__main__":
    main()
