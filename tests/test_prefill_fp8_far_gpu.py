"""Chunked prefill against an e4m3 page pool that is a view of one poisoned 4.25 GiB byte buffer, with live pages beyond byte offsets 2^31 and 2^32: the call
must match a compact twin bit for bit, meet the float64 bars, and leave every byte outside o / lse untouched.  An e4m3 cache's strides are bytes: pointer
arithmetic in 16-bit elements left in a tile's descriptor base would double every page offset and read poison (0xFF is an e4m3 NaN code)."""
import pytest
import torch

import far_layouts as fl
import prefill_calls as pc
import prefill_fp8_calls as p8

pytestmark = pytest.mark.gpu

PAGE_STRIDE = 64 * fl.MIB + 5 * 4096          # bytes from page to page; the K pool starts at POOL_BASE, the V pool half a stride behind
POOL_BASE = 8 * fl.MIB
NUM_PAGES = 67                                # pages 32 .. 63 start between 2^31 and 2^32, pages 64 .. 66 past 2^32
SMALL = 1 * fl.MIB                            # q, o, lse, cu_seqlens_q, cache_seqlens, the block table and the descales: in front of the pool


def test_e4m3_pages_past_2_and_4_gib_match_a_compact_twin_and_nothing_else_is_written():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    if torch.cuda.get_device_properties(dev).total_memory < 3 * fl.ARENA_BYTES:
        pytest.skip("needs %d GiB of device memory" % (3 * fl.ARENA_BYTES // fl.GIB))
    H, Hkv, D, dtype, page = 4, 2, 128, torch.float16, 64
    lens, nqs = (300, 129, 65), (200, 129, 3)
    c = p8.make_case(lens, nqs, H, Hkv, D, dtype, 61, dev, descales="general", prefix=False)
    q, cu = c["q"], c["cu"]
    live = [33, 64, 40, 66, 63, 32, 65, 50, 36, 48]        # 5 + 3 + 2 pages, all past 2^31, three of them past 2^32
    assert len(set(live)) == 10 and POOL_BASE + 32 * PAGE_STRIDE > 2 ** 31 and POOL_BASE + 64 * PAGE_STRIDE > 2 ** 32
    assert POOL_BASE + NUM_PAGES * PAGE_STRIDE <= fl.ARENA_BYTES and PAGE_STRIDE % 16 == 0

    arena = fl.new_arena(fl.ARENA_BYTES, dev)

    def pool(base):                 # (element strides of an e4m3 tensor are bytes)
        return arena.as_strided((NUM_PAGES, page, Hkv, D), (PAGE_STRIDE, Hkv * D, D, 1), base)

    def small(t, at):               # a copy of t inside the arena at byte offset `at` (16-byte aligned)
        raw = arena[at:at + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
        raw.copy_(t)
        return raw

    kpool, vpool = pool(POOL_BASE), pool(POOL_BASE + PAGE_STRIDE // 2)
    bt = torch.tensor([pc.BAD_PAGES[i % 2] for i in range(3 * 6)], dtype=torch.int32).view(3, 6)
    compact = [torch.full((len(live) + 1, page, Hkv, D), p8.NAN_BYTE, dtype=torch.uint8, device=dev) for _ in range(2)]
    bt_c, nxt, written = bt.clone(), 0, []
    for b, n in enumerate(lens):
        for j in range(-(-n // page)):
            pid = live[nxt]
            bt[b, j], bt_c[b, j] = pid, nxt
            for far, near, seqs in ((kpool, compact[0], c["kc"]), (vpool, compact[1], c["vc"])):
                rows = seqs[b][j * page:(j + 1) * page].to(p8.E4M3).view(torch.uint8)
                far[pid, :rows.shape[0]] = rows                 # (the rest of the page stays poison: 0xFF is an e4m3 NaN)
                near[nxt, :rows.shape[0]] = rows
                written.append((far[pid, :rows.shape[0]], rows))
            nxt += 1
    at = [SMALL + i * 512 * 1024 for i in range(8)]
    qa, cua, la, bta = small(q, at[0]), small(cu, at[1]), small(torch.tensor(lens, dtype=torch.int32, device=dev), at[2]), small(bt.to(dev), at[3])
    kda, vda = small(c["kd"], at[6]), small(c["vd"], at[7])
    oa = arena[at[4]:at[4] + q.numel() * 2].view(dtype).view(q.shape)
    lsea = arena[at[5]:at[5] + H * q.shape[0] * 4].view(torch.float32).view(H, q.shape[0])
    scale = D ** -0.5
    p8.prefill_fp8_c(qa, kpool.view(p8.E4M3), vpool.view(p8.E4M3), cua, la, bta, max(nqs), scale, kda, vda, window_left=150, out=(oa, lsea))
    torch.cuda.synchronize()
    got = (oa.clone(), lsea.clone())
    twin = p8.prefill_fp8_c(q, compact[0].view(p8.E4M3), compact[1].view(p8.E4M3), cu, la.clone(), bt_c.to(dev), max(nqs), scale, c["kd"], c["vd"], window_left=150)
    assert pc.bits_equal(got[0], twin[0]) and pc.bits_equal(got[1], twin[1])
    assert not pc.check_float64("far", got[0], got[1], pc.reference(q, cu, c["kt"], c["vt"], scale, 150))
    # every byte outside o / lse: what was written there before the call, then poison again
    for t, src in written + [(qa, q), (cua, cu), (bta, bt.to(dev)), (kda, c["kd"]), (vda, c["vd"])]:
        assert torch.equal(t, src)
    for t in [w[0] for w in written] + [qa, cua, la, bta, oa, lsea, kda, vda]:
        t.view(torch.uint8).fill_(fl.POISON)
    assert fl.arena_is_poison(arena), "first stray byte at %r" % fl.first_stray_byte(arena)
