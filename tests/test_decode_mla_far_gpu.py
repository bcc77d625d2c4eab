"""Latent-cache decode against a page pool whose live pages start past byte offsets 2^31 and 2^32 of one poisoned buffer, with the block table and the
workspace past 2^32 as well: the call must match a compact twin bit for bit and leave every byte outside o / lse / the workspace untouched (the kernel
forms every address in 64 bits: DESIGN section 28)."""
import pytest
import torch

import decode_calls as dc
import decode_refs as dr
import far_layouts as fl
import mla_refs as mr

pytestmark = pytest.mark.gpu

PAGE_STRIDE = 64 * fl.MIB + 5 * 4096          # bytes from page to page
POOL_BASE = 8 * fl.MIB
NUM_PAGES = 67                                # pages 32 .. 63 start between 2^31 and 2^32, pages 64 .. 66 past 2^32
SMALL = 1 * fl.MIB                            # q, o, lse and cache_seqlens: in front of the pool
FAR_SMALL = POOL_BASE + NUM_PAGES * PAGE_STRIDE + fl.MIB      # the block table and the workspace: behind it, past 2^32


def test_pages_table_and_workspace_past_4_gib_match_a_compact_twin_and_nothing_else_is_written():
    dev = dc.dev()
    if torch.cuda.get_device_properties(dev).total_memory < 3 * fl.ARENA_BYTES:
        pytest.skip("needs %d GiB of device memory" % (3 * fl.ARENA_BYTES // fl.GIB))
    H, Nq, dtype, page, split = 16, 2, torch.bfloat16, 64, 3
    lens = [300, 129, 65]
    q, kv = mr.inputs(3, H, Nq, 320, lens, dtype, 61)
    live = [33, 64, 40, 66, 63, 32, 65, 50, 36, 48]        # 5 + 3 + 2 pages, all past 2^31, three of them past 2^32
    assert len(set(live)) == 10 and POOL_BASE + 32 * PAGE_STRIDE > 2 ** 31 and POOL_BASE + 64 * PAGE_STRIDE > 2 ** 32 and FAR_SMALL > 2 ** 32
    ws_bytes = 3 * split * Nq * H * 513 * 4
    assert FAR_SMALL + fl.MIB + ws_bytes <= fl.ARENA_BYTES

    arena = fl.new_arena(fl.ARENA_BYTES, dev)
    pool = arena.view(dtype).as_strided((NUM_PAGES, page, mr.D), (PAGE_STRIDE // 2, mr.D, 1), POOL_BASE // 2)

    def small(t, at):           # a copy of t inside the arena at byte offset `at` (16-byte aligned)
        raw = arena[at:at + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
        raw.copy_(t)
        return raw

    bt = torch.tensor([[-3, NUM_PAGES + 9][i % 2] for i in range(3 * 6)], dtype=torch.int32).view(3, 6)      # unused entries: ids outside the pool
    compact = torch.full((len(live) + 1, page, mr.D), float("nan"), dtype=dtype, device=dev)
    bt_c, nxt, written = bt.clone(), 0, []
    for b, n in enumerate(lens):
        for j in range(-(-n // page)):
            pid = live[nxt]
            bt[b, j], bt_c[b, j] = pid, nxt
            rows = kv[b, j * page:min((j + 1) * page, n)].to(dev)
            pool[pid, :rows.shape[0]] = rows                    # (the rest of the page stays poison: 0xFFFF is a NaN in both 16-bit formats)
            compact[nxt, :rows.shape[0]] = rows
            written.append((pool[pid, :rows.shape[0]], rows))
            nxt += 1
    qd = q.to(dev)
    at = [SMALL + i * 512 * 1024 for i in range(4)]
    qa, la = small(qd, at[0]), small(torch.tensor(lens, dtype=torch.int32, device=dev), at[1])
    oa = arena[at[2]:at[2] + 3 * Nq * H * mr.DV * 2].view(dtype).view(3, Nq, H, mr.DV)
    lsea = arena[at[3]:at[3] + 3 * H * Nq * 4].view(torch.float32).view(3, H, Nq)
    bta = small(bt.to(dev), FAR_SMALL)
    wsa = arena[FAR_SMALL + fl.MIB:FAR_SMALL + fl.MIB + ws_bytes].view(torch.float32)
    mr.mla_c(qa, pool, la, split, block_table=bta, o=oa, lse=lsea, ws=wsa)
    got = (oa.clone(), lsea.clone())
    twin = mr.mla_c(qd, compact, la.clone(), split, block_table=bt_c.clamp(0, len(live)).to(dev))
    assert dc.same_bits(got, twin)
    dr.check(got[0], got[1], mr.refs(q, kv, lens, dc.code(dtype)), lens, dc.code(dtype), "far")
    # every byte outside o / lse / the workspace: what was written there before the call, then poison again
    for t, src in written + [(qa, qd), (bta, bt.to(dev))]:
        assert torch.equal(t, src)
    for t in [w[0] for w in written] + [qa, la, bta, oa, lsea, wsa]:
        t.view(torch.uint8).fill_(fl.POISON)
    assert fl.arena_is_poison(arena), "first stray byte at %r" % fl.first_stray_byte(arena)
