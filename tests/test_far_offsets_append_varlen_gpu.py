"""Far-offset test of the packed KV-cache append (kvcache_append_varlen / fa2_kvcache_append_varlen), in the manner of tests/test_far_offsets_append_gpu.py
and with the helpers of tests/far_layouts.py (Slot, place_rows, _bslot, validate, the arena and harvest).  The packed k / v / q rows are 16 MiB + 12 KiB
apart in one poisoned arena: the rows from token 128 on lie past byte offset 2^31, those from token 256 on past 2^32.  The pool's pages lie 64 MiB +
20 KiB apart, and every sequence's new tokens land in pages below 2^31, between 2^31 and 2^32 and past 2^32; the block table's rows are 2^31 + 12 KiB
apart.  Every product of the kernel — token times row pitch, page id times page stride, row times row pitch, sequence times block-table stride — must be
64-bit.  The call (rotary, GPT-NeoX pairing, q given; eight tail tokens behind cu[B]) matches a compact twin with its own page numbering bit for bit,
every byte of the pool outside the targeted rows is still poison, and after the views are poisoned again the whole arena is poison.  The module skips
when the device has less free memory than the arena plus 2 GiB, like its model."""
import pytest
import torch

import decode_calls as dc
import far_layouts as fl
import prefill_calls as pc
from rocwmma_fattn.FlashAttn import kvcache_append_varlen

pytestmark = pytest.mark.gpu

DT, H, HKV, D, PAGE, PER = torch.float16, 4, 2, 128, 64, 16
COUNTS, LENS, TOTAL = (130, 70, 60), (200, 70, 1000), 268       # 260 owned tokens, 8 behind cu[B]
PITCH = 16 * fl.MIB + 3 * 4096                                  # bytes between two packed rows
ROWS_AT = fl.MIB + 1040                                         # the first row's columns: behind the compact tensors, in front of the pool
# logical page -> region of its physical page, per sequence (the pages its new tokens touch)
REGIONS = {(0, 1): "low", (0, 2): "mid", (0, 3): "high", (1, 0): "mid", (1, 1): "high", (2, 14): "high", (2, 15): "mid"}


@pytest.fixture(scope="module")
def arena():
    dev = dc.dev()
    free, _ = torch.cuda.mem_get_info()
    if free < fl.ARENA_BYTES + 2 * fl.GIB:
        pytest.skip("the far-offset arena needs %.2f GiB + 2 GiB of free device memory, the device reports %.2f GiB" % (fl.ARENA_BYTES / fl.GIB, free / fl.GIB))
    a = fl.new_arena(fl.ARENA_BYTES, dev)
    yield a
    del a
    torch.cuda.empty_cache()


def _page_at(p):
    return fl.DECODE_POOL_BASE + p * fl.DECODE_PAGE_STRIDE


def _far_slots():
    i32 = torch.int32
    slots = fl.place_rows([("k_new", DT, (TOTAL, HKV, D)), ("v_new", DT, (TOTAL, HKV, D)), ("q", DT, (TOTAL, H, D))], PITCH, start=ROWS_AT)
    block = fl._up(PAGE * HKV * D * 2, 4096) + 4096
    for i, n in enumerate(("k", "v")):
        slots[n] = fl._bslot(n, DT, (fl.DECODE_NUM_PAGES, PAGE, HKV, D), [fl.DECODE_PAGE_STRIDE, HKV * D * 2, D * 2], _page_at(0) + i * block)
    slots["cu"] = fl.Slot("cu", i32, (len(COUNTS) + 1,), (1,), 4096)
    slots["lens"] = fl.Slot("lens", i32, (len(COUNTS),), (1,), 8192)
    slots["bt"] = fl.Slot("bt", i32, (len(COUNTS), PER), (fl.FAR_STEP // 4, 1), 16384)
    return slots, block


def _twin_slots(pages):
    slots, cur = {}, 0
    for n, dt, shape in (("k_new", DT, (TOTAL, HKV, D)), ("v_new", DT, (TOTAL, HKV, D)), ("q", DT, (TOTAL, H, D)), ("k", DT, (pages, PAGE, HKV, D)),
                         ("v", DT, (pages, PAGE, HKV, D)), ("cu", torch.int32, (len(COUNTS) + 1,)), ("lens", torch.int32, (len(COUNTS),)),
                         ("bt", torch.int32, (len(COUNTS), PER))):
        st = [1]
        for m in reversed(shape[1:]):
            st.insert(0, st[0] * m)
        es = torch.empty((), dtype=dt).element_size()
        slots[n] = fl.Slot(n, dt, shape, tuple(st), cur, "packed" if n in ("k_new", "v_new", "q") else None)
        cur += fl._up(st[0] * shape[0] * es, 4096) + 4096
    return slots, cur


def _tables(rot, n):
    inv = 10000.0 ** (-torch.arange(0, rot, 2, dtype=torch.float64) / rot)
    ang = torch.arange(n, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().float(), ang.sin().float()


def test_packed_append_from_far_rows_into_far_pages(arena):
    dev = arena.device
    B = len(COUNTS)
    slots, block = _far_slots()
    fl.validate(list(slots.values()), arena.numel())                     # bounds and overlaps before anything runs
    # physical pages by region, and the two block tables
    at = [_page_at(p) for p in range(fl.DECODE_NUM_PAGES)]
    region = {"low": [p for p, a in enumerate(at) if a + 2 * block <= 1 << 31], "mid": [p for p, a in enumerate(at) if a > 1 << 31 and a + 2 * block <= 1 << 32],
              "high": [p for p, a in enumerate(at) if a > 1 << 32]}
    bt = torch.tensor([pc.BAD_PAGES[i % 2] for i in range(B * PER)], dtype=torch.int32).reshape(B, PER)
    bt_t = bt.clone()
    for n, ((s, pg), r) in enumerate(sorted(REGIONS.items())):
        bt[s, pg] = region[r].pop()
        bt_t[s, pg] = (3 * n + 2) % len(REGIONS)
    assert len(set(bt[bt >= 0].tolist()) - {2 ** 30}) == len(REGIONS) and sorted(set(bt_t[(bt_t >= 0) & (bt_t < 2 ** 30)].tolist())) == list(range(len(REGIONS)))
    twin, tbytes = _twin_slots(len(REGIONS) + 1)
    tarena = fl.new_arena(fl._up(tbytes, 8) + 8, dev)
    fl.validate(list(twin.values()), tarena.numel())
    cu = [0, 130, 200, 260]
    targets = [(s, i, LENS[s] - COUNTS[s] + i) for s in range(B) for i in range(COUNTS[s])]
    assert all(0 <= p < PER * PAGE and (s, p // PAGE) in REGIONS for (s, i, p) in targets)
    # what the layout claims: source rows and destination pages past 2^31 and past 2^32, a block-table row past 2^32
    assert slots["k_new"].slice_range(0, 128)[0] > 1 << 31 and slots["k_new"].slice_range(0, 127)[1] < 1 << 31 and slots["q"].slice_range(0, 256)[0] > 1 << 32
    starts = [at[int(bt[s, p // PAGE])] for (s, i, p) in targets]
    assert any(a < 1 << 31 for a in starts) and any(1 << 31 < a < 1 << 32 for a in starts) and max(starts) > 1 << 32
    assert slots["bt"].slice_range(0, 2)[0] > 1 << 32
    g = torch.Generator(device="cpu").manual_seed(0x5EED7000)
    data = {"q": torch.randn((TOTAL, H, D), generator=g).to(DT), "k_new": torch.randn((TOTAL, HKV, D), generator=g).to(DT),
            "v_new": torch.randn((TOTAL, HKV, D), generator=g).to(DT), "cu": torch.tensor(cu, dtype=torch.int32), "lens": torch.tensor(LENS, dtype=torch.int32)}
    cos, sin = (t.to(dev) for t in _tables(D, PER * PAGE))
    results = []
    for ar, sl, table in ((arena, slots, bt), (tarena, twin, bt_t)):
        fl.write_inputs(ar, sl, dict(data, bt=table))
        V = {n: s.view(ar) for n, s in sl.items()}
        q_rot = kvcache_append_varlen(V["k"], V["v"], V["k_new"], V["v_new"], V["cu"], V["lens"], block_table=V["bt"], rotary_cos=cos, rotary_sin=sin,
                                      rotary_interleaved=False, q=V["q"])
        torch.cuda.synchronize()
        got = fl.harvest(ar, sl)                                         # raises when a byte outside the views was written
        assert fl.arena_is_poison(ar)
        for n in ("q", "k_new", "v_new", "cu", "lens"):                  # the inputs are untouched
            assert torch.equal(got[n].cpu(), data[n]), n
        assert torch.equal(got["bt"].cpu(), table)
        rows = {}
        for n in ("k", "v"):
            pool = got[n].cpu().contiguous().view(torch.uint8)
            mask = torch.ones(pool.shape[:2], dtype=torch.bool)
            for (s, i, p) in targets:
                mask[int(table[s, p // PAGE]), p % PAGE] = False
            assert bool((pool[mask] == fl.POISON).all()), (n, "a byte of the pool outside the targeted rows changed")
            rows[n] = torch.stack([pool[int(table[s, p // PAGE]), p % PAGE] for (s, i, p) in targets])
            assert not bool((rows[n] == fl.POISON).all(dim=-1).any()), (n, "a targeted row was not written")
        results.append((rows, q_rot.cpu()))
    (far_rows, far_q), (twin_rows, twin_q) = results
    assert torch.equal(far_rows["k"], twin_rows["k"]) and torch.equal(far_rows["v"], twin_rows["v"]), "the appended rows against the compact twin"
    assert torch.equal(far_q.view(torch.int16), twin_q.view(torch.int16)) and bool(torch.isfinite(far_q.float()).all())
    # V is not rotated: the source rows bit for bit; the tail tokens' q rows come back as they were, the owned ones rotated
    assert torch.equal(far_rows["v"], data["v_new"][:260].contiguous().view(torch.uint8))
    assert torch.equal(far_q[260:].view(torch.int16), data["q"][260:].view(torch.int16)) and not torch.equal(far_q[:260], data["q"][:260])
    assert not torch.equal(far_rows["k"], data["k_new"][:260].contiguous().view(torch.uint8))
