"""Far-offset test of the KV-cache append (kvcache_append / fa2_kvcache_append), in the manner of tests/test_far_offsets_gpu.py and on its layouts
(tests/far_layouts.py: decode_slots, decode_inputs, the arena helpers): the paged decode case whose pages lie 64 MiB apart — below 2^31, between 2^31
and 2^32, past 2^32 —, whose q, block table and descales have batches 2^31 + 12 KiB apart, once with a 16-bit and once with an e4m3 pool.  The
appended rows (k, v [B, Nnew, Hkv, D]) are two further batch-far views of the arena.  Every product of the kernel — page id times page stride, batch
times batch stride, row times row pitch, the block table's and the descales' batch strides — must be 64-bit.

The caches start as the decode case's image with the LAST Nnew rows of every sequence poisoned again; the call (rotary, GPT-NeoX pairing, q given)
must write exactly those rows: they match a compact twin with its own page numbering bit for bit, so does the rotated q, every other byte of the
pool is the image's, and after the views are poisoned again the whole arena is poison.  The module skips when the device has less free memory than
the arena plus 2 GiB, like its model."""
import numpy as np
import pytest
import torch

import decode_calls as dc
import far_layouts as fl
from rocwmma_fattn.FlashAttn import kvcache_append

pytestmark = pytest.mark.gpu

CASE = fl.DECODE_CASES[6]            # decode_paged64: f16, D 128, H 10, Hkv 2, Nq 4, lengths (1000, 0, 129), block table far
NEW_AT = (4 * fl.MIB + 1040, 5 * fl.MIB + 2080)      # k_new / v_new: behind the case's compact tensors, in front of the pool


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


def _slots(case, fmt):
    """decode_slots plus the appended rows: far k_new / v_new with the batch stride of the other batch-far tensors, compact ones for the twin"""
    slots, twin, tbytes = fl.decode_slots(case, fmt)
    io = fl.DTYPES[case["dt"]]
    B, Nq, Hkv, D = case["B"], case["Nq"], case["Hkv"], case["D"]
    for name, at in zip(("k_new", "v_new"), NEW_AT):
        slots[name] = fl.Slot(name, io, (B, Nq, Hkv, D), (fl.FAR_STEP // 2, Hkv * D, D, 1), at)
        twin[name] = fl.Slot(name, io, (B, Nq, Hkv, D), (Nq * Hkv * D, Hkv * D, D, 1), tbytes)
        tbytes += fl._up(B * Nq * Hkv * D * 2, 4096) + 4096
    return slots, twin, tbytes


def _tables(rot, n):
    inv = 10000.0 ** (-torch.arange(0, rot, 2, dtype=torch.float64) / rot)
    ang = torch.arange(n, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().float(), ang.sin().float()


@pytest.mark.parametrize("fmt", fl.DECODE_FORMATS)
def test_append_into_far_pages(fmt, arena):
    case, dev = CASE, arena.device
    B, Nq, Hkv, D, page = case["B"], case["Nq"], case["Hkv"], case["D"], case["page"]
    data = fl.decode_inputs(case, fmt)
    g = torch.Generator(device="cpu").manual_seed(case["seed"] + 1)
    data["k_new"], data["v_new"] = (torch.randn((B, Nq, Hkv, D), generator=g).to(fl.DTYPES[case["dt"]]) for _ in range(2))
    bt, bt_t, _, _ = fl.decode_block_tables(case, fmt)
    bt = bt.copy()
    for b, n in enumerate(case["lens"]):                                 # a sequence's pages in ascending physical order: its LAST pages, the append's
        bt[b, :-(-n // page)] = np.sort(bt[b, :-(-n // page)])           # targets, are the ones past 2^31 and past 2^32
    slots, twin, tbytes = _slots(case, fmt)
    fl.validate(list(slots.values()), arena.numel())                     # bounds and overlaps before anything runs
    tarena = fl.new_arena(fl._up(tbytes, 8) + 8, dev)
    fl.validate(list(twin.values()), tarena.numel())
    # what the layouts claim
    assert slots["k_new"].slice_range(0, 1)[0] > 1 << 31 and slots["k_new"].slice_range(0, 2)[0] > 1 << 32
    assert slots["bt"].slice_range(0, 2)[0] > 1 << 32 and (fmt != "fp8" or slots["kd"].slice_range(0, 2)[0] > 1 << 32)
    targets = [(b, n - Nq + i) for b, n in enumerate(case["lens"]) for i in range(Nq) if n - Nq + i >= 0]
    starts = [slots["k"].offset + int(bt[b, p // page]) * fl.DECODE_PAGE_STRIDE for (b, p) in targets]
    assert any(1 << 31 < s < 1 << 32 for s in starts) and max(starts) > 1 << 32, "target pages past 2^31 and past 2^32"
    cos, sin = (t.to(dev) for t in _tables(D, fl.DECODE_NMAX))
    results = []
    for ar, sl, table in ((arena, slots, bt), (tarena, twin, bt_t)):
        images = fl.decode_images(case, fmt, sl, data, table)
        for n in ("k_new", "v_new"):
            images[n] = data[n].contiguous().view(torch.uint8)
        before = {n: images[n].clone() for n in ("k", "v")}
        for (b, p) in targets:                                           # the rows the append must write: poison again
            for n in ("k", "v"):
                before[n][int(table[b, p // page]), p % page] = fl.POISON
        for n, im in images.items():
            sl[n].bytes_view(ar).copy_(before.get(n, im))
        V = {n: s.view(ar) for n, s in sl.items()}
        q_rot = kvcache_append(V["k"], V["v"], V["k_new"], V["v_new"], V["lens"], block_table=V["bt"], rotary_cos=cos, rotary_sin=sin, rotary_interleaved=False,
                               k_descale=V.get("kd"), v_descale=V.get("vd"), q=V["q"])
        torch.cuda.synchronize()
        got = fl.harvest(ar, {n: s for n, s in sl.items() if n not in ("o", "lse")})       # raises when a byte outside the views was written
        assert fl.arena_is_poison(ar)
        # inputs untouched, and every byte of the pool outside the targets is the image's
        assert not fl.image_failures(got, {n: im for n, im in images.items() if n not in ("k", "v")})
        rows = {}
        for n in ("k", "v"):
            pool = got[n].cpu().contiguous().view(torch.uint8).reshape(before[n].shape)
            mask = torch.ones(pool.shape[:2], dtype=torch.bool)
            for (b, p) in targets:
                mask[int(table[b, p // page]), p % page] = False
            assert torch.equal(pool[mask], before[n][mask]), (fmt, n, "a byte outside the targeted rows changed")
            rows[n] = torch.stack([pool[int(table[b, p // page]), p % page] for (b, p) in targets])
            assert not bool((rows[n] == fl.POISON).all(dim=-1).any()), (fmt, n, "a targeted row was not written")
        results.append((rows, q_rot.cpu()))
    (far_rows, far_q), (twin_rows, twin_q) = results
    assert torch.equal(far_rows["k"], twin_rows["k"]) and torch.equal(far_rows["v"], twin_rows["v"]), "the appended rows against the compact twin"
    assert torch.equal(far_q.view(torch.int16), twin_q.view(torch.int16)) and bool(torch.isfinite(far_q.float()).all())
    # V is not rotated: the source bit for bit (16-bit), or torch's cast of v / descale after the clamp (e4m3, power-of-two descales)
    src = torch.stack([data["v_new"][b, p - (case["lens"][b] - Nq)] for (b, p) in targets])
    if fmt == "fp8":
        d = torch.ones(len(targets), Hkv, 1) if data["vd"] is None else torch.stack([data["vd"][b] for (b, p) in targets])[:, :, None]
        want = (src.float() / d).clamp(-448.0, 448.0).to(fl.E4M3).view(torch.uint8)
    else:
        want = src.contiguous().view(torch.uint8)
    assert torch.equal(far_rows["v"], want)
    assert len(targets) == 2 * Nq and np.all(np.asarray(bt)[[b for b, _ in targets], [p // page for _, p in targets]] >= 0)
