"""GPU tests of the lightning indexer on an e4m3 index-key cache: mla_indexer_logits / mla_indexer_topk on rows of 132 bytes and on (codes, scales)
blocks, and kvcache_append_mla_index.  The reference and the bar: tests/test_mla_indexer_fp8.py (float64 on the codes and scales the cache holds)."""
import pytest
import torch

import decode_calls as dc
import test_mla_indexer as ti
import test_mla_indexer_fp8 as t8
from rocwmma_fattn.FlashAttn import kvcache_append_mla_index, mla_index_cache_to_fp8, mla_indexer_logits, mla_indexer_q_to_fp8, mla_indexer_topk
from test_mla_indexer_gpu import I32_MAX, on

pytestmark = pytest.mark.gpu
PAGE = 64


def block_views(buf):
    """A buffer of vLLM's blocks [P, 64 * 132] (a page's 64 x 128 code bytes, then its 64 scales) -> its (codes, scales) views"""
    return buf[:, :PAGE * 128].view(len(buf), PAGE, 128), buf[:, PAGE * 128:].view(torch.float32)


def blocks(pool):
    """A pool of row pages [P, 64, 132] -> the same tokens as a buffer of blocks"""
    return torch.cat([pool[:, :, :128].reshape(len(pool), -1), pool[:, :, 128:].reshape(len(pool), -1)], 1).contiguous()


def paged_rows(cache, lens, seed):
    """The whole pages of every sequence in 0xFF-filled pages of 64 under a shuffled block table; behind a sequence's last live page: a far id"""
    bt, total, placed = dc.block_table(lens, cache.shape[1] // PAGE, PAGE, torch.Generator().manual_seed(seed))
    pool = torch.full((total, PAGE, 132), 0xFF, dtype=torch.uint8)
    for b, j, pid in placed:
        pool[pid] = cache[b, j * PAGE:(j + 1) * PAGE]
    for b, n in enumerate(lens):
        bt[b, -(-n // PAGE):] = I32_MAX
    return pool, bt


@pytest.mark.parametrize("key", t8.CASES)
def test_logits_against_float64_in_every_layout(key):
    q, w, lens, cache, ref, _ = t8.case(*key)
    pool, bt = paged_rows(cache, lens, key[1] + key[2])
    qd, wd, ld, cd, poold, bufd, btd = on(dc.dev(), q, w, lens, cache, pool, blocks(pool), bt)
    got = mla_indexer_logits(qd, cd, wd, ld)
    assert got.shape == ref.shape and got.dtype == torch.float32
    t8.check_logits(got, key)
    assert torch.equal(mla_indexer_logits(qd, cd.view(torch.float8_e4m3fn).unsqueeze(2), wd, ld), got), "float8_e4m3fn rows with a head axis of 1"
    n = bt.shape[1] * PAGE
    for name, k in (("rows", poold), ("blocks", block_views(bufd))):
        paged = mla_indexer_logits(qd, k, wd, ld, block_table=btd)
        assert paged.shape[2] == n and torch.equal(paged.view(torch.int32), got[:, :, :n].view(torch.int32)), name + "-paged equals contiguous bit for bit"


@pytest.mark.parametrize("H", [16, 64])
def test_a_16_bit_q_equals_its_quantised_pair(H):
    key = (torch.float16, H, 3, "")
    q, w, lens, cache, _, _ = t8.case(*key)
    q = q.clone()
    q[0, 0, 1] = 0                                     # a head of all zeros: scale 1
    q[2, 1, 5, 77] = 6e4                               # one outlier: every other column of the head becomes a small code
    q8, w8 = mla_indexer_q_to_fp8(q, w)
    assert float(w8[0, 0, 1]) == float(w[0, 0, 1]) and int(q8[2, 1, 5].view(torch.uint8)[77]) == 0x7E
    qd, wd, q8d, w8d, ld, cd = on(dc.dev(), q, w, q8, w8, lens, cache)
    a, b = mla_indexer_logits(qd, cd, wd, ld), mla_indexer_logits(q8d, cd, w8d, ld)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool(torch.isfinite(a[2, 1, :298]).all())


APPEND_LENS = (7, 70, 129)                             # capacity 128: sequence 2 has tokens beyond the cache


def append_case(layout, packed, nnew):
    """-> the call's arguments and the bytes the buffer must hold afterwards: a 0xA5-poisoned cache (rows: contiguous [3, 128, 132]; blocks: a pool of 7
    pages under a table whose entry [1, 1] names a page outside the pool) with the row of every token that has a place rewritten"""
    g = torch.Generator().manual_seed(nnew + packed)
    counts = (2, 0, 5) if packed else (nnew,) * 3
    x = torch.randn((sum(counts) + 2 * packed, 128), generator=g).to(torch.bfloat16)      # packed: two rows beyond cu[B] that no sequence owns
    x[1] = 0
    cu = torch.tensor([0, counts[0], counts[0] + counts[1], sum(counts)], dtype=torch.int32)
    bt = torch.tensor([[3, 0], [5, 7], [1, 6]], dtype=torch.int32)
    buf = torch.full((3, 128, 132) if layout == "rows" else (7, PAGE * 132), 0xA5, dtype=torch.uint8)
    return x, cu, counts, bt, buf


@pytest.mark.parametrize("pow2", [False, True])
@pytest.mark.parametrize("packed,nnew", [(False, 1), (False, 5), (True, 0)])
@pytest.mark.parametrize("layout", ["rows", "blocks"])
def test_append_writes_the_reference_bytes_and_nothing_else(layout, packed, nnew, pow2):
    x, cu, counts, bt, buf = append_case(layout, packed, nnew)
    want, rows = buf.clone(), mla_index_cache_to_fp8(x, scale_pow2=pow2)
    wcodes, wscales = block_views(want) if layout == "blocks" else (None, None)
    for b, n in enumerate(APPEND_LENS):
        for i in range(counts[b]):
            pos, row = n - counts[b] + i, rows[int(cu[b]) + i]
            if layout == "rows" and 0 <= pos < 128:
                want[b, pos] = row
            elif layout == "blocks" and 0 <= pos < 128 and 0 <= int(bt[b, pos // PAGE]) < 7:
                wcodes[bt[b, pos // PAGE], pos % PAGE] = row[:128]
                wscales[bt[b, pos // PAGE], pos % PAGE] = row[128:].view(torch.float32)[0]
    xd, cud, ld, btd, bufd = on(dc.dev(), x, cu, APPEND_LENS, bt, buf)
    cache = bufd if layout == "rows" else block_views(bufd)
    kvcache_append_mla_index(cache, xd if packed else xd.view(3, nnew, 128), ld, block_table=btd if layout == "blocks" else None,
                             cu_seqlens=cud if packed else None, scale_pow2=pow2)
    assert torch.equal(bufd.cpu(), want), "the written rows are mla_index_cache_to_fp8's bytes; every other byte keeps its poison"
    assert not torch.equal(want, buf)


def test_the_step_appends_selects_and_replays_in_a_graph():
    dev, Nq, g = dc.dev(), 3, torch.Generator().manual_seed(13)
    q, _, w, _, _ = ti.case(torch.bfloat16, 64, Nq)
    k16, new = torch.randn((5, 320, 128), generator=g).to(torch.bfloat16), torch.randn((5, Nq, 128), generator=g).to(torch.bfloat16)
    qd, wd, ld, newd, cached = on(dev, q, w, ti.LENS, new, mla_index_cache_to_fp8(k16))

    def step(topk):
        kvcache_append_mla_index(cached, newd, ld)
        return mla_indexer_topk(qd, cached, wd, ld, topk=topk, return_logits=True)

    idx, logits = step(400)                            # topk >= capacity: every position 0 .. pos, then -1
    want = torch.arange(400).expand(5, Nq, 400).clone()
    for b, n in enumerate(ti.LENS):
        for i in range(Nq):
            want[b, i, max(n - Nq + i + 1, 0):] = -1
            if n - Nq + i >= 0:
                assert torch.equal(cached[b, n - Nq + i].cpu(), mla_index_cache_to_fp8(new[b, i])), "the row the step appended"
    assert torch.equal(idx.cpu(), want.to(torch.int32))
    assert torch.equal(step(64)[0].cpu(), ti.topk_ref(logits.cpu(), ti.LENS, 64)), "the list is the stable sort's of the library's own logits"
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        idx, logits = step(64)
    for lens in (ti.LENS, (320, 64, 3, 300, 129), (1, 320, 65, 0, 200), ti.LENS):
        ld.copy_(torch.tensor(lens, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        eager = step(64)
        assert torch.equal(idx, eager[0]) and torch.equal(logits.view(torch.int32), eager[1].view(torch.int32)), lens
        assert torch.equal(idx.cpu(), ti.topk_ref(logits.cpu(), lens, 64)), lens
