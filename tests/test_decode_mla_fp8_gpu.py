"""GPU tests of flash_attention_decode_mla on an e4m3 latent cache of 656-byte rows, dense and sparse.  References: mla_refs.refs (the oracle and float64)
on the DEQUANTISED cache, and the 16-bit call on it, which the e4m3 call must equal bit for bit.  Before quantising, the four column groups are
multiplied by (1, 4, 1/4, 16) and row j by 1 + j % 7, so a swapped group or a neighbour's scale is far outside any bar; every dead row is 0xFF bytes."""
import functools

import pytest
import torch

import decode_calls as dc
import decode_refs as dr
import mla_refs as mr
import test_decode_mla_sparse_gpu as sp
from rocwmma_fattn.FlashAttn import flash_attention_decode_mla, mla_cache_from_fp8, mla_cache_to_fp8

pytestmark = pytest.mark.gpu
F16, BF16, LN2, I32_MAX, ROW = torch.float16, torch.bfloat16, 0.6931471805599453, 2 ** 31 - 1, 656
CAP, LENS = 1312, ((1, 31, 32, 33), (64, 65, 97, 0), (300, 1000, 1311, 7))
SHAPES = ((1, 1), (16, 1), (17, 3), (128, 1), (128, 4))                                    # (H, Nq)
SPARSE = ((1, 1, 1), (16, 3, 31), (128, 1, 33), (128, 3, 200), (16, 1, 200))               # (H, Nq, topk) on sp.NMAX, sp.LENS


def quantised(kv):
    """[B, N, 576] N(0, 1) -> (the e4m3 cache, its dequantised 16-bit twin), the groups and rows scaled first.  The factors are (1, 4, 1/4, 16) and
    1 + j % 7 over their largest product, 112: the ratios between groups and between rows are what a wrong scale shows in, and the values stay within
    N(0, 1), where decode_refs.check's absolute bars were derived (with factors up to 112 the oracle itself misses them against float64)"""
    f = torch.tensor([1.0, 4.0, 0.25, 16.0]).repeat_interleave(128) / 112.0
    x = kv.float()
    x[..., :512] *= f * (1 + torch.arange(kv.shape[1]) % 7)[:, None]
    c8 = mla_cache_to_fp8(x.to(kv.dtype))
    return c8, mla_cache_from_fp8(c8, kv.dtype)


def pages(c8, lens, page, g):
    """dc.paged for a byte cache: shuffled physical pages, everything no block table names 0xFF -> pool, block table"""
    bt, total, placed = dc.block_table(lens, c8.shape[1] // page, page, g)
    pool = torch.full((total, page, ROW), 0xFF, dtype=torch.uint8)
    for b, j, pid in placed:
        pool[pid] = c8[b, j * page:(j + 1) * page]
    return pool, bt


def call(q, kv, lens, split, **kw):
    o, lse = flash_attention_decode_mla(q, kv, lens, num_splits=split, return_lse=True, **kw)
    return o, lse / LN2


@functools.lru_cache(maxsize=None)
def dense_case(s, k, dtype):
    (H, Nq), lens = SHAPES[s], LENS[k]
    q, kv = mr.inputs(4, H, Nq, CAP, lens, dtype, 600 + 10 * s + k, poison=False)
    c8, deq = quantised(kv)
    for b, n in enumerate(lens):
        c8[b, n:] = 0xFF
    return q, c8, deq, mr.refs(q, deq, lens, dc.code(dtype))


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("s", range(len(SHAPES)))
def test_dense_against_oracle_float64_and_the_16bit_call(s, dtype):
    for k, lens in enumerate(LENS):
        q, c8, deq, refs = dense_case(s, k, dtype)
        qd, cd, dd, ld = sp.on(dc.dev(), q, c8, deq, lens)
        for split in (1, 2, 5, 0):                     # 5 parts of 41 tiles: lengths up to 33 leave four of them empty
            got = call(qd, cd, ld, split)
            dr.check(*got, refs, lens, dc.code(dtype), ("fp8", SHAPES[s], lens, split))
            assert dc.same_bits(got, call(qd, dd, ld, split)), ("the 16-bit call on the dequantised cache", SHAPES[s], lens, split)


@pytest.mark.parametrize("kind", ["page64", "page128", "strided"])
def test_paged_and_strided_equal_contiguous_bit_for_bit(kind):
    dev, H, Nq, lens, dtype, g = dc.dev(), 17, 3, [300, 129, 65, 0], F16 if kind == "page64" else BF16, torch.Generator().manual_seed(5)
    q, kv = mr.inputs(4, H, Nq, 384, lens, dtype, 78, poison=False)
    kv[1, :128] = kv[0, :128]
    c8 = quantised(kv)[0]
    for b, n in enumerate(lens):
        c8[b, n:] = 0xFF
    qd, cd, ld = sp.on(dev, q, c8, lens)
    if kind == "strided":                              # a row pitch of 672 bytes inside a wider buffer, 0xFF between the rows
        buf, bt = torch.full((4, 385, 672), 0xFF, dtype=torch.uint8, device=dev), None
        cache = buf[:, 1:, :ROW]
        cache.copy_(cd)
    else:
        page = int(kind[4:])
        cache, bt = pages(c8, lens, page, g)
        cache[bt[1, 0]] = 0xFF                         # one page shared by two sequences
        bt[1, 0] = bt[0, 0]
        for b, n in enumerate(lens):
            bt[b, -(-n // page):] = I32_MAX
        cache, bt = sp.on(dev, cache, bt)
    for split in (1, 2):
        got = call(qd, cache.view(torch.float8_e4m3fn) if split == 2 else cache, ld, split, block_table=bt)
        assert dc.same_bits(got, call(qd, cd, ld, split)) and bool(torch.isfinite(got[0]).all()), (kind, split)
    if kind == "strided":
        assert bool((buf[:, :, ROW:] == 0xFF).all()) and bool((buf[:, 0] == 0xFF).all()) and torch.equal(buf[:, 1:, :ROW], cd)


@functools.lru_cache(maxsize=None)
def sparse_case(s, dtype):
    H, Nq, topk = SPARSE[s]
    q, kv = mr.inputs(len(sp.LENS), H, Nq, sp.NMAX, sp.LENS, dtype, 700 + s, poison=False)
    idx = sp.lists(len(sp.LENS), Nq, sp.LENS, topk, torch.Generator().manual_seed(800 + s))
    c8, deq = quantised(kv)
    named = torch.zeros(kv.shape[:2], dtype=torch.bool)
    for r, js in enumerate(sp.gathered(q, deq, idx, sp.LENS)[0]):
        named[r // Nq, js] = True
    c8[~named] = 0xFF                                  # every row no valid entry names
    _, gq, gk, glens = sp.gathered(q, deq, idx, sp.LENS)
    assert sum(n > 0 for n in glens) > len(glens) // 2 and 0 in glens
    return q, c8, deq, idx, glens, mr.refs(gq, gk, glens, dc.code(dtype))


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("s", range(len(SPARSE)))
def test_sparse_lists_rows_and_the_16bit_call(s, dtype):
    q, c8, deq, idx, glens, refs = sparse_case(s, dtype)
    qd, cd, dd, idxd, ld = sp.on(dc.dev(), q, c8, deq, idx, sp.LENS)
    pool, bt = sp.on(dc.dev(), *pages(c8, sp.LENS, 64, torch.Generator().manual_seed(6)))
    for split in (1, 2, 5):                            # (sp.lists: row (3, 0) keeps half a list of -1, the last row none: parts without a valid entry)
        got = call(qd, cd, ld, split, indices=idxd)
        sp.check(*got, refs, glens, dtype, ("fp8 sparse", SPARSE[s], split))
        assert dc.same_bits(got, call(qd, dd, ld, split, indices=idxd)), ("the 16-bit sparse call on the dequantised cache", SPARSE[s], split)
        assert dc.same_bits(got, call(qd, pool, ld, split, indices=idxd, block_table=bt)), ("paged", SPARSE[s], split)


@pytest.mark.parametrize("sparse", [False, True])
def test_graph_replay_follows_lengths_table_indices_and_cache_bytes_changed_in_place(sparse):
    dev, H, Nq, topk, g = dc.dev(), 16, 3, 69, torch.Generator().manual_seed(9)
    q, kv = mr.inputs(3, H, Nq, sp.NMAX, [sp.NMAX] * 3, BF16, 92, poison=False)
    c8 = quantised(kv)[0]
    pool, bt = pages(c8, [sp.NMAX] * 3, 64, g)
    lens_a, lens_b = [300, 65, 33], [129, 0, 320]
    idx_a, idx_b = sp.lists(3, Nq, lens_a, topk, g), sp.lists(3, Nq, lens_b, topk, g)
    qd, pa, ld, btd, idxd = sp.on(dev, q, pool, lens_a, bt, idx_a)
    pb = pa.flip(1).contiguous()                       # other bytes in every page: the rows of a page in reverse order
    poold = pa.clone()
    run = lambda: flash_attention_decode_mla(qd, poold, ld, block_table=btd, indices=idxd if sparse else None, return_lse=True, num_splits=2)      # noqa: E731
    run()                                              # (warm-up: the library is loaded outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = run()
    for lens, idx, table, bytes_ in ((lens_a, idx_a, bt, pa), (lens_b, idx_b, bt, pa), (lens_b, idx_b, bt.flip(1), pb), (lens_a, idx_b, bt, pb), (lens_a, idx_a, bt, pa)):
        ld.copy_(torch.tensor(lens, dtype=torch.int32))
        idxd.copy_(idx), btd.copy_(table), poold.copy_(bytes_)
        graph.replay()
        torch.cuda.synchronize()
        eager = run()
        assert torch.equal(o.view(torch.int16), eager[0].view(torch.int16)) and torch.equal(lse, eager[1]), lens
