"""GPU tests of flash_attention_prefill_mla.  Reference: every packed token as a one-row sequence over its valid entries, in list order, gathered on the
CPU for mla_refs.refs (the oracle and float64, decode_refs.check's bars); cache rows nobody names are NaN.  The float64 / oracle test drives the C
entries on o and lse that were filled with NaN before the call: finite O and an LSE without NaN afterwards mean that every element was written."""
import ctypes
import functools

import pytest
import torch

import decode_calls as dc
import decode_refs as dr
import mla_refs as mr
import test_mla_indexer_varlen as tv
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import (flash_attention_decode_mla, flash_attention_prefill_mla, mla_cache_from_fp8, mla_cache_to_fp8, mla_indexer_topk,
                                     mla_indexer_topk_varlen)
from test_decode_mla_sparse_gpu import I32_MAX, LN2, lists, on

pytestmark = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16
# a zero-length sequence; a keyless one; dead rows (Nq_s > len_s); a chunk of 70 tokens over five pages of 64 — and two slack tokens beyond cu[B]
NQ, LENS, SLACK, NMAX = (0, 1, 3, 70), (5, 0, 2, 300), 2, 384
TOTAL = sum(NQ) + SLACK
CU = torch.tensor([0] + [sum(NQ[:s + 1]) for s in range(len(NQ))], dtype=torch.int32)
HEADS, TOPKS = (1, 17, 64, 128), (1, 31, 33, 69, 200)      # a partial wave, a partial block, one block, two; tile edges and three or more tiles


def packed_lists(topk, g, nq=NQ, lens=LENS, total=TOTAL):
    """test_decode_mla_sparse_gpu.lists per sequence (its junk values, its all-invalid and half-padded rows); slack rows name live-looking positions"""
    rows = [lists(1, n, [lens[s]], topk, g)[0] for s, n in enumerate(nq) if n]
    return torch.cat(rows + [torch.randint(0, 5, (total - sum(nq), topk), generator=g).to(torch.int32)])


def valid_rows(idx, nq=NQ, lens=LENS):
    """per packed token: (sequence, its valid entries in list order); a token nobody owns: (-1, [])"""
    out = []
    for s, n in enumerate(nq):
        for i in range(n):
            out.append((s, [j for j in idx[len(out)].tolist() if 0 <= j <= lens[s] - n + i]))
    return out + [(-1, [])] * (len(idx) - len(out))


@functools.lru_cache(maxsize=None)
def case(H, topk, dtype):
    q = mr.inputs(TOTAL, H, 1, 1, [1] * TOTAL, dtype, 7000 + 10 * H + topk, poison=False)[0]      # [total, 1, H, 576]
    kv = mr.inputs(len(NQ), 1, 1, NMAX, LENS, dtype, 8000 + 10 * H + topk, poison=False)[1]
    idx = packed_lists(topk, torch.Generator().manual_seed(9000 + 10 * H + topk))
    rows, named = valid_rows(idx), torch.zeros(kv.shape[:2], dtype=torch.bool)
    for s, js in rows:
        named[s, js] = True
    kv[~named] = float("nan")
    keys = torch.zeros((TOTAL, max(1, max(len(js) for _, js in rows)), mr.D), dtype=dtype)
    for t, (s, js) in enumerate(rows):
        keys[t, :len(js)] = kv[s, js]
    glens = [len(js) for _, js in rows]
    assert sum(n > 0 for n in glens) > TOTAL // 2 and glens.count(0) > SLACK
    return q[:, 0], kv, idx, glens, mr.refs(q, keys, glens, dc.code(dtype))


def prefill(q, kv, cu, lens, idx, block_table=None):
    o, lse = flash_attention_prefill_mla(q, kv, cu, lens, idx, block_table=block_table, return_lse=True)
    return o, lse / LN2


def prefill_c(q, kv, cu, lens, idx):
    """fa2_fwd_prefill_mla_sparse / _fp8 (a uint8 cache) on NaN-filled o and lse, contiguous cache -> (o, log2 lse)"""
    (total, H, _), k = q.shape, mr.kv4(kv)
    o = torch.full((total, H, mr.DV), float("nan"), dtype=q.dtype, device=q.device)
    lse = torch.full((H, total), float("nan"), dtype=torch.float32, device=q.device)
    entry = getattr(_fa2_lib.load(), "fa2_fwd_prefill_mla_sparse_fp8" if kv.dtype == torch.uint8 else "fa2_fwd_prefill_mla_sparse")
    _fa2_lib.check(entry(dc.code(q.dtype), q.data_ptr(), k.data_ptr(), o.data_ptr(), lse.data_ptr(), idx.data_ptr(), cu.data_ptr(), lens.data_ptr(), None,
                         len(lens), H, total, mr.D, mr.DV, idx.shape[1], k.shape[1], 0, 0, dc.s2(q), dc.s3(k), dc.s2(o), lse.stride(0), idx.stride(0), 0,
                         mr.SCALE, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return o, lse


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("topk", TOPKS)
@pytest.mark.parametrize("H", HEADS)
def test_against_float64_and_the_oracle_on_nan_filled_outputs(H, topk, dtype):
    q, kv, idx, glens, refs = case(H, topk, dtype)
    qd, kvd, cud, ld, idxd, kv8 = on(dc.dev(), q, kv, CU, LENS, idx, mla_cache_to_fp8(kv))
    o, lse2 = prefill_c(qd, kvd, cud, ld, idxd)
    dr.check(o[:, None], lse2.t()[:, :, None], refs, glens, dc.code(dtype), ("prefill", H, topk))
    assert torch.equal(prefill(qd, kvd, cud, ld, idxd)[0].view(torch.int16), o.view(torch.int16)), "the operator makes the same call"
    # e4m3 rows, NaN-filled outputs again: bit for bit the 16-bit call on the dequantised cache — and with that finite where `o` above is
    o8, lse8 = prefill_c(qd, kv8, cud, ld, idxd)
    want = prefill_c(qd, mla_cache_from_fp8(kv8, dtype), cud, ld, idxd)
    assert dc.same_bits((o8, lse8), want) and bool(torch.isfinite(o8).all()) and not bool(torch.isnan(lse8).any())
    assert torch.equal(torch.isfinite(lse8), torch.isfinite(lse2)) and bool((o8[~torch.isfinite(lse8.t())] == 0).all())


def host_loop(q, kv, lens, idx, block_table=None, nq=NQ):
    """The route without the packed call: flash_attention_decode_mla(indices=, num_splits=1) per sequence, in calls of Nq * H <= 512 rows"""
    H, o, lse, t = q.shape[1], torch.zeros((len(q), q.shape[1], mr.DV), dtype=q.dtype, device=q.device), torch.full((q.shape[1], len(q)), float("-inf"), device=q.device), 0
    for s, n in enumerate(nq):
        for a in range(0, n, 512 // H):
            b = min(n, a + 512 // H)
            got = flash_attention_decode_mla(q[None, t + a:t + b], kv if block_table is not None else kv[s:s + 1], lens[s:s + 1] - (n - b), num_splits=1,
                                             block_table=None if block_table is None else block_table[s:s + 1], indices=idx[None, t + a:t + b], return_lse=True)
            o[t + a:t + b], lse[:, t + a:t + b] = got[0][0], got[1][0] / LN2
        t += n
    return o, lse


@pytest.mark.parametrize("kind", ["decode", "decode8", "page64", "page128", "strided"])
def test_bit_for_bit(kind):
    dev, (H, topk), dtype = dc.dev(), (128 if kind == "decode8" else 17, 69), F16 if kind == "page64" else BF16
    q, kv = mr.inputs(TOTAL, H, 1, 1, [1] * TOTAL, dtype, 71, poison=False)[0][:, 0], mr.inputs(len(NQ), 1, 1, NMAX, LENS, dtype, 72)[1]
    qd, kvd, cud, ld, idxd = on(dev, q, kv, CU, LENS, packed_lists(topk, torch.Generator().manual_seed(73)))
    want = prefill(qd, kvd, cud, ld, idxd)
    assert bool(torch.isfinite(want[0]).all())
    if kind.startswith("decode"):
        cache = kvd if kind == "decode" else on(dev, mla_cache_to_fp8(kv))[0]
        assert dc.same_bits(prefill(qd, cache, cud, ld, idxd), host_loop(qd, cache, ld, idxd))
        return
    if kind == "strided":
        cache, bt = torch.full((len(NQ), NMAX, 640), float("nan"), dtype=dtype, device=dev)[:, :, 32:608], None
        qs, lst = torch.full((TOTAL, H + 1, 584), float("nan"), dtype=dtype, device=dev)[:, 1:, 8:], torch.full((TOTAL, topk + 7), 3, dtype=torch.int32, device=dev)[:, 3:-4]
        cache.copy_(kvd), qs.copy_(qd), lst.copy_(idxd)
    else:
        page = int(kind[4:])
        cache, bt = mr.paged(kv, LENS, page, torch.Generator().manual_seed(5))
        for s, n in enumerate(LENS):
            bt[s, -(-n // page):] = I32_MAX
        (cache, bt), qs, lst = on(dev, cache, bt), qd, idxd
    assert dc.same_bits(prefill(qs, cache, cud, ld, lst, block_table=bt), want), kind


def test_graph_replay_follows_cu_lengths_indices_and_block_table_changed_in_place():
    dev, H, topk, g = dc.dev(), 16, 69, torch.Generator().manual_seed(9)
    q, kv = mr.inputs(TOTAL, H, 1, 1, [1] * TOTAL, BF16, 91, poison=False)[0][:, 0], mr.inputs(len(NQ), 1, 1, NMAX, [NMAX] * 4, BF16, 92)[1]
    pool, bt = mr.paged(kv, [NMAX] * 4, 64, g, spare=1)
    steps = [(NQ, LENS), ((70, 1, 0, 5), (129, 384, 7, 3)), ((1, 1, 1, 1), (300, 0, 65, 33)), (NQ, LENS)]
    cus = [torch.tensor([0] + [sum(n[:s + 1]) for s in range(4)], dtype=torch.int32) for n, _ in steps]
    idxs = [packed_lists(topk, g, n, lens) for n, lens in steps]
    qd, poold, cud, ld, btd, idxd = on(dev, q, pool, cus[0], steps[0][1], bt, idxs[0])
    call = lambda: flash_attention_prefill_mla(qd, poold, cud, ld, idxd, block_table=btd, return_lse=True)      # noqa: E731
    call()                                             # (warm-up: the library is loaded outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = call()
    for (n, lens), cu, idx, table in zip(steps, cus, idxs, (bt, bt.flip(1), bt, bt)):
        cud.copy_(cu), ld.copy_(torch.tensor(lens, dtype=torch.int32)), idxd.copy_(idx), btd.copy_(table)
        graph.replay()
        torch.cuda.synchronize()
        eager = call()
        assert torch.equal(o.view(torch.int16), eager[0].view(torch.int16)) and torch.equal(lse, eager[1]), lens
        assert bool((o[sum(n):] == 0).all()) and bool((lse[:, sum(n):] == float("-inf")).all())


def test_the_packed_indexer_feeds_the_packed_attention():
    """mla_indexer_topk_varlen -> flash_attention_prefill_mla equals, per sequence, mla_indexer_topk -> the host loop of sparse decode calls"""
    dev, H, topk = dc.dev(), 16, 64
    (qi, w), cu, icache, _, _ = tv.case(BF16, 64)
    B, total, g = len(tv.LENS), len(qi), torch.Generator().manual_seed(37)
    q, kv = torch.randn((total, H, mr.D), generator=g).to(BF16), mr.inputs(B, 1, 1, tv.CAP, tv.LENS, BF16, 38)[1]
    qid, wd, cud, ld, icd, qd, kv8 = on(dev, qi, w, cu, tv.LENS, icache, q, mla_cache_to_fp8(kv))
    idx = mla_indexer_topk_varlen(qid, icd, wd, cud, ld, topk=topk)
    got = prefill(qd, kv8, cud, ld, idx)
    per_seq = torch.full_like(idx, -1)
    for s, (a, b) in enumerate(zip(cu.tolist()[:-1], cu.tolist()[1:])):
        if b > a:
            per_seq[a:b] = mla_indexer_topk(qid[None, a:b], icd[s:s + 1], wd[None, a:b], ld[s:s + 1], topk=topk)[0]
    assert torch.equal(idx, per_seq)
    assert dc.same_bits(got, host_loop(qd, kv8, ld, per_seq, nq=tv.COUNTS)) and bool(torch.isfinite(got[0]).all())
