"""GPU tests of flash_attention_decode_mla(indices=).  Reference: each token's valid entries, in list order, gathered on the CPU for mla_refs.refs; unnamed rows NaN."""
import functools

import pytest
import torch

import decode_calls as dc
import decode_refs as dr
import mla_refs as mr
import test_kvappend_mla_gpu as fused
from rocwmma_fattn.FlashAttn import flash_attention_decode_mla, kvcache_append_mla, merge_attention

pytestmark = pytest.mark.gpu
F16, BF16, LN2, I32_MAX = torch.float16, torch.bfloat16, 0.6931471805599453, 2 ** 31 - 1
NMAX, LENS = 320, (0, 2, 300, 129, 65)     # no key; shorter than Nq = 3 (dead rows); ten tiles over five pages of 64; one key into a fifth tile; a third
SHAPES = ((1, 1, 1), (16, 3, 31), (17, 1, 32), (64, 3, 33), (128, 1, 69), (128, 3, 200), (17, 3, 69), (16, 1, 200))


def lists(B, Nq, lens, topk, g):
    idx = torch.empty((B, Nq, topk), dtype=torch.int64)
    for b, n in enumerate(lens):
        for i in range(Nq):
            pos = n - Nq + i
            junk = torch.tensor([-1, min(pos + 1, n), n, NMAX + 7, -2 ** 31, I32_MAX, -5])
            row = junk[torch.randint(0, len(junk), (topk,), generator=g)]
            if pos >= 0:
                row = torch.where(torch.rand(topk, generator=g) < 0.6, torch.randint(0, pos + 1, (topk,), generator=g), row)
                row[:2] = int(torch.randint(0, pos + 1, (1,), generator=g))
            idx[b, i] = row
    if topk > 1:
        idx[B - 2, 0, (topk + 1) // 2:] = -1
    idx[B - 1, Nq - 1] = -1
    return idx.to(torch.int32)


def gathered(q, kv, idx, lens):
    B, Nq, H, _ = q.shape
    rows = [[j for j in idx[b, i].tolist() if 0 <= j <= lens[b] - Nq + i] for b in range(B) for i in range(Nq)]
    keys = torch.zeros((B * Nq, max(1, max(map(len, rows))), mr.D), dtype=kv.dtype)
    for r, js in enumerate(rows):
        keys[r, :len(js)] = kv[r // Nq, js]
    return rows, q.reshape(B * Nq, 1, H, mr.D), keys, [len(js) for js in rows]


def check(o, lse2, refs, glens, dtype, tag):
    B, Nq, H, _ = o.shape
    dr.check(o.reshape(B * Nq, 1, H, mr.DV), lse2.permute(0, 2, 1).reshape(B * Nq, H, 1), refs, glens, dc.code(dtype), tag)


@functools.lru_cache(maxsize=None)
def case(s, dtype):
    H, Nq, topk = SHAPES[s]
    q, kv = mr.inputs(len(LENS), H, Nq, NMAX, LENS, dtype, 400 + s, poison=False)
    idx = lists(len(LENS), Nq, LENS, topk, torch.Generator().manual_seed(500 + s))
    named = torch.zeros(kv.shape[:2], dtype=torch.bool)
    for r, js in enumerate(gathered(q, kv, idx, LENS)[0]):
        named[r // Nq, js] = True
    kv[~named] = float("nan")
    _, gq, gk, glens = gathered(q, kv, idx, LENS)
    assert sum(n > 0 for n in glens) > len(glens) // 2 and 0 in glens
    return q, kv, idx, glens, mr.refs(gq, gk, glens, dc.code(dtype))


def sparse(q, kv, lens, idx, num_splits, block_table=None):
    o, lse = flash_attention_decode_mla(q, kv, lens, block_table=block_table, indices=idx, num_splits=num_splits, return_lse=True)
    return o, lse / LN2


def on(dev, *ts):
    return tuple(None if t is None else (t if torch.is_tensor(t) else torch.tensor(t, dtype=torch.int32)).to(dev) for t in ts)


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("s", range(len(SHAPES)))
def test_lists_and_rows(s, dtype):
    q, kv, idx, glens, refs = case(s, dtype)
    qd, kvd, idxd, ld = on(dc.dev(), q, kv, idx, LENS)
    for split in (1, 2, 5):                            # topk 69 under 5: more parts than tiles; row (3, 0) leaves whole parts without a valid entry
        check(*sparse(qd, kvd, ld, idxd, split), refs, glens, dtype, ("sparse", SHAPES[s], split))
    if s == 5:                                         # two halves of a list through merge_attention: the whole list, under the same bars
        a, b = (flash_attention_decode_mla(qd, kvd, ld, indices=idxd[:, :, lo:lo + 100], return_lse=True) for lo in (0, 100))
        o, lse = merge_attention([a[0], b[0]], [a[1], b[1]], BNHD_fmt=True)
        check(o, lse / LN2, refs, glens, dtype, "merged")


@pytest.mark.parametrize("kind", ["page64", "page128", "dense", "strided"])
def test_bit_for_bit(kind):
    dev, H, Nq, topk, lens, dtype = dc.dev(), 17, 3, 69, [300, 129, 65, 0], F16 if kind == "page64" else BF16
    q, kv = mr.inputs(4, H, Nq, 384, lens, dtype, 77)
    kv[1, :128] = kv[0, :128]
    qd, kvd, idxd, ld = on(dev, q, kv, lists(4, Nq, lens, topk, torch.Generator().manual_seed(8)), lens)
    if kind == "dense":
        idxd = torch.arange(384, dtype=torch.int32, device=dev).expand(4, Nq, 384)
        dense = flash_attention_decode_mla(qd, kvd, ld, num_splits=1, return_lse=True)
        assert dc.same_bits(sparse(qd, kvd, ld, idxd, 1), (dense[0], dense[1] / LN2))
        return
    if kind == "strided":
        cache = torch.full((4, 384, 640), float("nan"), dtype=dtype, device=dev)[:, :, 32:608]
        lst, bt = torch.full((4, 5, topk + 7), 3, dtype=torch.int32, device=dev)[:, 1:4, 3:-4], None
        cache.copy_(kvd), lst.copy_(idxd)
    else:
        page = int(kind[4:])
        cache, bt = mr.paged(kv, lens, page, torch.Generator().manual_seed(5))
        cache[bt[1, 0]] = float("nan")
        bt[1, 0] = bt[0, 0]
        for b, n in enumerate(lens):
            bt[b, -(-n // page):] = I32_MAX
        cache, bt, lst = *on(dev, cache, bt), idxd
    for split in (1, 2):
        got = sparse(qd, cache, ld, lst, split, block_table=bt)
        assert dc.same_bits(got, sparse(qd, kvd, ld, idxd, split)) and bool(torch.isfinite(got[0]).all()), (kind, split)


def test_graph_replay_follows_indices_lengths_and_block_table_changed_in_place():
    dev, H, Nq, topk, g = dc.dev(), 16, 3, 69, torch.Generator().manual_seed(9)
    q, kv = mr.inputs(3, H, Nq, NMAX, [NMAX] * 3, BF16, 91)
    pool, bt = mr.paged(kv, [NMAX] * 3, 64, g, spare=1)
    lens_a, lens_b = [300, 65, 33], [129, 0, 320]
    idx_a, idx_b = lists(3, Nq, lens_a, topk, g), lists(3, Nq, lens_b, topk, g)
    qd, poold, ld, btd, idxd = on(dev, q, pool, lens_a, bt, idx_a)
    call = lambda: flash_attention_decode_mla(qd, poold, ld, block_table=btd, indices=idxd, return_lse=True, num_splits=2)      # noqa: E731
    call()                                             # (warm-up: the library is loaded outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, lse = call()
    for lens, idx, table in ((lens_a, idx_a, bt), (lens_b, idx_b, bt), (lens_b, idx_b, bt.flip(1)), (lens_a, idx_b, bt), (lens_a, idx_a, bt)):
        ld.copy_(torch.tensor(lens, dtype=torch.int32))
        idxd.copy_(idx), btd.copy_(table)
        graph.replay()
        torch.cuda.synchronize()
        eager = call()
        assert torch.equal(o.view(torch.int16), eager[0].view(torch.int16)) and torch.equal(lse, eager[1]), lens


@pytest.mark.parametrize("kind", ["contig", "page64"])
def test_fused_is_append_then_sparse_decode(kind):
    Nq = 2
    q, kv_c, k_pe, lens, before, bt, cos, sin, q_ref, kv_ref = fused.fused_case(BF16, Nq, kind, False, 300 + Nq)
    idx = lists(3, Nq, lens, 69, torch.Generator().manual_seed(2))
    idx[2, Nq - 1, 0] = lens[2] - 1                    # (lists() emptied this row) its own new token: the row the append has just written
    qd, kc, pe, ld, c1, c2, idxd, btd, cosd, sind = on(dc.dev(), q, kv_c, k_pe, lens, before, before, idx, bt, cos, sin)
    kw = dict(block_table=btd, rotary_cos=cosd, rotary_sin=sind, rotary_interleaved=False)
    o1, l1 = flash_attention_decode_mla(qd, c1, ld, return_lse=True, num_splits=2, scale=mr.SCALE, kv_c=kc, k_pe=pe, indices=idxd, **kw)
    q_out = kvcache_append_mla(c2, kc, pe, ld, q=qd, **kw)
    o2, l2 = flash_attention_decode_mla(q_out, c2, ld, block_table=btd, return_lse=True, num_splits=2, scale=mr.SCALE, indices=idxd)
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)) and torch.equal(l1, l2), "fused == append, then sparse decode on q_out"
    _, gq, gk, glens = gathered(q_ref, kv_ref, idx, lens)
    check(o1, l1 / LN2, mr.refs(gq, gk, glens, dc.code(BF16)), glens, BF16, ("fused", kind))
