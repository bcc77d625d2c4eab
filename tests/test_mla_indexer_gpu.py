"""GPU tests of mla_indexer_logits, topk_indices and mla_indexer_topk.  References and the bar: tests/test_mla_indexer.py (float64 logits; a stable sort)."""
import pytest
import torch

import decode_calls as dc
import mla_refs as mr
import test_mla_indexer as ti
from rocwmma_fattn.FlashAttn import flash_attention_decode_mla, mla_indexer_logits, mla_indexer_topk, topk_indices

pytestmark = pytest.mark.gpu
I32_MAX = 2 ** 31 - 1
TOPK_LENS, TOPK_CAP = (0, 1, 7, 2049, 5000), 5003


def on(dev, *ts):
    return tuple(None if t is None else (t if torch.is_tensor(t) else torch.tensor(t, dtype=torch.int32)).to(dev) for t in ts)


def paged_keys(k, lens, seed):
    """The first 320 rows of every sequence in NaN-filled pages of 64 under a shuffled block table; behind the last live page of a sequence: a far id"""
    pool, _, bt = dc.paged(k[:, :320].unsqueeze(2), k[:, :320].unsqueeze(2), lens, 64, torch.Generator().manual_seed(seed))
    for b, n in enumerate(lens):
        bt[b, -(-n // 64):] = I32_MAX
    return pool[:, :, 0], bt


@pytest.mark.parametrize("dtype,H,Nq", ti.CASES)
def test_logits_against_float64(dtype, H, Nq):
    q, k, w, _, _ = ti.case(dtype, H, Nq)
    qd, kd, wd, ld, poold, btd = on(dc.dev(), q, k, w, ti.LENS, *paged_keys(k, ti.LENS, H + Nq))
    got = mla_indexer_logits(qd, kd, wd, ld)
    assert got.shape == (5, Nq, ti.NMAX) and got.dtype == torch.float32
    ti.check_logits(got, dtype, H, Nq)
    paged = mla_indexer_logits(qd, poold, wd, ld, block_table=btd)
    assert paged.shape == (5, Nq, 320) and torch.equal(paged.view(torch.int32), got[:, :, :320].view(torch.int32)), "paged equals contiguous bit for bit"


def rows(kind, Nq):
    g = torch.Generator().manual_seed(len(kind) + Nq)
    x = torch.randn((len(TOPK_LENS), Nq, TOPK_CAP), generator=g)
    if kind == "ties":
        x = torch.randint(0, 3, x.shape, generator=g).float()
    elif kind == "equal":
        x = torch.full(x.shape, 0.5)
    elif kind == "ulp":                                # the top digits are shared: every radix pass has to discriminate
        x = 1 + torch.stack([torch.randperm(TOPK_CAP, generator=g) for _ in range(x.shape[0] * Nq)]).reshape(x.shape).float() * 2.0 ** -23
    elif kind == "special":
        x[torch.rand(x.shape, generator=g) < 0.02] = float("inf")
        x[torch.rand(x.shape, generator=g) < 0.02] = float("-inf")
        x[torch.rand(x.shape, generator=g) < 0.02] = float("nan")
    elif kind == "junk":                               # NaN and +inf beyond pos: never selected
        for b, n in enumerate(TOPK_LENS):
            for i in range(Nq):
                x[b, i, max(n - Nq + i + 1, 0)::2] = float("nan")
                x[b, i, max(n - Nq + i + 1, 0) + 1::2] = float("inf")
    return x


@pytest.mark.parametrize("topk", [1, 8, 64, 2048])
@pytest.mark.parametrize("Nq", [1, 3])
@pytest.mark.parametrize("kind", ["normal", "ties", "equal", "ulp", "special", "junk"])
def test_selection_is_exact(kind, Nq, topk):
    x = rows(kind, Nq)
    xd, ld = on(dc.dev(), x, TOPK_LENS)
    got = topk_indices(xd, ld, topk)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), ti.topk_ref(x, TOPK_LENS, topk)), (kind, Nq, topk)
    assert torch.equal(got, topk_indices(xd, ld, topk)), "two runs, the same bits"


@pytest.mark.parametrize("kind", ["contig", "page64"])
def test_the_step_end_to_end(kind):
    dev, H, Nq, lens = dc.dev(), 16, 3, list(ti.LENS)
    qi, ki, w, _, _ = ti.case(torch.bfloat16, 64, Nq)
    q, kv = mr.inputs(5, H, Nq, 320, lens, torch.bfloat16, 341)
    bt = None
    if kind == "page64":                               # one block table for the latent cache and the index-key cache
        kv, bt = mr.paged(kv, lens, 64, torch.Generator().manual_seed(3))
        pool = torch.full((kv.shape[0], 64, 128), float("nan"), dtype=ki.dtype)
        for b, n in enumerate(lens):
            for j in range(-(-n // 64)):
                pool[bt[b, j]] = ki[b, 64 * j:64 * j + 64]
        ki = pool
    else:
        ki = ki[:, :320]
    qd, kvd, qid, kid, wd, ld, btd = on(dev, q, kv, qi, ki, w, lens, bt)
    idx = mla_indexer_topk(qid, kid, wd, ld, block_table=btd, topk=400)      # topk >= capacity: every position 0 .. pos, then -1
    want = torch.arange(400).expand(5, Nq, 400).clone()
    for b, n in enumerate(lens):
        for i in range(Nq):
            want[b, i, max(n - Nq + i + 1, 0):] = -1
    assert torch.equal(idx.cpu(), want.to(torch.int32))
    sparse = flash_attention_decode_mla(qd, kvd, ld, block_table=btd, indices=idx, num_splits=1, return_lse=True)
    dense = flash_attention_decode_mla(qd, kvd, ld, block_table=btd, num_splits=1, return_lse=True)
    assert dc.same_bits(sparse, dense), "all keys selected, in ascending order: the dense sweep"
    idx64, logits = mla_indexer_topk(qid, kid, wd, ld, block_table=btd, topk=64, return_logits=True)
    sep = mla_indexer_logits(qid, kid, wd, ld, block_table=btd)
    assert torch.equal(logits.view(torch.int32), sep.view(torch.int32)) and torch.equal(idx64, topk_indices(sep, ld, 64))
    assert torch.equal(idx64[2].cpu(), ti.topk_ref(sep[2:3].cpu(), lens[2:3], 64)[0]) and int(idx64[2, 0, -1]) >= 63      # the 300-key sequence: a real selection


def test_graph_replay_follows_lengths_block_table_weights_and_cache_changed_in_place():
    dev, Nq, g = dc.dev(), 3, torch.Generator().manual_seed(12)
    qi, ki, w, _, _ = ti.case(torch.bfloat16, 64, Nq)
    ki = torch.randn((5, 320, 128), generator=g).to(torch.bfloat16)          # (every row finite: the lengths move)
    pool, _, bt = dc.paged(ki.unsqueeze(2), ki.unsqueeze(2), [320] * 5, 64, g, spare=1)
    qid, poold, wd, ld, btd = on(dev, qi, pool[:, :, 0].contiguous(), w, ti.LENS, bt)
    call = lambda: mla_indexer_topk(qid, poold, wd, ld, block_table=btd, topk=64, return_logits=True)      # noqa: E731
    call()                                             # (warm-up: the library is loaded outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        idx, logits = call()
    for lens, table, scale in ((ti.LENS, bt, 1.0), ((320, 64, 0, 300, 129), bt, -0.5), ((320, 64, 0, 300, 129), bt.flip(1), 2.0), (ti.LENS, bt, 1.0)):
        ld.copy_(torch.tensor(lens, dtype=torch.int32)), btd.copy_(table), wd.copy_(w * scale), poold.mul_(scale)
        graph.replay()
        torch.cuda.synchronize()
        eager = call()
        assert torch.equal(idx, eager[0]) and torch.equal(logits.view(torch.int32), eager[1].view(torch.int32)), lens
