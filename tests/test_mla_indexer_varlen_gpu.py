"""GPU tests of the packed (prefill) lightning indexer: mla_indexer_logits_varlen, topk_indices_varlen, mla_indexer_topk_varlen.  The packed case, the
float64 reference and the bar: tests/test_mla_indexer_varlen.py and section 35's bar (tests/test_mla_indexer_fp8.py)."""
import pytest
import torch

import decode_calls as dc
import test_mla_indexer_fp8_gpu as t8g
import test_mla_indexer_varlen as tv
from rocwmma_fattn.FlashAttn import (kvcache_append_mla_index, mla_index_cache_to_fp8, mla_indexer_logits, mla_indexer_logits_varlen, mla_indexer_topk,
                                     mla_indexer_topk_varlen, topk_indices_varlen)
from test_mla_indexer_gpu import on

pytestmark = pytest.mark.gpu
bits = lambda t: t.view(torch.int32)      # noqa: E731


def per_sequence(f, q, cache, w, cu, lens, width):
    """The uniform operator on each sequence's slice -> the packed rows it owns (rows nobody owns: `fill`-free, left out) as {row: value}"""
    out, cu = {}, cu.tolist()
    for s in range(len(cu) - 1):
        if cu[s + 1] > cu[s]:
            got = f(q[cu[s]:cu[s + 1]][None], cache[s:s + 1], w[cu[s]:cu[s + 1]][None], lens[s:s + 1])
            assert got.shape == (1, cu[s + 1] - cu[s], width)
            out.update({cu[s] + i: got[0, i] for i in range(cu[s + 1] - cu[s])})
    return out


@pytest.mark.parametrize("H", [16, 64])
@pytest.mark.parametrize("dtype", [torch.float8_e4m3fn, torch.bfloat16, torch.float16])
def test_logits_against_float64_the_uniform_call_and_every_layout(dtype, H):
    (q, w), cu, cache, ref, mag = tv.case(dtype, H)
    padded = torch.cat([cache, torch.full((len(tv.LENS), 12, 132), 0xFF, dtype=torch.uint8)], 1)      # 33 whole pages of 64 for the paged forms
    pool, bt = t8g.paged_rows(padded, tv.LENS, H)
    qd, wd, cud, ld, cd, poold, bufd, btd = on(dc.dev(), q, w, cu, tv.LENS, cache, pool, t8g.blocks(pool), bt)
    got = mla_indexer_logits_varlen(qd, cd, wd, cud, ld)
    assert got.shape == ref.shape and got.dtype == torch.float32
    live, g64 = torch.isfinite(ref), got.double().cpu()
    assert torch.equal(g64[~live], ref[~live]), "exactly -inf beyond pos, at negative positions and in rows nobody owns"
    err, bar = (g64 - ref)[live].abs(), 2 * (128 + H) * 2.0 ** -24 * mag[live]
    print("packed logits", dtype, H, "worst err / bar", float((err / bar.clamp_min(1e-300)).max()))
    assert bool((err <= bar).all())
    for t, row in per_sequence(mla_indexer_logits, qd, cd, wd, cu, ld, tv.CAP).items():
        assert torch.equal(bits(got[t]), bits(row)), "row %d equals the uniform call on its sequence bit for bit" % t
    for name, k in (("rows", poold), ("blocks", t8g.block_views(bufd))):
        paged = mla_indexer_logits_varlen(qd, k, wd, cud, ld, block_table=btd)
        assert paged.shape[1] == 33 * 64 and torch.equal(bits(paged[:, :tv.CAP]), bits(got)) and bool((paged[:, tv.CAP:] == float("-inf")).all()), name


@pytest.mark.parametrize("topk", [1, 64, 2048])
def test_selection_is_the_stable_sort_per_row(topk):
    (q, w), cu, cache, _, _ = tv.case(torch.bfloat16, 64)
    qd, wd, cud, ld, cd = on(dc.dev(), q, w, cu, tv.LENS, cache)
    logits = mla_indexer_logits_varlen(qd, cd, wd, cud, ld)
    got, lg = topk_indices_varlen(logits, cud, ld, topk).cpu(), logits.cpu()
    want = torch.full(got.shape, -1, dtype=torch.int32)
    for t, (s, pos) in enumerate(tv.positions()[1]):
        if s >= 0 and pos >= 0:
            keep = torch.sort(lg[t, :pos + 1], descending=True, stable=True)[1][:topk].sort()[0]
            want[t, :len(keep)] = keep.to(torch.int32)
    assert torch.equal(got, want)


def test_the_packed_step_appends_selects_and_replays_in_a_graph():
    dev, g = dc.dev(), torch.Generator().manual_seed(36)
    (q, w), cu, _, _, _ = tv.case(torch.bfloat16, 64)
    k16, new = torch.randn((5, tv.CAP, 128), generator=g).to(torch.bfloat16), torch.randn((len(q), 128), generator=g).to(torch.bfloat16)
    qd, wd, cud, ld, newd, cached = on(dev, q, w, cu, tv.LENS, new, mla_index_cache_to_fp8(k16))

    def step():
        kvcache_append_mla_index(cached, newd, ld, cu_seqlens=cud)
        return mla_indexer_topk_varlen(qd, cached, wd, cud, ld, topk=64, return_logits=True)

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        idx, logits = step()
    for counts, lens in ((tv.COUNTS, tv.LENS), ((3, 0, 100, 50, 6), (3, 7, 2100, 50, 1025)), ((1, 1, 1, 1, 1), (1, 2100, 64, 0, 1024)), (tv.COUNTS, tv.LENS)):
        cu = tv.positions(counts, lens)[0]
        cud.copy_(cu)
        ld.copy_(torch.tensor(lens, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        assert torch.equal(idx, eager[0]) and torch.equal(bits(logits), bits(eager[1])), lens
        for t, row in per_sequence(lambda *a: mla_indexer_topk(*a, topk=64), qd, cached, wd, cu, ld, 64).items():
            assert torch.equal(idx[t], row), (lens, t)
        assert bool((idx[int(cu[-1]):] == -1).all()) and bool((logits[int(cu[-1]):] == float("-inf")).all())
