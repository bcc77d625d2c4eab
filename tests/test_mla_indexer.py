"""CPU tests of the lightning indexer (include/fa2_gfx950.h: fa2_mla_indexer_logits, fa2_topk_indices) and the float64 reference and bar its GPU tests
use (tests/test_mla_indexer_gpu.py).  Nothing here touches a device."""
import functools

import pytest
import torch

import decode_calls as dc
import rocwmma_fattn
from rocwmma_fattn import FlashAttn, _fa2_lib
from test_decode_mla import ALIGN, DTYPE, GRID, HEAD_DIM, HEADER, NULLP, SHAPE

P, S2, S3 = dc.HOST, _fa2_lib.strides2, _fa2_lib.strides3
LENS, NMAX, D = (0, 2, 300, 129, 65), 323, 128      # the sparse decode test's lengths; a capacity that is no multiple of the 16-key tile
CASES = [(dtype, H, Nq) for dtype in (torch.float16, torch.bfloat16) for H in (16, 32, 64) for Nq in (1, 3)]


@functools.lru_cache(maxsize=None)
def case(dtype, H, Nq):
    """q_idx [5, Nq, H, 128], the index-key cache [5, 323, 128] with NaN in every row at or beyond its length, weights of both signs, and the float64
    reference: logits (-inf beyond pos) and, per element, the magnitude sum_h |w_h| sum_d |q_hd k_sd| the bar scales with."""
    g = torch.Generator().manual_seed(34 + H + Nq)
    q, k, w = torch.randn((5, Nq, H, D), generator=g).to(dtype), torch.randn((5, NMAX, D), generator=g).to(dtype), torch.randn((5, Nq, H), generator=g)
    ref, mag = torch.full((5, Nq, NMAX), float("-inf"), dtype=torch.float64), torch.zeros((5, Nq, NMAX), dtype=torch.float64)
    for b, n in enumerate(LENS):
        k[b, n:] = float("nan")
        qd, kd, wd = q[b].double(), k[b, :n].double(), w[b].double()
        full = (wd[..., None] * torch.einsum("ihd,sd->ihs", qd, kd).clamp_min(0)).sum(1)
        mag[b, :, :n] = (wd.abs()[..., None] * torch.einsum("ihd,sd->ihs", qd.abs(), kd.abs())).sum(1)
        for i in range(Nq):
            ref[b, i, :max(n - Nq + i + 1, 0)] = full[i, :max(n - Nq + i + 1, 0)]
    return q, k, w, ref, mag


def check_logits(got, dtype, H, Nq):
    """|got - ref| <= 2 (128 + H) 2^-24 sum_h |w_h| sum_d |q_hd k_sd| per live element — f32 accumulation of exact products over 128 + H terms, the
    factor 2 for a matrix pipe that may truncate its adds; exactly -inf beyond pos."""
    _, _, _, ref, mag = case(dtype, H, Nq)
    live = torch.isfinite(ref)
    got = got.double().cpu()
    assert torch.equal(got[~live], ref[~live]), "positions beyond pos are exactly -inf"
    err, bar = (got - ref)[live].abs(), 2 * (D + H) * 2.0 ** -24 * mag[live]
    print("logits", dtype, H, Nq, "worst err / bar", float((err / bar.clamp_min(1e-300)).max()))
    assert bool((err <= bar).all())


def topk_ref(logits, lens, topk):
    """Stable sort by (-value, position) over [0, pos] with NaN as -inf, take topk, sort ascending, pad with -1."""
    B, Nq, _ = logits.shape
    out = torch.full((B, Nq, topk), -1, dtype=torch.int32)
    for b in range(B):
        for i in range(Nq):
            n = max(lens[b] - Nq + i + 1, 0)
            v = logits[b, i, :n].clone()
            v[v.isnan()] = float("-inf")
            keep = torch.sort(v, descending=True, stable=True).indices[:topk].sort().values
            out[b, i, :len(keep)] = keep.to(torch.int32)
    return out


def test_symbols_are_declared_exported_and_bound():
    lib, text = _fa2_lib.load(), open(HEADER).read()
    for name, nargs in (("fa2_mla_indexer_logits", 20), ("fa2_topk_indices", 10)):
        assert name + "(" in text and len(_fa2_lib.SYMBOLS[name][1]) == nargs and getattr(lib, name).argtypes == _fa2_lib.SYMBOLS[name][1]
    assert "FA2_KERNEL_HIP_MLA_INDEXER = 12" in text and _fa2_lib.FA2_KERNEL_HIP_MLA_INDEXER == 12
    for name in ("mla_indexer_logits", "topk_indices", "mla_indexer_topk"):
        assert name in FlashAttn.__all__ and getattr(rocwmma_fattn, name) is getattr(FlashAttn, name)


def test_c_codes_in_the_documented_order():
    lib = _fa2_lib.load()
    ok = dict(dtype=0, q=P, k=P, w=P, logits=P, lens=P, bt=None, B=1, H=64, Nq=1, D=128, cap=256, page=0, pages=0, qs=S3(8192, 128, 8192), ks=S2(32768, 128),
              ws=S2(64, 64), ls=S2(256, 256), bts=0, stream=None)
    rc = lambda **kw: lib.fa2_mla_indexer_logits(*dict(ok, **kw).values())      # noqa: E731
    assert rc(B=65536) == GRID and rc(Nq=65536, ws=S2(0, 64)) == GRID            # well-formed but for the grid: everything before it passed
    for kw in (dict(q=None), dict(k=None), dict(w=None), dict(logits=None), dict(lens=None), dict(qs=None), dict(ks=None), dict(ws=None), dict(ls=None),
               dict(page=64, pages=4), dict(q=None, B=0, H=8, k=P + 2, dtype=2)):
        assert rc(**kw) == NULLP, kw
    for kw in (dict(B=0), dict(H=0), dict(Nq=0), dict(D=0), dict(cap=0), dict(page=32, bt=P), dict(page=64, pages=0, bt=P), dict(page=64, pages=1, bt=P, cap=2 ** 25),
               dict(ws=S2(-1, 64)), dict(ls=S2(256, -1)), dict(bts=-1), dict(B=0, H=8, k=P + 2, dtype=2)):
        assert rc(**kw) == SHAPE, kw
    for kw in (dict(H=8), dict(H=24), dict(H=80), dict(D=64), dict(D=136), dict(H=8, k=P + 2, dtype=2)):
        assert rc(**kw) == HEAD_DIM, kw
    for kw in (dict(q=P + 2), dict(k=P + 8), dict(w=P + 2), dict(logits=P + 1), dict(lens=P + 2), dict(bt=P + 2, page=64, pages=1), dict(qs=S3(8192, 132, 8192)),
               dict(ks=S2(4, 128)), dict(ks=S2(0, 0)), dict(ks=S2(0, 132)), dict(k=P + 2, dtype=2, B=65536)):
        assert rc(**kw) == ALIGN, kw
    assert rc(dtype=2, B=65536) == DTYPE and rc(w=P + 4, logits=P + 4, lens=P + 4, B=65536, H=48, page=128, pages=1, bt=P + 4) == GRID      # 4 bytes are enough

    ok = dict(logits=P, idx=P, lens=P, B=1, Nq=1, cap=256, topk=64, ls=S2(256, 256), ids=S2(64, 64), stream=None)
    rc = lambda **kw: lib.fa2_topk_indices(*dict(ok, **kw).values())             # noqa: E731
    assert rc(B=2 ** 16, Nq=2 ** 15) == GRID
    for kw in (dict(logits=None), dict(idx=None), dict(lens=None), dict(ls=None), dict(ids=None), dict(logits=None, topk=0, idx=P + 1)):
        assert rc(**kw) == NULLP, kw
    for kw in (dict(B=0), dict(Nq=0), dict(cap=0), dict(topk=0), dict(topk=-1), dict(topk=2 ** 31 - 64), dict(cap=2 ** 31 - 64), dict(ls=S2(-1, 256)),
               dict(ids=S2(64, -1)), dict(topk=0, idx=P + 1, B=2 ** 16, Nq=2 ** 15)):
        assert rc(**kw) == SHAPE, kw
    for kw in (dict(logits=P + 2), dict(idx=P + 1), dict(lens=P + 3), dict(idx=P + 2, B=2 ** 16, Nq=2 ** 15)):
        assert rc(**kw) == ALIGN, kw
    assert rc(topk=2 ** 31 - 65, cap=2 ** 31 - 65, logits=P + 4, B=2 ** 16, Nq=2 ** 15) == GRID


def test_python_argument_checks():
    q, k, w, lens = torch.zeros(2, 3, 64, 128, dtype=torch.float16), torch.zeros(2, 256, 128, dtype=torch.float16), torch.zeros(2, 3, 64), torch.zeros(2, dtype=torch.int32)
    bt = torch.zeros(2, 4, dtype=torch.int32)
    bad = [dict(q=q.float()), dict(k=k.bfloat16()), dict(w=w.half()), dict(q=q[0]), dict(k=k[0]), dict(w=w[0]), dict(q=q[..., :64], k=k[..., :64]), dict(k=k[..., :64]),
           dict(k=torch.zeros(2, 256, 576, dtype=torch.float16)), dict(q=q[:, :, :24], w=w[:, :, :24]), dict(q=q[:, :, :8], w=w[:, :, :8]), dict(w=w[:, :2]),
           dict(k=k.unsqueeze(2).expand(2, 256, 2, 128)), dict(k=k[:1]), dict(lens=lens.long()), dict(lens=lens[:1]), dict(lens=[1, 2]), dict(bt=bt),
           dict(k=torch.zeros(4, 32, 128, dtype=torch.float16), bt=bt), dict(k=k[:, :64], bt=bt.long()), dict(k=k[:, :64], bt=bt[:1]),
           dict(q=q.clone().requires_grad_()), dict(w=w.clone().requires_grad_()), dict()]      # (the last: well-formed, but not on a ROCm device)
    for kw in bad:
        a = dict(dict(q=q, k=k, w=w, lens=lens, bt=None), **kw)
        for f in (FlashAttn.mla_indexer_logits, FlashAttn.mla_indexer_topk):
            with pytest.raises(ValueError, match="fa2: mla_indexer|fa2: block_table|fa2: a contiguous|fa2: the page size"):
                f(a["q"], a["k"], a["w"], a["lens"], a["bt"])
    for topk in (0, -1, 2.0, True, None, 2 ** 31 - 64):
        with pytest.raises(ValueError, match="topk"):
            FlashAttn.mla_indexer_topk(q, k, w, lens, topk=topk)
        with pytest.raises(ValueError, match="topk"):
            FlashAttn.topk_indices(torch.zeros(2, 3, 256), lens, topk)
    logits = torch.zeros(2, 3, 256)
    for a in ((logits.half(), lens), (logits[0], lens), (logits, lens.long()), (logits, lens[:1]), (logits.clone().requires_grad_(), lens), (logits, lens)):
        with pytest.raises(ValueError, match="fa2: topk_indices"):
            FlashAttn.topk_indices(*a, 8)


@pytest.mark.parametrize("dtype,H,Nq", CASES)
def test_the_reference_in_float32_meets_its_own_bar(dtype, H, Nq):
    """The float64 formula evaluated in float32 one term at a time, in forward and in reversed head / column order, stays inside the bar the GPU test
    applies, at that test's shapes: the bar is one a correct f32 evaluation meets whatever its summation order."""
    q, k, w, _, _ = case(dtype, H, Nq)
    for order in (lambda n: range(n), lambda n: reversed(range(n))):
        out = torch.full((5, Nq, NMAX), float("-inf"))
        for b, n in enumerate(LENS):
            dot = torch.zeros((Nq, H, n))
            for d in order(D):
                dot += q[b, :, :, d].float()[..., None] * k[b, :n, d].float()
            acc = torch.zeros((Nq, n))
            for h in order(H):
                acc += w[b, :, h, None] * dot[:, h].clamp_min(0)
            for i in range(Nq):
                out[b, i, :max(n - Nq + i + 1, 0)] = acc[i, :max(n - Nq + i + 1, 0)]
        check_logits(out, dtype, H, Nq)
