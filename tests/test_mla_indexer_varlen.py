"""CPU tests of the packed (prefill) lightning indexer on an e4m3 index-key cache (include/fa2_gfx950.h: fa2_mla_indexer_logits_varlen_fp8,
fa2_topk_indices_varlen) and the packed case and float64 reference its GPU tests use (tests/test_mla_indexer_varlen_gpu.py).  No device is touched."""
import functools

import pytest
import torch

import decode_calls as dc
import rocwmma_fattn
from rocwmma_fattn import FlashAttn, _fa2_lib
from rocwmma_fattn.FlashAttn import mla_index_cache_to_fp8, mla_indexer_q_to_fp8
from test_decode_mla import ALIGN, DTYPE, GRID, HEAD_DIM, HEADER, NULLP, SHAPE

P, S2 = dc.HOST, _fa2_lib.strides2
COUNTS, LENS, CAP, EXTRA = (0, 1, 150, 5, 3), (40, 300, 2090, 3, 129), 2100, 2
# an empty sequence; a decode row; 150 tokens that cross the 128-token block (sequence changes inside both blocks) with a length in the third
# 1 024-key chunk; Nq_s > len_s (negative positions); two rows beyond cu[B]; a capacity that is no multiple of 16


def positions(counts=COUNTS, lens=LENS, extra=EXTRA):
    """-> cu [B + 1] and, per packed row, (sequence, pos) with sequence -1 for a row nobody owns"""
    cu, rows = [0], []
    for s, (c, n) in enumerate(zip(counts, lens)):
        rows += [(s, n - c + i) for i in range(c)]
        cu.append(cu[-1] + c)
    return torch.tensor(cu, dtype=torch.int32), rows + [(-1, -1)] * extra


@functools.lru_cache(maxsize=None)
def case(dtype, H):
    """-> q [total, H, 128] in `dtype` (float8_e4m3fn: mla_indexer_q_to_fp8's pair), w, cu, the cache uint8 [5, 2100, 132] with dead rows of 0xFF
    bytes, and the float64 reference on the stored codes and scales: logits (-inf beyond pos) and the magnitude the bar scales with"""
    g = torch.Generator().manual_seed(36 + H)
    cu, rows = positions()
    q = torch.randn((len(rows), H, 128), generator=g).to(torch.float16 if dtype == torch.float16 else torch.bfloat16)
    w, k = torch.randn((len(rows), H), generator=g), torch.randn((len(LENS), CAP, 128), generator=g).to(torch.bfloat16)
    q8, w8 = (t[0] for t in mla_indexer_q_to_fp8(q[None], w[None]))
    cache = torch.full((len(LENS), CAP, 132), 0xFF, dtype=torch.uint8)
    for b, n in enumerate(LENS):
        cache[b, :n] = mla_index_cache_to_fp8(k[b, :n])
    ref, mag = torch.full((len(rows), CAP), float("-inf"), dtype=torch.float64), torch.zeros((len(rows), CAP), dtype=torch.float64)
    for t, (s, pos) in enumerate(rows):
        if s >= 0 and pos >= 0:
            kd = cache[s, :pos + 1, :128].contiguous().view(torch.float8_e4m3fn).double()
            sd, qd, wd = cache[s, :pos + 1, 128:].contiguous().view(torch.float32).double()[:, 0], q8[t].double(), w8[t].double()
            ref[t, :pos + 1] = sd * (wd[:, None] * (qd @ kd.T).clamp_min(0)).sum(0)
            mag[t, :pos + 1] = sd.abs() * (wd.abs()[:, None] * (qd.abs() @ kd.abs().T)).sum(0)
    return (q8, w8) if dtype == torch.float8_e4m3fn else (q, w), cu, cache, ref, mag


def test_symbols_are_declared_exported_and_bound():
    lib, text = _fa2_lib.load(), open(HEADER).read()
    for name, nargs in (("fa2_mla_indexer_logits_varlen_fp8", 23), ("fa2_topk_indices_varlen", 11)):
        assert name + "(" in text and len(_fa2_lib.SYMBOLS[name][1]) == nargs and getattr(lib, name).argtypes == _fa2_lib.SYMBOLS[name][1]
    assert "FA2_KERNEL_HIP_MLA_INDEXER_PREFILL = 14" in text and _fa2_lib.FA2_KERNEL_HIP_MLA_INDEXER_PREFILL == 14
    for name in ("mla_indexer_logits_varlen", "topk_indices_varlen", "mla_indexer_topk_varlen"):
        assert name in FlashAttn.__all__ and getattr(rocwmma_fattn, name) is getattr(FlashAttn, name)


def test_c_codes_in_the_documented_order():
    lib = _fa2_lib.load()
    ok = dict(dtype=1, q=P, k=P, sc=P + 128, w=P, logits=P, cu=P, lens=P, bt=None, B=1, H=64, total=0, D=128, cap=256, page=0, pages=0, qs=S2(8192, 128),
              ks=S2(33792, 132), ss=S2(8448, 33), ws=64, ls=256, bts=0, stream=None)
    rc = lambda **kw: lib.fa2_mla_indexer_logits_varlen_fp8(*dict(ok, **kw).values())      # noqa: E731
    assert rc() == 0, "an empty token buffer passes every check and launches nothing"
    assert rc(total=65535 * 128 + 1) == GRID and rc(total=2 ** 40, dtype=3, k=P + 4, sc=P + 4, ks=S2(0, 128), ss=S2(0, 0)) == GRID
    for kw in (dict(q=None), dict(sc=None), dict(ss=None), dict(cu=None), dict(page=64, pages=4), dict(cu=None, B=0, H=8, k=P + 2, dtype=7)):
        assert rc(**kw) == NULLP, kw
    for kw in (dict(B=0), dict(total=-1), dict(D=0), dict(page=32, bt=P), dict(ls=-1), dict(ws=-1), dict(ss=S2(-1, 33)), dict(total=-1, H=8, cu=P + 2, dtype=7)):
        assert rc(**kw) == SHAPE, kw
    for kw in (dict(H=8), dict(H=24), dict(D=64), dict(H=24, cu=P + 2, dtype=7)):
        assert rc(**kw) == HEAD_DIM, kw
    for kw in (dict(q=P + 2), dict(qs=S2(8192, 132)), dict(dtype=3, qs=S2(8200, 128)), dict(w=P + 2), dict(k=P + 2), dict(sc=P + 130), dict(ks=S2(2, 132)),
               dict(cu=P + 2), dict(cu=P + 1, dtype=7, total=2 ** 40)):
        assert rc(**kw) == ALIGN, kw
    assert rc(dtype=2, total=2 ** 40) == DTYPE and rc(dtype=7) == DTYPE

    ok = dict(logits=P, idx=P, cu=P, lens=P, B=2, total=0, cap=256, topk=64, ls=256, is_=64, stream=None)
    rc = lambda **kw: lib.fa2_topk_indices_varlen(*dict(ok, **kw).values())      # noqa: E731
    assert rc() == 0 and rc(total=2 ** 31) == GRID
    for kw in (dict(logits=None), dict(idx=None), dict(cu=None), dict(lens=None, B=0)):
        assert rc(**kw) == NULLP, kw
    for kw in (dict(B=0), dict(total=-1), dict(cap=0), dict(topk=0), dict(ls=-1), dict(is_=-1), dict(topk=0, cu=P + 2)):
        assert rc(**kw) == SHAPE, kw
    for kw in (dict(logits=P + 2), dict(cu=P + 2), dict(lens=P + 1, total=2 ** 31)):
        assert rc(**kw) == ALIGN, kw


def test_python_argument_checks():
    q, w = torch.zeros(6, 64, 128, dtype=torch.float16), torch.zeros(6, 64)
    cu, lens, k = torch.tensor([0, 2, 6], dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 256, 132, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uniform mla_indexer_logits"):          # a 16-bit index-key cache names the uniform call
        FlashAttn.mla_indexer_logits_varlen(q, torch.zeros(2, 256, 128, dtype=torch.float16), w, cu, lens)
    bad = [dict(q=q[None]), dict(w=w[None]), dict(q=q.float()), dict(w=w.double()), dict(q=q[:, :24], w=w[:, :24]), dict(w=w[:5]), dict(cu=cu.long()),
           dict(cu=cu[:1]), dict(cu=cu.view(1, 3)), dict(lens=lens[:1]), dict(k=k[..., :128]), dict(q=q.requires_grad_()), dict(topk=0), dict()]
    for kw in bad:                                                                # (the last: well-formed, but no ROCm device)
        a = dict(dict(q=q.detach(), k=k, w=w, cu=cu, lens=lens, topk=8), **kw)
        fs = (FlashAttn.mla_indexer_topk_varlen,) if "topk" in kw else (FlashAttn.mla_indexer_logits_varlen, FlashAttn.mla_indexer_topk_varlen)
        for f in fs:
            with pytest.raises(ValueError, match="fa2: "):
                f(a["q"], a["k"], a["w"], a["cu"], a["lens"], **({"topk": a["topk"]} if f is FlashAttn.mla_indexer_topk_varlen else {}))
    x = torch.zeros(6, 256)
    for a in ((x[None], cu, lens, 8), (x.double(), cu, lens, 8), (x, cu.long(), lens, 8), (x, cu, lens.long(), 8), (x, cu, lens, 0), (x.requires_grad_(), cu, lens, 8),
              (x.detach(), cu, lens, 8)):
        with pytest.raises(ValueError, match="fa2: "):
            FlashAttn.topk_indices_varlen(*a)
