"""CPU tests of the lightning indexer on an e4m3 index-key cache (include/fa2_gfx950.h: fa2_mla_indexer_logits_fp8, fa2_kvcache_append_mla_index_fp8) and
the float64 reference and bar its GPU tests use (tests/test_mla_indexer_fp8_gpu.py).  Nothing here touches a device."""
import functools

import pytest
import torch

import decode_calls as dc
import rocwmma_fattn
import test_mla_indexer as ti
from rocwmma_fattn import FlashAttn, _fa2_lib
from rocwmma_fattn.FlashAttn import mla_index_cache_from_fp8, mla_index_cache_to_fp8, mla_indexer_q_to_fp8
from test_decode_mla import ALIGN, DTYPE, GRID, HEAD_DIM, HEADER, NULLP, SHAPE

P, S2, S3 = dc.HOST, _fa2_lib.strides2, _fa2_lib.strides3
LONG = (torch.bfloat16, 64, 3, "long")      # a length inside the second 512-key chunk: no length of ti.LENS crosses one
CASES = [c + ("",) for c in ti.CASES + [(torch.float16, 48, 1)]] + [LONG]


@functools.lru_cache(maxsize=None)
def case(dtype, H, Nq, kind=""):
    """ti.case's q, keys and weights (kind "long": lengths (530, 3) in a capacity of 600) with the keys quantised into rows of 132 bytes, every dead
    row 0xFF bytes (NaN codes, a NaN scale).  -> q, w, lens, cache uint8 [B, Nmax, 132], and the float64 reference on the codes and scales the cache
    holds with mla_indexer_q_to_fp8's q: logits (-inf beyond pos) and the magnitude k_scale sum_h |w'_h| sum_d |q8_hd k8_sd| the bar scales with."""
    if kind == "long":
        g, lens, nmax = torch.Generator().manual_seed(35), (530, 3), 600
        q, k, w = torch.randn((2, Nq, H, 128), generator=g).to(dtype), torch.randn((2, nmax, 128), generator=g).to(dtype), torch.randn((2, Nq, H), generator=g)
    else:
        (q, k, w, _, _), lens, nmax = ti.case(dtype, H, Nq), ti.LENS, ti.NMAX
    cache = torch.full((len(lens), nmax, 132), 0xFF, dtype=torch.uint8)
    q8, w8 = mla_indexer_q_to_fp8(q, w)
    ref, mag = torch.full((len(lens), Nq, nmax), float("-inf"), dtype=torch.float64), torch.zeros((len(lens), Nq, nmax), dtype=torch.float64)
    for b, n in enumerate(lens):
        cache[b, :n] = mla_index_cache_to_fp8(k[b, :n])
        qd, wd = q8[b].double(), w8[b].double()
        kd, sd = cache[b, :n, :128].contiguous().view(torch.float8_e4m3fn).double(), cache[b, :n, 128:].contiguous().view(torch.float32).double()[:, 0]
        full = sd * (wd[..., None] * torch.einsum("ihd,sd->ihs", qd, kd).clamp_min(0)).sum(1)
        mag[b, :, :n] = sd.abs() * (wd.abs()[..., None] * torch.einsum("ihd,sd->ihs", qd.abs(), kd.abs())).sum(1)
        for i in range(Nq):
            ref[b, i, :max(n - Nq + i + 1, 0)] = full[i, :max(n - Nq + i + 1, 0)]
    return q, w, lens, cache, ref, mag


def check_logits(got, key):
    """|got - ref| <= 2 (128 + H) 2^-24 k_scale sum_h |w'_h| sum_d |q8_hd k8_sd| per live element — section 34's bar on the operands the FP8 kernel
    multiplies (their products are exact in f32 too); exactly -inf beyond pos."""
    _, _, _, _, ref, mag = case(*key)
    live, got = torch.isfinite(ref), got.double().cpu()
    assert torch.equal(got[~live], ref[~live]), "positions beyond pos are exactly -inf"
    err, bar = (got - ref)[live].abs(), 2 * (128 + key[1]) * 2.0 ** -24 * mag[live]
    print("fp8 logits", key, "worst err / bar", float((err / bar.clamp_min(1e-300)).max()))
    assert bool((err <= bar).all())


def test_symbols_are_declared_exported_and_bound():
    lib, text = _fa2_lib.load(), open(HEADER).read()
    for name, nargs in (("fa2_mla_indexer_logits_fp8", 22), ("fa2_kvcache_append_mla_index_fp8", 18), ("fa2_kvcache_append_mla_index_varlen_fp8", 19)):
        assert name + "(" in text and len(_fa2_lib.SYMBOLS[name][1]) == nargs and getattr(lib, name).argtypes == _fa2_lib.SYMBOLS[name][1]
    assert "FA2_KERNEL_HIP_MLA_INDEXER_FP8 = 13" in text and _fa2_lib.FA2_KERNEL_HIP_MLA_INDEXER_FP8 == 13
    assert "#define FA2_DTYPE_E4M3 3" in text and _fa2_lib.FA2_DTYPE_E4M3 == 3
    for name in ("mla_indexer_q_to_fp8", "mla_index_cache_to_fp8", "mla_index_cache_from_fp8", "kvcache_append_mla_index"):
        assert name in FlashAttn.__all__ and getattr(rocwmma_fattn, name) is getattr(FlashAttn, name)


def test_c_codes_in_the_documented_order():
    lib = _fa2_lib.load()
    ok = dict(dtype=1, q=P, k=P, sc=P + 128, w=P, logits=P, lens=P, bt=None, B=1, H=64, Nq=1, D=128, cap=256, page=0, pages=0, qs=S3(8192, 128, 8192),
              ks=S2(33792, 132), ss=S2(8448, 33), ws=S2(64, 64), ls=S2(256, 256), bts=0, stream=None)
    rc = lambda **kw: lib.fa2_mla_indexer_logits_fp8(*dict(ok, **kw).values())      # noqa: E731
    assert rc(B=65536) == GRID and rc(B=65536, dtype=3, k=P + 4, sc=P + 4, ks=S2(0, 128), ss=S2(0, 0)) == GRID      # everything before the grid passed
    for kw in (dict(q=None), dict(k=None), dict(sc=None), dict(ss=None), dict(ks=None), dict(page=64, pages=4), dict(sc=None, B=0, H=8, k=P + 2, dtype=7)):
        assert rc(**kw) == NULLP, kw
    for kw in (dict(B=0), dict(D=0), dict(page=32, bt=P), dict(page=64, pages=0, bt=P), dict(ls=S2(256, -1)), dict(ss=S2(-1, 33)), dict(ss=S2(33, -1)),
               dict(ss=S2(-1, 33), H=8, k=P + 2, dtype=7)):
        assert rc(**kw) == SHAPE, kw
    for kw in (dict(H=8), dict(H=24), dict(D=64), dict(H=24, k=P + 2, dtype=7)):
        assert rc(**kw) == HEAD_DIM, kw
    for kw in (dict(q=P + 2), dict(qs=S3(8192, 132, 8192)), dict(dtype=3, qs=S3(8192, 136, 8192)), dict(w=P + 2), dict(k=P + 2), dict(sc=P + 130), dict(ks=S2(33792, 130)),
               dict(ks=S2(2, 132)), dict(ks=S2(0, 0)), dict(k=P + 1, dtype=7, B=65536)):
        assert rc(**kw) == ALIGN, kw
    assert rc(dtype=2, B=65536) == DTYPE and rc(dtype=7) == DTYPE

    ok = dict(dtype=0, x=P, k=P, sc=P + 128, lens=P, bt=None, B=2, Nnew=3, D=128, cap=256, page=0, pages=0, xs=S2(384, 128), ks=S2(33792, 132), ss=S2(8448, 33), bts=0,
              pow2=0, stream=None)
    rc = lambda **kw: lib.fa2_kvcache_append_mla_index_fp8(*dict(ok, **kw).values())      # noqa: E731
    pk = dict(ok, cu=P, total=0)
    order = ("dtype", "x", "k", "sc", "cu", "lens", "bt", "B", "total", "D", "cap", "page", "pages", "xs", "ks", "ss", "bts", "pow2", "stream")
    rcp = lambda **kw: lib.fa2_kvcache_append_mla_index_varlen_fp8(*(dict(pk, **kw)[n] for n in order))      # noqa: E731
    assert rcp() == 0 and rcp(total=2 ** 31) == GRID, "an empty token buffer launches nothing; everything before the grid passed"
    for f, extra in ((rc, dict(x=None)), (rc, dict(sc=None)), (rc, dict(ss=None)), (rc, dict(page=64, pages=2)), (rcp, dict(cu=None)), (rc, dict(k=None, B=0, D=64))):
        assert f(**extra) == NULLP, extra
    for f, extra in ((rc, dict(B=0)), (rc, dict(Nnew=0)), (rcp, dict(total=-1)), (rc, dict(page=96, bt=P)), (rc, dict(page=64, pages=0, bt=P)), (rc, dict(bts=-1)),
                     (rc, dict(ss=S2(-1, 33))), (rc, dict(Nnew=0, D=64, x=P + 2))):
        assert f(**extra) == SHAPE, extra
    assert rc(D=64) == HEAD_DIM and rc(D=132, x=P + 2, dtype=2) == HEAD_DIM
    for f, extra in ((rc, dict(x=P + 8)), (rc, dict(xs=S2(384, 132))), (rc, dict(xs=S2(384, 0))), (rc, dict(k=P + 2)), (rc, dict(sc=P + 129)), (rc, dict(ks=S2(33792, 130))),
                     (rc, dict(lens=P + 2)), (rcp, dict(cu=P + 2)), (rc, dict(k=P + 2, dtype=2))):
        assert f(**extra) == ALIGN, extra
    assert rc(dtype=2) == DTYPE and rc(dtype=3) == DTYPE


def test_python_argument_checks():
    q, w, lens = torch.zeros(2, 3, 64, 128, dtype=torch.float16), torch.zeros(2, 3, 64), torch.zeros(2, dtype=torch.int32)
    k, bt = torch.zeros(2, 256, 132, dtype=torch.uint8), torch.zeros(2, 4, dtype=torch.int32)
    codes, scales = torch.zeros(4, 64, 128, dtype=torch.uint8), torch.zeros(4, 64)
    bad = [dict(k=k.view(torch.float8_e5m2)), dict(k=k.view(torch.float8_e4m3fnuz)), dict(k=k[..., :128]), dict(k=torch.zeros(2, 256, 136, dtype=torch.uint8)),
           dict(k=(codes, scales[:3]), bt=bt), dict(k=(codes, scales.double()), bt=bt), dict(k=(codes[..., :64], scales), bt=bt), dict(k=(codes, scales, scales), bt=bt),
           dict(k=torch.zeros(2, 256, 133, dtype=torch.uint8)[..., :132]), dict(k=torch.zeros(2, 256, 134, dtype=torch.uint8)[..., 1:133]),
           dict(q=q[:, :, :24], w=w[:, :, :24]), dict(q=q.float()), dict(k=k[:1]), dict(k=k[:, :32], bt=bt), dict()]      # (the last: well-formed, but no ROCm device)
    for kw in bad:
        a = dict(dict(q=q, k=k, w=w, lens=lens, bt=None), **kw)
        for f in (FlashAttn.mla_indexer_logits, FlashAttn.mla_indexer_topk):
            with pytest.raises(ValueError, match="fa2: mla_indexer|fa2: a contiguous|fa2: the page size"):
                f(a["q"], a["k"], a["w"], a["lens"], a["bt"])
    with pytest.raises(ValueError, match="fa2: mla_indexer_logits takes fp16 or bf16"):      # an e4m3 q belongs to an e4m3 cache
        FlashAttn.mla_indexer_logits(q.to(torch.float8_e4m3fn), torch.zeros(2, 256, 128, dtype=torch.float16), w, lens)
    x = torch.zeros(2, 3, 128, dtype=torch.bfloat16)
    for a in ((torch.zeros(2, 256, 128, dtype=torch.bfloat16), x, lens), (k, x.float(), lens), (k, x[..., :64], lens), (k, x[0], lens), (k, x, lens.long()),
              (k[:1], x, lens), (k, x, lens)):
        with pytest.raises(ValueError, match="fa2: kvcache_append_mla_index|fa2: a contiguous"):
            FlashAttn.kvcache_append_mla_index(*a)


@pytest.mark.parametrize("pow2", [False, True])
def test_quantisation_round_trip_and_power_of_two_scales(pow2):
    g = torch.Generator().manual_seed(7)
    x = (torch.randn((64, 128), generator=g) * torch.logspace(-6, 4, 64)[:, None]).to(torch.bfloat16)
    x[3] = 0
    cache = mla_index_cache_to_fp8(x, scale_pow2=pow2)
    scale, amax = cache[:, 128:].contiguous().view(torch.float32).double(), x.double().abs().amax(-1, keepdim=True)
    y, back = x.double() / scale, mla_index_cache_from_fp8(cache, torch.float64) / scale
    ulp = 2.0 ** (y.abs().clamp_min(2.0 ** -6).log2().floor() - 3)
    assert bool(((back - y).abs() <= 0.5 * ulp + 2.0 ** -20 * y.abs()).all()), "within half an e4m3 ulp of x / scale"
    assert float(scale[3]) == 1.0 and bool((scale >= amax / 448 * (1 - 2.0 ** -23)).all())
    if pow2:
        assert bool((torch.frexp(scale)[0] == 0.5).all()) and bool((scale[amax > 0] < 2 * amax[amax > 0] / 448 * (1 + 2.0 ** -23)).all())
    assert torch.equal(mla_index_cache_from_fp8(cache.view(torch.float8_e4m3fn), torch.bfloat16), mla_index_cache_from_fp8(cache, torch.bfloat16))


@pytest.mark.parametrize("key", CASES)
def test_the_reference_in_float32_meets_its_own_bar(key):
    """The formula evaluated in float32 one term at a time, in forward and in reversed head / column order, stays inside the bar the GPU test applies,
    at that test's shapes: the GPU test cannot be failing on its reference."""
    q, w, lens, cache, ref, _ = case(*key)
    (q8, w8), H, Nq = mla_indexer_q_to_fp8(q, w), key[1], key[2]
    for order in (lambda n: range(n), lambda n: reversed(range(n))):
        out = torch.full(ref.shape, float("-inf"))
        for b, n in enumerate(lens):
            k8, sc = cache[b, :n, :128].contiguous().view(torch.float8_e4m3fn).float(), cache[b, :n, 128:].contiguous().view(torch.float32)[:, 0]
            dot = torch.zeros((Nq, H, n))
            for d in order(128):
                dot += q8[b, :, :, d].float()[..., None] * k8[:, d]
            acc = torch.zeros((Nq, n))
            for h in order(H):
                acc += w8[b, :, h, None] * dot[:, h].clamp_min(0)
            for i in range(Nq):
                out[b, i, :max(n - Nq + i + 1, 0)] = (acc * sc)[i, :max(n - Nq + i + 1, 0)]
        check_logits(out, key)
