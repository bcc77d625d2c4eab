"""CPU tests of the KV-cache append (include/fa2_gfx950.h: fa2_kvcache_append, fa2_kvappend_slot, fa2_rotary_eval; kvcache_append and the k / v / rotary_*
keywords of flash_attention_decode): the symbols, the shared position function exhaustively, the shared rotary arithmetic against float64 under a bar
derived from one rounding of an f32 value, every validation code of the new entry and the order they are checked in, and the operator's argument checks.
Nothing here touches a device: every rejected call returns before the launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import decode_calls as dc
from conftest import ROOT
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention_decode, kvcache_append
from kvappend_refs import rotary_bar, rotary_ref64

HEADER = os.path.join(ROOT, "include", "fa2_gfx950.h")
SYMBOLS = ("fa2_kvcache_append", "fa2_kvappend_slot", "fa2_rotary_eval")
OK, NULLP, SHAPE, HEAD_DIM, ALIGN, DTYPE, SCALE, GRID = 0, -1, -2, -3, -4, -5, -6, -7
F16, BF16, F32 = _fa2_lib.FA2_DTYPE_F16, _fa2_lib.FA2_DTYPE_BF16, _fa2_lib.FA2_DTYPE_F32
C16, C8 = _fa2_lib.FA2_CACHE_16BIT, _fa2_lib.FA2_CACHE_E4M3
E4M3 = torch.float8_e4m3fn


def test_symbols_are_declared_exported_and_bound():
    lib = _fa2_lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _fa2_lib.SYMBOLS, name
        assert getattr(lib, name).argtypes == _fa2_lib.SYMBOLS[name][1]
    assert len(_fa2_lib.SYMBOLS["fa2_kvcache_append"][1]) == 37
    # the decode section no longer lists the append under "Not here", and points at the new section
    full = open(HEADER).read()
    assert "Not here: appending" not in full and "fa2_kvcache_append (its own section" in full


def test_slot_exhaustively():
    """-1, or len - Nnew + i inside [0, capacity_keys): never anything else; strictly increasing in i over the written tokens."""
    lib = _fa2_lib.load()
    pos = ctypes.c_int64()
    for cap in (0, 1, 64, 128, 256):
        for nnew in (1, 2, 3, 4, 5, 6, 130):
            for ln in range(-2, 301):
                last = -1
                for i in range(nnew):
                    assert lib.fa2_kvappend_slot(ln, cap, nnew, i, ctypes.byref(pos)) == OK
                    p, want = pos.value, ln - nnew + i
                    if 0 <= want < cap:
                        assert p == want, (ln, cap, nnew, i, p)
                        assert p > last
                        last = p
                    else:
                        assert p == -1, (ln, cap, nnew, i, p)
    assert _fa2_lib.kvappend_slot(65, 1024, 3, 0) == 62 and _fa2_lib.kvappend_slot(2, 1024, 3, 0) == -1 and _fa2_lib.kvappend_slot(1025, 1024, 1, 0) == -1
    assert lib.fa2_kvappend_slot(1, 1, 1, 0, None) == NULLP
    for (ln, cap, nnew, i) in ((1, -1, 1, 0), (1, 1, 0, 0), (1, 1, 1, -1), (1, 1, 1, 1)):
        assert lib.fa2_kvappend_slot(ln, cap, nnew, i, ctypes.byref(pos)) == SHAPE


def _rotary_eval(x, cos, sin, rot, inter, dt):
    lib = _fa2_lib.load()
    xb = x.contiguous()
    y = torch.empty_like(xb)
    c, s = (np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (cos, sin))
    fp = ctypes.POINTER(ctypes.c_float)
    rc = lib.fa2_rotary_eval(F16 if dt == torch.float16 else BF16, xb.data_ptr(), c.ctypes.data_as(fp), s.ctypes.data_as(fp), x.numel(), rot, int(inter),
                             y.data_ptr())
    assert rc == OK
    return y


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("inter", [True, False], ids=["gptj", "neox"])
def test_rotary_eval_against_float64(dt, inter):
    g = torch.Generator().manual_seed(5)
    for D in (64, 128):
        for rot in (16, 32, D):
            for trial in range(8):
                x = (torch.randn(D, generator=g) * (4.0 if trial % 2 else 1.0)).to(dt)
                ang = torch.rand(rot // 2, generator=g, dtype=torch.float64) * 200.0
                cos, sin = ang.cos().float(), ang.sin().float()
                y = _rotary_eval(x, cos, sin, rot, inter, dt)
                ref, mag = rotary_ref64(x.double(), cos.double(), sin.double(), rot, inter)
                err = (y.double() - ref).abs()
                assert bool((err <= rotary_bar(ref, mag, dt)).all()), (D, rot, float(err.max()))
                assert torch.equal(y[rot:].view(torch.int16), x[rot:].view(torch.int16)), "columns at or beyond rotary_dim are bit-identical"
                assert not torch.equal(y[:rot], x[:rot])
    # the identity rotation returns every finite input bit for bit (the 16-bit <-> f32 conversions of the host side, over the whole format)
    allbits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dt)
    finite = torch.isfinite(allbits.float())
    one, zero = torch.ones(256), torch.zeros(256)
    for chunk in torch.where(finite, allbits, torch.zeros_like(allbits)).reshape(128, 512):      # (Inf * 0 is NaN: non-finite inputs are left out)
        y = _rotary_eval(chunk, one, zero, 512, inter, dt)
        assert torch.equal(y.float(), chunk.float())
    assert int(finite.sum()) > 60000


def test_rotary_eval_error_codes():
    lib = _fa2_lib.load()
    buf = (ctypes.c_float * 64)()
    x = torch.zeros(64, dtype=torch.float16)

    def a(**kw):
        v = dict(dt=F16, x=x.data_ptr(), c=buf, s=buf, D=64, rot=32, i=1, y=x.data_ptr())
        v.update(kw)
        return lib.fa2_rotary_eval(*[v[n] for n in ("dt", "x", "c", "s", "D", "rot", "i", "y")])

    assert a() == OK
    assert a(x=None) == NULLP and a(c=None) == NULLP and a(s=None) == NULLP and a(y=None) == NULLP
    assert a(D=0) == SHAPE
    for kw in (dict(D=60), dict(D=520), dict(rot=0), dict(rot=8), dict(rot=24), dict(rot=80), dict(rot=-16)):
        assert a(**kw) == HEAD_DIM, kw
    assert a(dt=2) == DTYPE and a(dt=2, rot=24) == HEAD_DIM and a(dt=2, D=0) == SHAPE and a(D=0, x=None) == NULLP


P = dc.HOST                                  # 16-byte aligned host memory that no call here ever touches
DEFAULTS = dict(dtype=F16, fmt=C16, kn=P, vn=P, k=P, v=P, lens=P, bt=None, B=2, Hkv=2, N=1, D=128, cap=256, page=0, pages=0, kns=_fa2_lib.strides3(256, 128, 256),
                vns=_fa2_lib.strides3(256, 128, 256), ks=_fa2_lib.strides3(256 * 256, 128, 256), vs=_fa2_lib.strides3(256 * 256, 128, 256), bts=0, q=None, qo=None,
                H=0, Nq=0, qs=None, qos=None, cos=None, sin=None, rdt=F32, rot=0, sro=0, ros=0, inter=1, kd=None, vd=None, ds=None)


def _call(**kw):
    """fa2_kvcache_append on host memory that is never touched: every call here is refused before the launch."""
    return dc.host_call("append", DEFAULTS, **kw)


def _ptr():
    buf = ctypes.create_string_buffer(64)
    _ptr.keep.append(buf)
    return (ctypes.addressof(buf) + 15) & ~15


_ptr.keep = []


def _rotary(p, **kw):
    return dict(dict(cos=p, sin=p, rdt=F32, rot=64, sro=16, ros=32), **kw)


def _with_q(p, **kw):
    s3 = _fa2_lib.strides3
    a = _rotary(p, q=p, qo=p, H=8, Nq=1, qs=s3(1024, 128, 1024), qos=s3(1024, 128, 1024))
    a.update(kw)
    return a


def test_every_error_code():
    p = _ptr()
    s3, s2 = _fa2_lib.strides3, _fa2_lib.strides2
    # a well-formed call gets past every check: it is stopped here by a defect of the LAST class only
    assert _call(B=1 << 30, N=4) == GRID and _call(**_with_q(p, B=1 << 30, N=4, Nq=4)) == GRID
    assert _call(fmt=C8, kd=p, vd=p, ds=s2(2, 1), B=1 << 30, N=4) == GRID
    for name in ("kn", "vn", "k", "v", "lens", "kns", "vns", "ks", "vs"):
        assert _call(**{name: None}) == NULLP, name
    assert _call(page=64, pages=4, bt=None) == NULLP
    for name in ("q", "qo", "qs", "qos"):
        assert _call(**_with_q(p, **{name: None})) == NULLP, name
    assert _call(**_rotary(p, cos=None)) == NULLP and _call(**_rotary(p, sin=None)) == NULLP
    assert _call(fmt=C8, kd=p, ds=None) == NULLP and _call(fmt=C8, vd=p, ds=None) == NULLP
    for kw in (dict(B=0), dict(Hkv=0), dict(N=0), dict(D=0), dict(cap=0), dict(page=48, pages=4, bt=p), dict(page=-64, pages=4, bt=p),
               dict(page=64, pages=0, bt=p), dict(page=1 << 20, cap=1 << 12, pages=4, bt=p), _with_q(p, H=0), _with_q(p, H=7), _with_q(p, Nq=2),
               _with_q(p, cos=None, sin=None), _rotary(p, sro=0), _rotary(p, ros=-32), dict(fmt=C8, kd=p, ds=s2(-2, 1)), dict(fmt=C8, vd=p, ds=s2(2, -1))):
        assert _call(**kw) == SHAPE, kw
    for kw in (dict(D=60), dict(D=520), dict(D=1024), dict(fmt=C8, D=72), _rotary(p, rot=0), _rotary(p, rot=8), _rotary(p, rot=24), _rotary(p, rot=144),
               _rotary(p, rot=-16)):
        assert _call(**kw) == HEAD_DIM, kw
    assert _call(D=72, kns=s3(144, 72, 144), vns=s3(144, 72, 144), B=1 << 30, N=4) == GRID           # a multiple of 8 serves a 16-bit cache
    for kw in (dict(kn=p + 8), dict(vn=p + 8), dict(k=p + 8), dict(v=p + 4), dict(lens=p + 2), dict(page=64, pages=4, bt=p + 2), dict(kns=s3(256, 132, 256)),
               dict(vns=s3(256, 128, 0)), dict(ks=s3(65536, 128, 260)), dict(vs=s3(-65536, 128, 256)), dict(page=64, pages=4, bt=p, bts=-4),
               dict(fmt=C8, ks=s3(65536 + 8, 128, 256)), dict(fmt=C8, vs=s3(65536, 136, 256)), dict(fmt=C8, kd=p + 2, ds=s2(2, 1)),
               dict(fmt=C8, vd=p + 1, ds=s2(2, 1)), _with_q(p, q=p + 8), _with_q(p, qo=p + 8), _with_q(p, qs=s3(1024, 132, 1024)),
               _with_q(p, qos=s3(1024, 128, -1024)), _rotary(p, cos=p + 8), _rotary(p, sin=p + 4), _rotary(p, ros=34), _rotary(p, rdt=F16, ros=36)):
        assert _call(**kw) == ALIGN, kw
    assert _call(**_rotary(p, ros=36, B=1 << 30, N=4)) == GRID                                          # f32 rows: multiples of 4 elements
    for kw in (dict(dtype=2), dict(dtype=-1), dict(fmt=2), dict(fmt=-1), _rotary(p, rdt=BF16), _rotary(p, rdt=3), dict(kd=p, ds=s2(2, 1)),
               dict(vd=p, ds=s2(2, 1))):
        assert _call(**kw) == DTYPE, kw
    assert _call(dtype=BF16, **_rotary(p, rdt=BF16, B=1 << 30, N=4)) == GRID
    assert _call(B=1 << 16, N=1 << 15) == GRID and _call(B=1 << 15, N=1 << 15, Hkv=1 << 20) == GRID


def test_error_precedence():
    """null pointer, sizes, head dim / rotary_dim, alignment, dtype, grid: a call with two defects reports the earlier."""
    p = _ptr()
    defects = [(NULLP, dict(vns=None)), (SHAPE, dict(N=0)), (HEAD_DIM, dict(D=60)), (ALIGN, dict(ks=_fa2_lib.strides3(65536, 128, 260))),
               (DTYPE, dict(dtype=7)), (GRID, dict(B=1 << 30, N=4))]
    for i, (code, kw) in enumerate(defects):
        assert _call(**kw) == code
        for (_, later) in defects[i + 1:]:
            assert _call(**dict(later, **kw)) == code, (kw, later)
    rot = [(NULLP, dict(sin=None)), (SHAPE, dict(sro=0)), (HEAD_DIM, dict(rot=24)), (ALIGN, dict(ros=34)), (DTYPE, dict(rdt=BF16))]
    for i, (code, kw) in enumerate(rot):
        assert _call(**_rotary(p, **kw)) == code
        for (_, later) in rot[i + 1:]:
            assert _call(**_rotary(p, **dict(later, **kw))) == code, (kw, later)


def _args(B=2, Nq=1, H=8, Hkv=2, D=128, Nmax=128, dt=torch.float16, cache=torch.float16):
    q = torch.zeros(B, Nq, H, D, dtype=dt)
    kc, vc = (torch.zeros(B, Nmax, Hkv, D, dtype=torch.float16).to(cache) for _ in range(2))
    k, v = (torch.zeros(B, Nq, Hkv, D, dtype=dt) for _ in range(2))
    return q, kc, vc, k, v, torch.ones(B, dtype=torch.int32)


def test_operator_argument_checks():
    """Raised before any device work: CPU tensors reach the checks."""
    q, kc, vc, k, v, lens = _args()
    cos, sin = torch.ones(16, 32), torch.zeros(16, 32)
    # rotary without k / v; one of k / v alone; Nnew != Nq in the fused call
    with pytest.raises(ValueError, match="rotary without an append"):
        flash_attention_decode(q, kc, vc, lens, rotary_cos=cos, rotary_sin=sin)
    with pytest.raises(ValueError, match="k and v together"):
        flash_attention_decode(q, kc, vc, lens, k=k)
    with pytest.raises(ValueError, match=r"k.shape\[1\] == Nq"):
        flash_attention_decode(q, kc, vc, lens, k=k.expand(2, 3, 2, 128), v=v.expand(2, 3, 2, 128))
    with pytest.raises(ValueError, match="k and v together"):
        flash_attention_decode(q, kc, vc, lens, k=k.to(torch.bfloat16), v=v.to(torch.bfloat16))
    # a descale with a 16-bit cache, in either call
    with pytest.raises(ValueError, match="descale.*float8_e4m3fn caches"):
        kvcache_append(kc, vc, k, v, lens, k_descale=torch.ones(2, 2))
    with pytest.raises(ValueError, match="descale.*float8_e4m3fn caches"):
        flash_attention_decode(q, kc, vc, lens, v_descale=torch.ones(2, 2), k=k, v=v)
    # rotary_dim: not a multiple of 16, above D, tables of different shapes, one table alone
    for bad in (torch.ones(16, 12), torch.ones(16, 72), torch.ones(16, 4)):
        with pytest.raises(ValueError, match="multiple of 16"):
            kvcache_append(kc, vc, k, v, lens, rotary_cos=bad, rotary_sin=bad)
        with pytest.raises(ValueError, match="multiple of 16"):
            flash_attention_decode(q, kc, vc, lens, k=k, v=v, rotary_cos=bad, rotary_sin=bad)
    with pytest.raises(ValueError, match="of one shape"):
        kvcache_append(kc, vc, k, v, lens, rotary_cos=cos, rotary_sin=sin[:, :16])
    with pytest.raises(ValueError, match="come together"):
        kvcache_append(kc, vc, k, v, lens, rotary_cos=cos)
    # mismatched table dtypes; a 16-bit table that is not k's dtype
    with pytest.raises(ValueError, match="share one dtype"):
        kvcache_append(kc, vc, k, v, lens, rotary_cos=cos, rotary_sin=sin.half())
    with pytest.raises(ValueError, match="share one dtype"):
        kvcache_append(kc, vc, k, v, lens, rotary_cos=cos.bfloat16(), rotary_sin=sin.bfloat16())
    with pytest.raises(ValueError, match="share one dtype"):
        flash_attention_decode(q, kc, vc, lens, k=k, v=v, rotary_cos=cos.double(), rotary_sin=sin.double())
    # q without rotary, q of another shape; k / v of different shapes; a head dim the append does not serve; an e4m3 cache with D % 16 != 0
    with pytest.raises(ValueError, match="nothing to do"):
        kvcache_append(kc, vc, k, v, lens, q=q)
    with pytest.raises(ValueError, match="Hkv dividing H"):
        kvcache_append(kc, vc, k, v, lens, rotary_cos=cos, rotary_sin=sin, q=q[:, :, :3])
    with pytest.raises(ValueError, match="one shape and dtype"):
        kvcache_append(kc, vc, k, v[:, :, :1], lens)
    with pytest.raises(ValueError, match="inconsistent"):
        kvcache_append(kc, vc[..., :64], k, v, lens)
    q9, kc9, vc9, k9, v9, _ = _args(D=100)
    with pytest.raises(ValueError, match="multiples of 8"):
        kvcache_append(kc9, vc9, k9, v9, lens)
    q8, kc8, vc8, k8, v8, _ = _args(D=72, cache=E4M3)
    with pytest.raises(ValueError, match="multiples of 8"):
        kvcache_append(kc8, vc8, k8, v8, lens)
    with pytest.raises(ValueError, match="e5m2 and the fnuz formats"):
        kvcache_append(kc.to(torch.float8_e5m2), vc.to(torch.float8_e5m2), k, v, lens)
    with pytest.raises(ValueError, match="cache_seqlens must be"):
        kvcache_append(kc, vc, k, v, lens.long())
    # everything in order: only the device is missing
    with pytest.raises(RuntimeError, match="ROCm device"):
        kvcache_append(kc, vc, k, v, lens, rotary_cos=cos, rotary_sin=sin, q=q)
    with pytest.raises(RuntimeError, match="ROCm device"):
        flash_attention_decode(q, kc, vc, lens, k=k, v=v, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=False)


def _brief(calls):
    """the decode entry with its q, the append with its argument count, q, q_out and rotary_dim; the size queries left out"""
    out = []
    for name, a in calls:
        if name == "fa2_fwd_decode":
            out.append(("decode", dc.arg("plain", a, "q")))
        elif name == "fa2_kvcache_append":
            out.append(("append", len(a)) + tuple(dc.arg("append", a, n) for n in ("q", "qo", "rot")))
        else:
            assert name == "fa2_fwd_decode_workspace_bytes", name
    return out


def test_the_fused_call_appends_then_decodes_on_the_rotated_q(monkeypatch):
    rec = dc.recording_lib(monkeypatch)
    q, kc, vc, k, v, lens = _args()
    cos, sin = torch.ones(16, 32), torch.zeros(16, 32)
    flash_attention_decode(q, kc, vc, lens)                                                  # no new keyword: the one launch it made before
    assert _brief(rec.calls) == [("decode", q.data_ptr())]
    del rec.calls[:]
    flash_attention_decode(q, kc, vc, lens, k=k, v=v)                                        # no rotary: q is not touched and not passed
    assert _brief(rec.calls) == [("append", 37, None, None, 0), ("decode", q.data_ptr())]
    del rec.calls[:]
    flash_attention_decode(q, kc, vc, lens, k=k, v=v, rotary_cos=cos, rotary_sin=sin)
    (tag, n, qin, qout, rot), (tag2, qdec) = _brief(rec.calls)
    assert (tag, n, qin, rot, tag2) == ("append", 37, q.data_ptr(), 64, "decode") and qout not in (None, q.data_ptr()) and qdec == qout
    assert kvcache_append(kc, vc, k, v, lens) is None
