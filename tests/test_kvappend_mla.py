"""CPU tests of the append for a latent (MLA) KV cache (include/fa2_gfx950.h: fa2_kvcache_append_mla, fa2_kvcache_append_mla_varlen,
fa2_kvappend_mla_chunks; kvcache_append_mla, kvcache_append_mla_varlen and the kv_c / k_pe / rotary_* keywords of flash_attention_decode_mla): the
symbols, every validation code of the two entries and the order they are checked in on host memory that is never touched, the argument checks of
the three operators and the calls they make through a stand-in library, the unit -> chunks map the kernel and the host share, the expected-image
builder of the GPU tests against fa2_rotary_eval, the sanitizer run of the kernel's addressing as a stand-alone program, and the private segment of
the new unit's kernels.  Nothing here touches a device: every rejected call returns before the launch."""
import concurrent.futures
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import decode_calls as dc
import mla_append_refs as ar
from conftest import PKG, ROOT
from rocwmma_fattn import FlashAttn, _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention_decode_mla, kvcache_append_mla, kvcache_append_mla_varlen

HEADER = os.path.join(ROOT, "include", "fa2_gfx950.h")
SYMBOLS = ("fa2_kvcache_append_mla", "fa2_kvcache_append_mla_varlen", "fa2_kvappend_mla_chunks")
OK, NULLP, SHAPE, HEAD_DIM, ALIGN, DTYPE, SCALE, GRID = 0, -1, -2, -3, -4, -5, -6, -7
F16, BF16, F32 = _fa2_lib.FA2_DTYPE_F16, _fa2_lib.FA2_DTYPE_BF16, _fa2_lib.FA2_DTYPE_F32
S2, S3 = _fa2_lib.strides2, _fa2_lib.strides3


def S1(a):
    return (ctypes.c_int64 * 1)(a)


def test_symbols_are_declared_exported_and_bound_and_the_operators_are_public():
    lib = _fa2_lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _fa2_lib.SYMBOLS, name
        assert getattr(lib, name).argtypes == _fa2_lib.SYMBOLS[name][1]
    for entry, symbol in (("append_mla", "fa2_kvcache_append_mla"), ("append_mla_varlen", "fa2_kvcache_append_mla_varlen")):
        proto = re.search(r"\b%s\s*\((.*?)\);" % symbol, text, flags=re.S).group(1)
        assert dc.ENTRIES[entry][0] == symbol
        assert len(proto.split(",")) == len(_fa2_lib.SYMBOLS[symbol][1]) == len(dc.ENTRIES[entry][1]) == 31
    assert _fa2_lib.SYMBOLS["fa2_kvcache_append_mla_varlen"][1][8] is ctypes.c_int64, "total is a 64-bit count"
    assert len(_fa2_lib.SYMBOLS["fa2_fwd_decode_mla"][1]) == 25, "the decode entry keeps its 25 arguments"
    import rocwmma_fattn
    for name, f in (("kvcache_append_mla", kvcache_append_mla), ("kvcache_append_mla_varlen", kvcache_append_mla_varlen)):
        assert name in FlashAttn.__all__ and getattr(rocwmma_fattn, name) is f


# ---------------------------------------------------------------------------------------------------------------- the unit -> chunks map
def test_chunks_map():
    """Both values of halves: the 36 units of a row cover chunks 0 .. 71 exactly once.  halves: every pair (64 + c, 68 + c) shares a unit, and the
    units in front of the tail are (2u, 2u + 1); without: every unit is (2u, 2u + 1).  No unit mixes kv_c's chunks (0 .. 63) with k_pe's."""
    for halves in (0, 1):
        pairs = [_fa2_lib.kvappend_mla_chunks(u, halves) for u in range(36)]
        assert sorted(c for p in pairs for c in p) == list(range(72))
        assert all((a < 64) == (b < 64) for a, b in pairs)
        if halves:
            assert pairs[:32] == [(2 * u, 2 * u + 1) for u in range(32)] and pairs[32:] == [(64 + c, 68 + c) for c in range(4)]
        else:
            assert pairs == [(2 * u, 2 * u + 1) for u in range(36)]
    lib = _fa2_lib.load()
    a, b = ctypes.c_int(), ctypes.c_int()
    assert lib.fa2_kvappend_mla_chunks(0, 0, None, ctypes.byref(b)) == NULLP and lib.fa2_kvappend_mla_chunks(0, 0, ctypes.byref(a), None) == NULLP
    assert lib.fa2_kvappend_mla_chunks(-1, 0, ctypes.byref(a), ctypes.byref(b)) == SHAPE and lib.fa2_kvappend_mla_chunks(36, 1, ctypes.byref(a), ctypes.byref(b)) == SHAPE


# ---------------------------------------------------------------------------------------------------------------- the C-ABI's checks
P = dc.HOST                                  # 16-byte aligned host memory that no call here ever touches
KS = S3(256 * 576, 576, 576)
UNIFORM = dict(dtype=F16, kn=P, vn=P, k=P, lens=P, bt=None, B=2, N=3, D=576, Dv=512, cap=256, page=0, pages=0, kns=S2(3 * 512, 512), vns=S2(3 * 64, 64), ks=KS,
               bts=0, q=None, qo=None, H=0, Nq=0, qs=None, qos=None, cos=None, sin=None, rdt=F32, rot=0, sro=0, ros=0, inter=1)
PACKED = dict(dtype=F16, kn=P, vn=P, k=P, cu=P, lens=P, bt=None, B=2, total=5, D=576, Dv=512, cap=256, page=0, pages=0, kns=S1(512), vns=S1(64), ks=KS, bts=0, q=None,
              qo=None, H=0, qs=None, qos=None, cos=None, sin=None, rdt=F32, rot=0, sro=0, ros=0, inter=1)
BIG = {False: dict(B=65536, N=32768), True: dict(total=2 ** 31)}       # the defect of the LAST class: a call that carries it got past every other check


def _call(packed, **kw):
    """The entry on host memory that is never touched: every call here returns before a launch."""
    return dc.host_call("append_mla_varlen" if packed else "append_mla", PACKED if packed else UNIFORM, **kw)


def _rotary(**kw):
    return dict(dict(cos=P, sin=P, rdt=F32, rot=64, sro=16, ros=32), **kw)


def _with_q(packed, **kw):
    a = _rotary(q=P, qo=P, H=16)
    a.update(dict(qs=S2(576, 16 * 576), qos=S2(576, 16 * 576)) if packed else dict(Nq=3, qs=S3(3 * 16 * 576, 576, 16 * 576), qos=S3(3 * 16 * 576, 576, 16 * 576)))
    a.update(kw)
    if not packed and "Nq" not in kw:
        a["Nq"] = kw.get("N", 3)                                 # Nq == Nnew, whatever Nnew a case sets
    return a


@pytest.mark.parametrize("packed", [False, True], ids=["uniform", "packed"])
def test_every_error_code(packed):
    call, big, p = (lambda **kw: _call(packed, **kw)), BIG[packed], P
    with_q = lambda **kw: _with_q(packed, **kw)                  # noqa: E731
    assert call(**big) == GRID and call(**with_q(**big)) == GRID
    for name in ("kn", "vn", "k", "lens", "kns", "vns", "ks") + (("cu",) if packed else ()):
        assert call(**{name: None}) == NULLP, name
    assert call(page=64, pages=4, bt=None) == NULLP
    for name in ("q", "qo", "qs", "qos"):
        assert call(**with_q(**{name: None})) == NULLP, name
    assert call(**_rotary(cos=None)) == NULLP and call(**_rotary(sin=None)) == NULLP
    sizes = [dict(B=0), dict(D=0), dict(Dv=0), dict(cap=0), dict(page=48, pages=4, bt=p), dict(page=-64, pages=4, bt=p), dict(page=64, pages=0, bt=p),
             dict(page=1 << 20, cap=1 << 12, pages=4, bt=p), with_q(H=0), with_q(H=129), with_q(cos=None, sin=None), _rotary(sro=0), _rotary(ros=-32)]
    sizes += [dict(total=-1)] if packed else [dict(N=0), with_q(Nq=2), with_q(Nq=0)]
    for kw in sizes:
        assert call(**kw) == SHAPE, kw
    for kw in (dict(D=512), dict(D=584), dict(D=640), dict(Dv=576), dict(Dv=256), dict(D=128, Dv=128), _rotary(rot=32), _rotary(rot=128), _rotary(rot=0),
               _rotary(rot=48), with_q(rot=32)):
        assert call(**kw) == HEAD_DIM, kw
    one = S1 if packed else (lambda a: S2(3 * a, a))
    for kw in (dict(kn=p + 8), dict(vn=p + 8), dict(k=p + 4), dict(lens=p + 2), dict(page=64, pages=4, bt=p + 2), dict(kns=one(516)), dict(vns=one(0)),
               dict(kns=one(-512)), dict(ks=S3(256 * 576, 576, 580)), dict(ks=S3(-576, 576, 576)), dict(page=64, pages=4, bt=p, bts=-4), with_q(q=p + 8),
               with_q(qo=p + 8), with_q(qs=S2(580, 16 * 576) if packed else S3(0, 580, 16 * 576)), with_q(qos=S2(576, -576) if packed else S3(0, 576, -576)),
               _rotary(cos=p + 8), _rotary(sin=p + 4), _rotary(ros=34), _rotary(rdt=F16, ros=36)) + ((dict(cu=p + 2), dict(cu=p + 1)) if packed else ()):
        assert call(**kw) == ALIGN, kw
    assert call(**_rotary(ros=36, **big)) == GRID                                                   # f32 rows: multiples of 4 elements
    for kw in (dict(dtype=2), dict(dtype=-1), _rotary(rdt=BF16), _rotary(rdt=3)):
        assert call(**kw) == DTYPE, kw
    assert call(dtype=BF16, **_rotary(rdt=BF16, **big)) == GRID and call(**with_q(H=128, **big)) == GRID and call(**with_q(H=1, **big)) == GRID


def test_an_empty_token_buffer_is_success_without_a_launch():
    """total = 0 passes the checks and returns FA2_OK: the pointers are host memory, so a launch would not have."""
    assert _call(True, total=0) == OK and _call(True, **_with_q(True, total=0)) == OK
    assert _call(True, total=0, cu=None) == NULLP and _call(True, total=0, D=512) == HEAD_DIM and _call(True, total=0, dtype=9) == DTYPE      # the checks still run


@pytest.mark.parametrize("packed", [False, True], ids=["uniform", "packed"])
def test_error_precedence(packed):
    """null pointer, sizes, head dim / rotary_dim, alignment, dtype, grid — fa2_kvcache_append's order: a call with two defects reports the earlier."""
    defects = [(NULLP, dict(lens=None)), (SHAPE, dict(B=0)), (HEAD_DIM, dict(Dv=500)), (ALIGN, dict(lens=P + 2)), (DTYPE, dict(dtype=7)), (GRID, BIG[packed])]
    for i, (code, kw) in enumerate(defects):
        assert _call(packed, **kw) == code
        for (_, later) in defects[i + 1:]:
            assert _call(packed, **dict(later, **kw)) == code, (kw, later)
    rot = [(NULLP, dict(sin=None)), (SHAPE, dict(sro=0)), (HEAD_DIM, dict(rot=32)), (ALIGN, dict(ros=34)), (DTYPE, dict(rdt=BF16))]
    for i, (code, kw) in enumerate(rot):
        assert _call(packed, **_rotary(**kw)) == code
        for (_, later) in rot[i + 1:]:
            assert _call(packed, **_rotary(**dict(later, **kw))) == code, (kw, later)
    assert _call(packed, **_with_q(packed, H=129, D=512)) == SHAPE and _call(packed, **_with_q(packed, cos=None, sin=None, D=512)) == SHAPE


# ---------------------------------------------------------------------------------------------------------------- the operators
def _args(B=2, nnew=3, H=16, dt=torch.float16, page=64):
    kv = torch.zeros(6, page, 576, dtype=dt)
    kv_c, k_pe, q = torch.zeros(B, nnew, 512, dtype=dt), torch.zeros(B, nnew, 64, dtype=dt), torch.zeros(B, nnew, H, 576, dtype=dt)
    return kv, kv_c, k_pe, q, torch.tensor([70, 100], dtype=torch.int32), torch.zeros(B, 3, dtype=torch.int32)


COS, SIN = torch.ones(16, 32), torch.zeros(16, 32)


def test_uniform_operator_argument_checks():
    kv, kv_c, k_pe, q, lens, bt = _args()
    f = kvcache_append_mla
    rot = dict(rotary_cos=COS, rotary_sin=SIN)
    bad = [
        ((kv, kv_c[0], k_pe[0], lens, bt), {}),                                        # ranks
        ((kv[0], kv_c, k_pe, lens, bt), {}),
        ((kv.unsqueeze(2).expand(6, 64, 2, 576), kv_c, k_pe, lens, bt), {}),           # a head axis that is not 1
        ((kv, kv_c[..., :256], k_pe, lens, bt), {}), ((kv, kv_c, k_pe[..., :32], lens, bt), {}), ((kv[..., :512], kv_c, k_pe, lens, bt), {}),      # widths
        ((kv, kv_c, k_pe[:, :2], lens, bt), {}), ((kv, kv_c[:1], k_pe, lens, bt), {}),  # one row of each per token
        ((kv, kv_c.bfloat16(), k_pe, lens, bt), {}), ((kv, kv_c, k_pe.bfloat16(), lens, bt), {}), ((kv.bfloat16(), kv_c, k_pe, lens, bt), {}),     # dtypes
        ((kv.float(), kv_c.float(), k_pe.float(), lens, bt), {}),
        ((kv, kv_c[:, :0], k_pe[:, :0], lens, bt), {}),                                # Nnew = 0
        ((kv, kv_c, k_pe, lens, bt), dict(rotary_cos=COS)), ((kv, kv_c, k_pe, lens, bt), dict(rotary_sin=SIN)),      # the tables come together
        ((kv, kv_c, k_pe, lens, bt), dict(rotary_cos=COS[:, :16], rotary_sin=SIN[:, :16])),                           # rotary_dim 32
        ((kv, kv_c, k_pe, lens, bt), dict(rotary_cos=torch.ones(16, 64), rotary_sin=torch.zeros(16, 64))),            # rotary_dim 128
        ((kv, kv_c, k_pe, lens, bt), dict(rotary_cos=COS, rotary_sin=SIN.half())), ((kv, kv_c, k_pe, lens, bt), dict(rotary_cos=COS.bfloat16(), rotary_sin=SIN.bfloat16())),
        ((kv, kv_c, k_pe, lens, bt), dict(q=q)),                                       # q without tables
        ((kv, kv_c, k_pe, lens, bt), dict(q=q[:, :2], **rot)), ((kv, kv_c, k_pe, lens, bt), dict(q=q[..., :512], **rot)), ((kv, kv_c, k_pe, lens, bt), dict(q=q[0], **rot)),
        ((kv, kv_c, k_pe, lens, bt), dict(q=q.bfloat16(), **rot)), ((kv, kv_c, k_pe, lens, bt), dict(q=torch.zeros(2, 3, 129, 576, dtype=torch.float16), **rot)),
        ((kv, kv_c, k_pe, lens.long(), bt), {}), ((kv, kv_c, k_pe, lens[:1], bt), {}), ((kv, kv_c, k_pe, lens, bt[:1]), {}), ((kv, kv_c, k_pe, lens, bt.long()), {}),
        ((torch.zeros(6, 48, 576, dtype=torch.float16), kv_c, k_pe, lens, bt), {}),    # page size 48
        ((kv[:1], kv_c, k_pe, lens, None), {}),                                        # a contiguous cache of another batch
    ]
    for a, kw in bad:
        with pytest.raises(ValueError):
            f(*a, **kw)
    with pytest.raises(ValueError, match="nothing to do"):
        f(kv, kv_c, k_pe, lens, bt, q=q)
    with pytest.raises(ValueError, match=r"\[seqlen_ro, 32\]"):
        f(kv, kv_c, k_pe, lens, bt, rotary_cos=COS[:, :16], rotary_sin=SIN[:, :16])
    with pytest.raises(RuntimeError, match="ROCm device"):                             # everything in order: only the device is missing
        f(kv, kv_c, k_pe, lens, bt, q=q, rotary_interleaved=False, **rot)
    with pytest.raises(RuntimeError, match="ROCm device"):                             # a head axis of size 1 on all three
        f(kv.unsqueeze(2), kv_c.unsqueeze(2), k_pe.unsqueeze(2), lens, bt)


def test_packed_operator_argument_checks():
    kv, kv_c, k_pe, q, lens, bt = _args()
    kv_c, k_pe, q = kv_c.reshape(6, 512), k_pe.reshape(6, 64), q.reshape(6, 16, 576)
    cu = torch.tensor([0, 2, 5], dtype=torch.int32)
    f = kvcache_append_mla_varlen
    rot = dict(rotary_cos=COS, rotary_sin=SIN)
    for a, kw in [((kv, kv_c[None], k_pe[None], cu, lens, bt), {}), ((kv, kv_c, k_pe[:5], cu, lens, bt), {}), ((kv, kv_c, k_pe.bfloat16(), cu, lens, bt), {}),
                  ((kv, kv_c, k_pe, cu.long(), lens, bt), {}), ((kv, kv_c, k_pe, cu[:1], lens, bt), {}), ((kv, kv_c, k_pe, [0, 2, 5], lens, bt), {}),
                  ((kv, kv_c, k_pe, cu, lens[:1], bt), {}), ((kv, kv_c, k_pe, cu, lens, bt), dict(q=q)), ((kv, kv_c, k_pe, cu, lens, bt), dict(q=q[:5], **rot)),
                  ((kv, kv_c, k_pe, cu, lens, bt), dict(q=q[None], **rot)), ((kv, kv_c, k_pe, cu, lens, bt), dict(rotary_cos=COS[:, :16], rotary_sin=SIN[:, :16])),
                  ((kv, kv_c, k_pe, cu, lens, bt), dict(rotary_cos=torch.ones(16, 64), rotary_sin=torch.zeros(16, 64)))]:
        with pytest.raises(ValueError):
            f(*a, **kw)
    with pytest.raises(RuntimeError, match="ROCm device"):
        f(kv, kv_c, k_pe, cu, lens, bt, q=q, **rot)
    with pytest.raises(RuntimeError, match="ROCm device"):                             # an empty token buffer still meets every check
        f(kv, kv_c[:0], k_pe[:0], cu, lens, bt)


def test_fused_decode_argument_checks():
    kv, kv_c, k_pe, q, lens, bt = _args(nnew=1)
    f = flash_attention_decode_mla
    rot = dict(rotary_cos=COS, rotary_sin=SIN)
    with pytest.raises(ValueError, match="rotary without an append"):
        f(q, kv, lens, bt, **rot)
    with pytest.raises(ValueError, match="rotary without an append"):
        f(q, kv, lens, bt, rotary_sin=SIN)
    for kw in (dict(kv_c=kv_c), dict(k_pe=k_pe), dict(kv_c=kv_c[:1], k_pe=k_pe[:1]), dict(kv_c=kv_c.expand(2, 2, 512), k_pe=k_pe.expand(2, 2, 64))):
        with pytest.raises(ValueError, match="kv_c and k_pe together"):
            f(q, kv, lens, bt, **kw)
    for kw in (dict(kv_c=kv_c.bfloat16(), k_pe=k_pe.bfloat16()), dict(kv_c=kv_c, k_pe=k_pe, rotary_cos=COS), dict(kv_c=kv_c[..., :256], k_pe=k_pe),
               dict(kv_c=kv_c, k_pe=k_pe, rotary_cos=COS[:, :16], rotary_sin=SIN[:, :16]), dict(kv_c=kv_c, k_pe=k_pe, num_splits=129, **rot),
               dict(kv_c=kv_c, k_pe=k_pe, num_splits=-1, **rot)):
        with pytest.raises(ValueError):
            f(q, kv, lens, bt, **kw)
    with pytest.raises(RuntimeError, match="ROCm device"):
        f(q, kv, lens, bt, kv_c=kv_c, k_pe=k_pe, rotary_interleaved=False, **rot)
    with pytest.raises(RuntimeError, match="ROCm device"):
        f(q, kv, lens, bt, kv_c=kv_c, k_pe=k_pe)


def _plain(a):
    return tuple(tuple(x) if isinstance(x, ctypes.Array) else x for x in a)


def test_the_operators_hand_the_entries_what_the_tensors_say(monkeypatch):
    """CPU tensors under the recording library.  The two slices of one [B, Nnew, 584] projection output and a cache view with a row stride of 584 reach
    the entry as they are; a source the kernel cannot address is copied; the packed call sends one row stride each and {head, row} for q."""
    rec = dc.recording_lib(monkeypatch)
    dt = torch.bfloat16
    proj = torch.zeros(2, 3, 584, dtype=dt)
    kv_c, k_pe = proj[..., :512], proj[..., 512:576]
    pool = torch.zeros(6, 64, 584, dtype=dt)[..., :576]
    q = torch.zeros(2, 3, 16, 576, dtype=dt)
    lens, bt = torch.tensor([70, 100], dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32)[:, :3]
    cos, sin = COS.clone(), SIN.clone()
    q_out = kvcache_append_mla(pool, kv_c, k_pe, lens, bt, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=False, q=q)
    (name, args), = rec.calls
    got = dict(zip(dc.ENTRIES["append_mla"][1], _plain(args)))
    assert name == "fa2_kvcache_append_mla" and len(args) == 31
    assert got == dict(dtype=BF16, kn=kv_c.data_ptr(), vn=k_pe.data_ptr(), k=pool.data_ptr(), lens=lens.data_ptr(), bt=bt.data_ptr(), B=2, N=3, D=576, Dv=512, cap=3, page=64,
                       pages=6, kns=(3 * 584, 584), vns=(3 * 584, 584), ks=(64 * 584, 576, 584), bts=4, q=q.data_ptr(), qo=q_out.data_ptr(), H=16, Nq=3,
                       qs=(3 * 16 * 576, 576, 16 * 576), qos=(3 * 16 * 576, 576, 16 * 576), cos=cos.data_ptr(), sin=sin.data_ptr(), rdt=F32, rot=64, sro=16, ros=32,
                       inter=0, stream=None)
    assert k_pe.data_ptr() == proj.data_ptr() + 1024 and q_out.data_ptr() != q.data_ptr() and tuple(q_out.shape) == tuple(q.shape)
    del rec.calls[:]
    odd = torch.zeros(2, 3, 516, dtype=dt)[..., :512]                                  # row stride 516: no multiple of 8 -> copied
    assert kvcache_append_mla(pool, odd, k_pe, lens, bt) is None
    got = dict(zip(dc.ENTRIES["append_mla"][1], _plain(rec.calls[0][1])))
    assert got["kn"] not in (odd.data_ptr(), None) and got["kns"] == (3 * 512, 512) and got["vn"] == k_pe.data_ptr()
    assert (got["q"], got["qo"], got["H"], got["Nq"], got["qs"], got["qos"], got["cos"], got["sin"], got["rot"], got["sro"], got["ros"]) == (None, None, 0, 0, None, None, None, None, 0, 0, 0)
    del rec.calls[:]
    with pytest.raises(ValueError, match="16-byte aligned storage"):                   # a cache the kernel cannot address raises: it is never copied
        kvcache_append_mla(torch.zeros(2, 128, 580, dtype=dt)[..., :576], kv_c, k_pe, lens)
    assert rec.calls == []
    # packed
    flat = torch.zeros(8, 584, dtype=dt)
    cu = torch.tensor([0, 2, 5], dtype=torch.int32)
    qp = torch.zeros(8, 16, 576, dtype=dt)
    c16, s16 = cos.to(dt), sin.to(dt)
    q_out = kvcache_append_mla_varlen(pool, flat[:, :512], flat[:, 512:576], cu, lens, bt, rotary_cos=c16, rotary_sin=s16, q=qp)
    (name, args), = rec.calls
    got = dict(zip(dc.ENTRIES["append_mla_varlen"][1], _plain(args)))
    assert name == "fa2_kvcache_append_mla_varlen" and len(args) == 31
    assert got == dict(dtype=BF16, kn=flat.data_ptr(), vn=flat.data_ptr() + 1024, k=pool.data_ptr(), cu=cu.data_ptr(), lens=lens.data_ptr(), bt=bt.data_ptr(), B=2, total=8,
                       D=576, Dv=512, cap=3, page=64, pages=6, kns=(584,), vns=(584,), ks=(64 * 584, 576, 584), bts=4, q=qp.data_ptr(), qo=q_out.data_ptr(), H=16,
                       qs=(576, 16 * 576), qos=(576, 16 * 576), cos=c16.data_ptr(), sin=s16.data_ptr(), rdt=BF16, rot=64, sro=16, ros=32, inter=1, stream=None)
    del rec.calls[:]
    assert kvcache_append_mla_varlen(pool, flat[:0, :512], flat[:0, 512:576], cu, lens, bt) is None and rec.calls == [], "an empty token buffer: no call"


def test_the_fused_decode_appends_then_attends_on_the_rotated_q(monkeypatch):
    rec = dc.recording_lib(monkeypatch)
    dt = torch.float16
    kv = torch.zeros(2, 128, 576, dtype=dt)
    q = torch.zeros(2, 2, 16, 576, dtype=dt)
    proj = torch.zeros(2, 2, 584, dtype=dt)
    kv_c, k_pe = proj[..., :512], proj[..., 512:576]
    lens = torch.tensor([70, 100], dtype=torch.int32)
    # without the keywords: exactly the calls of before — the size query and the 25-argument entry on q itself
    o = flash_attention_decode_mla(q, kv, lens, num_splits=1)
    assert [n for n, _ in rec.calls] == ["fa2_fwd_decode_mla_workspace_bytes", "fa2_fwd_decode_mla"]
    base = dict(zip(dc.ENTRIES["mla"][1], _plain(rec.calls[1][1])))
    assert len(rec.calls[1][1]) == 25 and base["q"] == q.data_ptr() and base["o"] == o.data_ptr() and base["k"] == kv.data_ptr()
    del rec.calls[:]
    # with the new tokens and tables: the append, then the same two calls on the rotated q
    o = flash_attention_decode_mla(q, kv, lens, num_splits=1, kv_c=kv_c, k_pe=k_pe, rotary_cos=COS, rotary_sin=SIN, rotary_interleaved=False)
    assert [n for n, _ in rec.calls] == ["fa2_kvcache_append_mla", "fa2_fwd_decode_mla_workspace_bytes", "fa2_fwd_decode_mla"]
    app = dict(zip(dc.ENTRIES["append_mla"][1], _plain(rec.calls[0][1])))
    dec = dict(zip(dc.ENTRIES["mla"][1], _plain(rec.calls[2][1])))
    assert app["q"] == q.data_ptr() and app["qo"] not in (None, q.data_ptr()) and dec["q"] == app["qo"], "the attention reads the rotated q"
    assert (app["kn"], app["vn"], app["k"], app["lens"], app["B"], app["N"], app["Nq"], app["H"], app["rot"], app["inter"]) == \
        (kv_c.data_ptr(), k_pe.data_ptr(), kv.data_ptr(), lens.data_ptr(), 2, 2, 2, 16, 64, 0)
    assert {k: v for k, v in dec.items() if k not in ("q", "o", "lse")} == {k: v for k, v in base.items() if k not in ("q", "o", "lse")}
    del rec.calls[:]
    # without tables: k_pe is copied, q is not touched and not passed
    flash_attention_decode_mla(q, kv, lens, num_splits=1, kv_c=kv_c, k_pe=k_pe)
    app = dict(zip(dc.ENTRIES["append_mla"][1], _plain(rec.calls[0][1])))
    dec = dict(zip(dc.ENTRIES["mla"][1], _plain(rec.calls[2][1])))
    assert (app["q"], app["qo"], app["H"], app["rot"]) == (None, None, 0, 0) and dec["q"] == q.data_ptr()
    del rec.calls[:]
    # a call either half refuses makes no C call at all
    for kw in (dict(num_splits=129), dict(rotary_cos=COS[:, :16], rotary_sin=SIN[:, :16]), dict(rotary_sin=None)):
        with pytest.raises(ValueError):
            flash_attention_decode_mla(q, kv, lens, **dict(dict(kv_c=kv_c, k_pe=k_pe, rotary_cos=COS, rotary_sin=SIN), **kw))
        assert rec.calls == []


# ---------------------------------------------------------------------------------------------------------------- the image builder against fa2_rotary_eval
def _rotary_eval64(x, cos_row, sin_row, inter, dt):
    """fa2_rotary_eval on the 64-wide sub-row: the host side of the kernel's arithmetic"""
    lib = _fa2_lib.load()
    xb = x.contiguous()
    y = torch.empty_like(xb)
    c, s = (np.ascontiguousarray(t.float().numpy(), dtype=np.float32) for t in (cos_row, sin_row))
    fp = ctypes.POINTER(ctypes.c_float)
    assert lib.fa2_rotary_eval(F16 if dt == torch.float16 else BF16, xb.data_ptr(), c.ctypes.data_as(fp), s.ctypes.data_as(fp), 64, 64, int(inter), y.data_ptr()) == OK
    return y


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("inter", [True, False], ids=["gptj", "neox"])
@pytest.mark.parametrize("tab", ["f32", "16bit"])
def test_the_image_builder_against_rotary_eval(dt, inter, tab):
    """expect() on a one-sequence cache, row by row against fa2_rotary_eval on k_pe (and on q's tail): bit for bit on every element that is not a NaN,
    and a NaN where fa2_rotary_eval has one (a NaN's payload is not part of the contract).  Rows 0 .. 2 hold subnormals, Inf and NaN."""
    n, H = 12, 3
    kv_c, k_pe, q = ar.inputs(n, H, dt, 11)
    k_pe[1, 3], k_pe[1, 40], q[1, 1, 520] = float("inf"), float("-inf"), float("inf")
    k_pe[2, 5], k_pe[2, 33], q[2, 0, 575] = float("nan"), float("nan"), float("nan")
    cos, sin = ar.tables(20, torch.float32 if tab == "f32" else dt)
    lens = [17]                                                  # positions 5 .. 16
    cache = ar.poisoned((1, 24, 576), dt)
    img, q_out = ar.expect(cache, kv_c, k_pe, ar.uniform_owners(1, n), lens, None, q, cos, sin, inter)

    def same(a, b):
        nan = torch.isnan(b.float())
        return torch.equal(torch.isnan(a.float()), nan) and torch.equal(ar.bits(a)[~nan], ar.bits(b)[~nan])
    for i in range(n):
        p = 17 - n + i
        assert torch.equal(ar.bits(img[0, p, :512]), ar.bits(kv_c[i])), "kv_c lands bit for bit"
        assert same(img[0, p, 512:], _rotary_eval64(k_pe[i], cos[p], sin[p], inter, dt)), (i, p)
        for h in range(H):
            assert torch.equal(ar.bits(q_out[i, h, :512]), ar.bits(q[i, h, :512]))
            assert same(q_out[i, h, 512:], _rotary_eval64(q[i, h, 512:], cos[p], sin[p], inter, dt)), (i, h)
    untouched = [r for r in range(24) if not 5 <= r <= 16]
    assert bool((ar.bits(img[0, untouched]) == ar.POISON).all()) and not torch.equal(ar.bits(img[0, 5:17, 512:]), ar.bits(k_pe))
    assert int(torch.isnan(img[0, 5:17].float()).sum()) >= 2 and float(k_pe[0].float().abs()[k_pe[0] != 0].min()) < 6e-5 * (dt == torch.float16) + 1e-38
    # without tables k_pe is copied; a token outside the cache writes nothing and its q row is still rotated by the clamped table row
    img2, _ = ar.expect(cache, kv_c, k_pe, ar.uniform_owners(1, n), lens)
    assert torch.equal(ar.bits(img2[0, 5:17, 512:]), ar.bits(k_pe))
    img3, q3 = ar.expect(cache, kv_c, k_pe, ar.uniform_owners(1, n), [30], None, q, cos, sin, inter)      # positions 18 .. 29: 24 .. 29 lie outside
    assert bool((ar.bits(img3[0, :18]) == ar.POISON).all()) and torch.equal(ar.bits(img3[0, 18:24, :512]), ar.bits(kv_c[:6]))
    assert same(q3[11, 0, 512:], _rotary_eval64(q[11, 0, 512:], cos[19], sin[19], inter, dt))


# ---------------------------------------------------------------------------------------------------------------- sanitizers, on host code
def test_the_addressing_under_asan_and_ubsan(tmp_path):
    """tools/kvappend_mla_sanitize.cpp: a stand-alone program with its own main that walks every unit of every group through the function the kernels
    call, on sources and a cache allocated to the byte."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the host program cannot be compiled")
    exe = str(tmp_path / "kvappend_mla_sanitize")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(PKG, "csrc"), "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "kvappend_mla_sanitize.cpp"), "-o", exe], check=True, capture_output=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok:"), (res.returncode, res.stdout[-2000:], res.stderr[-4000:])


# ---------------------------------------------------------------------------------------------------------------- the new unit, compiled
def test_no_kernel_of_the_new_unit_has_a_private_segment():
    """kvappend_mla_hip.cpp compiled for gfx950 with the product build's flags, both dtypes: four kernels (the uniform and the packed one, twice), none
    with scratch, none with a dynamic stack."""
    spec = importlib.util.spec_from_file_location("_fa2_build_mla_append", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    units = [u for u in build.UNITS if u[1] == "kvappend_mla_hip.cpp"]
    assert len(units) == 2

    def asm(u):
        flags = [f for f in build.HIPCC_FLAGS if f != "--offload-compress"]
        cmd = [build._hipcc()] + flags + list(u[2]) + ["-I", build.INCLUDE, "-I", build.CSRC, "--cuda-device-only", "-S", os.path.join(build.CSRC, u[1]), "-o", "-"]
        return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    with concurrent.futures.ThreadPoolExecutor(2) as ex:
        texts = list(ex.map(asm, units))
    found = {}
    for text in texts:
        for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
            found[name] = (int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)),
                           int(re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", body).group(1)))
    assert len(found) == 4 and sum("kvappend_mla_kernel" in n for n in found) == 2 and sum("kvappend_mla_varlen_kernel" in n for n in found) == 2, sorted(found)
    assert all(v == (0, 0) for v in found.values()), found
