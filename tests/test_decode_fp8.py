"""CPU tests of decode attention on FP8 (e4m3) KV caches (include/fa2_gfx950.h: fa2_fwd_decode_fp8 and its queries): every validation code of the
new entry and the order they are checked in — the stride-multiple-of-16 and descale-alignment cases included —, the plan and the workspace size
against the stated rule, the argument checks of flash_attention_decode for fp8 caches and descales, and that a 16-bit call with the new keywords
left at None still goes to fa2_fwd_decode.  Nothing here touches a device: every rejected call returns before the launch."""
import ctypes
import os
import re

import pytest
import torch

import decode_calls as dc
from conftest import ROOT
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention_decode

HEADER = os.path.join(ROOT, "include", "fa2_gfx950.h")
FP8_SYMBOLS = ("fa2_fwd_decode_fp8", "fa2_fwd_decode_fp8_plan", "fa2_fwd_decode_fp8_workspace_bytes")
OK, NULLP, SHAPE, HEAD_DIM, ALIGN, DTYPE, SCALE, GRID = 0, -1, -2, -3, -4, -5, -6, -7
F16, BF16 = _fa2_lib.FA2_DTYPE_F16, _fa2_lib.FA2_DTYPE_BF16
E4M3 = torch.float8_e4m3fn


def test_symbols_are_declared_exported_and_bound():
    lib = _fa2_lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in FP8_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _fa2_lib.SYMBOLS, name
        assert getattr(lib, name).argtypes == _fa2_lib.SYMBOLS[name][1]
    # fa2_fwd_decode's list plus the two descale pointers and their stride pair
    assert len(_fa2_lib.SYMBOLS["fa2_fwd_decode_fp8"][1]) == len(_fa2_lib.SYMBOLS["fa2_fwd_decode"][1]) + 3


def _ws(dt, B, H, Hkv, Nq, D, cap, page=0, ns=0):
    return _fa2_lib.load().fa2_fwd_decode_fp8_workspace_bytes(dt, B, H, Hkv, Nq, D, cap, page, ns)


def test_plan_and_workspace_follow_the_stated_rule():
    """Pure host functions of shape, capacity and CU count: row tiles of 16 (three run four), a key tile that divides 64, a forced split honoured,
    B * Hkv * nsplit * rows * (D + 1) * 4 workspace bytes, no split for a grid that covers the chip, no part shorter than 8 key tiles of the capacity."""
    shapes = [(1, 32, 8, 1, 128, 8192, 0), (32, 32, 8, 1, 128, 4096, 0), (4, 8, 8, 1, 64, 16384, 0), (8, 32, 8, 4, 128, 8192, 0), (1, 32, 1, 1, 128, 32, 256),
              (3, 12, 4, 3, 64, 100, 0)]
    for (B, H, Hkv, Nq, D, cap, page) in shapes:
        for dt in (F16, BF16):
            a = _fa2_lib.decode_fp8_plan(dt, B, H, Hkv, Nq, D, cap, page).as_dict()
            assert a == _fa2_lib.decode_fp8_plan(dt, B, H, Hkv, Nq, D, cap, page).as_dict()
            rows = Nq * (H // Hkv)
            assert a["kernel"] == _fa2_lib.FA2_KERNEL_HIP_DECODE and a["key_tile"] in (32, 64)
            assert a["row_tiles"] == {1: 1, 2: 2, 3: 4, 4: 4}[-(-rows // 16)]
            assert 1 <= a["nsplit"] <= 16
            for ns in range(1, 17):
                f = _fa2_lib.decode_fp8_plan(dt, B, H, Hkv, Nq, D, cap, page, ns).as_dict()
                assert f["nsplit"] == ns and f["row_tiles"] == a["row_tiles"] and f["key_tile"] == a["key_tile"]
                assert _ws(dt, B, H, Hkv, Nq, D, cap, page, ns) == (0 if ns == 1 else B * Hkv * ns * rows * (D + 1) * 4)
            assert _ws(dt, B, H, Hkv, Nq, D, cap, page) == (0 if a["nsplit"] == 1 else B * Hkv * a["nsplit"] * rows * (D + 1) * 4)
    for (B, H, Hkv, Nq) in ((32, 32, 8, 1), (256, 8, 1, 1), (64, 16, 1, 4)):
        plan = _fa2_lib.decode_fp8_plan(F16, B, H, Hkv, Nq, 128, 8192)
        assert B * Hkv * plan.row_tiles >= 256 and plan.nsplit == 1 and _ws(F16, B, H, Hkv, Nq, 128, 8192) == 0
    tile = _fa2_lib.decode_fp8_plan(F16, 1, 8, 8, 1, 128, 1024).key_tile
    for cap in (1, tile, 8 * tile, 16 * tile - 1, 16 * tile, 40 * tile):
        assert _fa2_lib.decode_fp8_plan(F16, 1, 8, 8, 1, 128, cap).nsplit == max(1, min(16, -(-cap // tile) // 8)), cap
    # the same codes / 0 for arguments the call would refuse
    lib, plan = _fa2_lib.load(), _fa2_lib.DecodePlan()
    assert lib.fa2_fwd_decode_fp8_plan(F16, 2, 8, 2, 1, 128, 256, 0, 0, None) == NULLP
    assert lib.fa2_fwd_decode_fp8_plan(F16, 2, 8, 2, 17, 96, 256, 0, 0, ctypes.byref(plan)) == SHAPE
    assert lib.fa2_fwd_decode_fp8_plan(7, 2, 8, 2, 1, 96, 256, 0, 0, ctypes.byref(plan)) == HEAD_DIM
    assert lib.fa2_fwd_decode_fp8_plan(7, 2, 8, 2, 1, 128, 256, 0, 0, ctypes.byref(plan)) == DTYPE
    assert _ws(F16, 2, 8, 2, 17, 128, 256, 0, 4) == 0 and _ws(7, 2, 8, 2, 1, 128, 256, 0, 4) == 0


P = dc.HOST                                  # 16-byte aligned host memory that no call here ever touches
DEFAULTS = dict(dtype=F16, q=P, k=P, v=P, o=P, lse=P, lens=P, bt=None, B=2, H=8, Hkv=2, Nq=1, D=128, cap=256, page=0, pages=0,
                qs=_fa2_lib.strides3(1024, 128, 1024), ks=_fa2_lib.strides3(256 * 256, 128, 256), vs=_fa2_lib.strides3(256 * 256, 128, 256),
                os=_fa2_lib.strides3(1024, 128, 1024), ls=_fa2_lib.strides2(8, 1), bts=0, scale=0.1, kd=P, vd=P, ds=_fa2_lib.strides2(2, 1), ns=1, ws=None, wsb=0)


def _call(**kw):
    """fa2_fwd_decode_fp8 on host memory that is never touched: every call here is refused before the launch."""
    return dc.host_call("fp8", DEFAULTS, **kw)


def test_every_error_code():
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    s3, s2 = _fa2_lib.strides3, _fa2_lib.strides2
    for name in ("q", "k", "v", "o", "lse", "lens", "qs", "ks", "vs", "os", "ls"):
        assert _call(**{name: None}) == NULLP, name
    assert _call(page=64, pages=4, bt=None) == NULLP
    # the stride pair is needed as soon as one descale is given, and only then
    assert _call(ds=None) == NULLP and _call(kd=None, ds=None) == NULLP and _call(vd=None, ds=None) == NULLP
    for kw in (dict(B=0), dict(H=0), dict(Hkv=0), dict(Nq=0), dict(D=0), dict(cap=0), dict(H=8, Hkv=3), dict(H=2, Hkv=4), dict(Nq=17), dict(H=128, Hkv=1),
               dict(page=48, pages=4, bt=p), dict(page=-64, pages=4, bt=p), dict(page=32, pages=4, bt=p), dict(ns=17), dict(ns=-1),
               dict(page=64, pages=0, bt=p), dict(ls=s2(-8, 1)), dict(ds=s2(-2, 1)), dict(ds=s2(2, -1))):
        assert _call(**kw) == SHAPE, kw
    for D in (96, 32, 256, 8, 129):
        assert _call(D=D) == HEAD_DIM, D
    for kw in (dict(q=p + 8), dict(k=p + 8), dict(v=p + 8), dict(o=p + 4), dict(lse=p + 2), dict(lens=p + 1), dict(page=64, pages=4, bt=p + 2),
               dict(qs=s3(1024, 132, 1024)), dict(os=s3(-1024, 128, 1024)), dict(page=64, pages=4, bt=p, bts=-4),
               dict(ks=s3(65536, 128, 0)), dict(vs=s3(65536, 128, 260)),
               # cache strides are multiples of 16: a multiple of 8 is not enough for an e4m3 cache, in any of the three places, K or V
               dict(ks=s3(65536 + 8, 128, 256)), dict(ks=s3(65536, 136, 256)), dict(ks=s3(65536, 128, 264)),
               dict(vs=s3(65536 + 8, 128, 256)), dict(vs=s3(65536, 136, 256)), dict(vs=s3(65536, 128, 264)),
               # 4-byte descales
               dict(kd=p + 2), dict(vd=p + 1), dict(kd=None, vd=p + 2), dict(kd=p + 3, vd=None)):
        assert _call(**kw) == ALIGN, kw
    # ... while q and o keep multiples of 8, and descale strides are free
    assert _call(qs=s3(1024 + 8, 136, 1024 + 8), os=s3(1024 + 8, 136, 1024 + 8), ds=s2(3, 5), scale=float("nan")) == SCALE
    assert _call(dtype=2) == DTYPE and _call(dtype=-1) == DTYPE
    assert _call(scale=float("nan")) == SCALE and _call(scale=float("inf")) == SCALE
    assert _call(B=65536) == GRID
    need = _ws(F16, 2, 8, 2, 1, 128, 256, 0, 2)
    assert need == 2 * 2 * 2 * 4 * 129 * 4
    assert _call(ns=2, ws=None) == NULLP
    assert _call(ns=2, ws=p + 4, wsb=need) == ALIGN
    assert _call(ns=2, ws=p, wsb=need - 1) == SHAPE
    # both descales null: the stride pair may be null too (the call gets as far as the scale check)
    assert _call(kd=None, vd=None, ds=None, scale=float("nan")) == SCALE


def test_error_precedence():
    """null pointer, shape, head dim, alignment, dtype, scale, grid, workspace — fa2_fwd_decode's order: a call with two defects reports the earlier."""
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    defects = [(NULLP, dict(ds=None)), (SHAPE, dict(Nq=17)), (HEAD_DIM, dict(D=96)), (ALIGN, dict(ks=_fa2_lib.strides3(65536, 128, 264))),
               (DTYPE, dict(dtype=7)), (SCALE, dict(scale=float("nan"))), (GRID, dict(B=65536)), (NULLP, dict(ns=2, ws=None))]
    for i, (code, kw) in enumerate(defects):
        assert _call(**kw) == code
        for (_, later) in defects[i + 1:]:
            assert _call(**dict(later, **kw)) == code, (kw, later)
    assert _call(kd=p + 2, dtype=7) == ALIGN and _call(kd=p + 2, D=96) == HEAD_DIM and _call(ds=_fa2_lib.strides2(-1, 1), kd=p + 2) == SHAPE


def _args(B=2, Nq=1, H=8, Hkv=2, D=128, Nmax=128, dt=torch.float16, cache=E4M3):
    q = torch.zeros(B, Nq, H, D, dtype=dt)
    k, v = (torch.zeros(B, Nmax, Hkv, D, dtype=torch.float16).to(cache) for _ in range(2))
    return q, k, v, torch.ones(B, dtype=torch.int32)


def test_python_argument_checks():
    """Raised before any device work: CPU tensors reach the checks."""
    q, k, v, lens = _args()
    kd = torch.ones(2, 2)
    with pytest.raises(ValueError, match="one dtype"):                   # mixed cache dtypes, either way round
        flash_attention_decode(q, k, v.to(torch.float16), lens)
    with pytest.raises(ValueError, match="one dtype"):
        flash_attention_decode(q, k.to(torch.float16), v, lens)
    for other in (torch.float8_e5m2, torch.float8_e4m3fnuz):
        with pytest.raises(ValueError, match="e5m2 and the fnuz formats"):
            flash_attention_decode(q, k.to(torch.float16).to(other), v.to(torch.float16).to(other), lens)
    with pytest.raises(ValueError, match="fp16 or bf16 q"):               # q stays a 16-bit tensor
        flash_attention_decode(q.to(E4M3), k, v, lens)
    q16, k16, v16, _ = _args(cache=torch.float16)
    with pytest.raises(ValueError, match="descale.*float8_e4m3fn caches"):      # a descale with a 16-bit cache
        flash_attention_decode(q16, k16, v16, lens, k_descale=kd)
    with pytest.raises(ValueError, match="descale.*float8_e4m3fn caches"):
        flash_attention_decode(q16, k16, v16, lens, v_descale=kd)
    for bad in (torch.ones(2, 3), torch.ones(2), torch.ones(2, 2, 1), torch.ones(2, 2, dtype=torch.float64), torch.ones(2, 2, dtype=torch.float16), 1.0):
        with pytest.raises(ValueError, match=r"float32 tensors of shape \[B, Hkv\]"):
            flash_attention_decode(q, k, v, lens, k_descale=bad)
        with pytest.raises(ValueError, match=r"float32 tensors of shape \[B, Hkv\]"):
            flash_attention_decode(q, k, v, lens, k_descale=kd, v_descale=bad)
    with pytest.raises(ValueError, match="head dims 64 and 128"):
        flash_attention_decode(*_args(D=96))
    with pytest.raises(ValueError, match="multiple of 64"):
        pool = torch.zeros(8, 48, 2, 128, dtype=torch.float16).to(E4M3)
        flash_attention_decode(q, pool, pool, lens, block_table=torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="ROCm device"):               # everything in order: only the device is missing
        flash_attention_decode(q, k, v, lens, k_descale=kd, v_descale=kd)
    with pytest.raises(RuntimeError, match="ROCm device"):
        flash_attention_decode(q, k, v, lens)


def test_cache_strides_must_be_multiples_of_16(monkeypatch):
    """An e4m3 cache view whose strides are multiples of 8 only (fine for a 16-bit cache) is refused with a ValueError, never copied.  (The tensors
    are CPU tensors that claim a ROCm device, so that the call gets past the device check; it is refused before any device work.)"""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    q, k, _, lens = _args(Nmax=64)
    n = 64 * 2 * 128
    flat = torch.zeros(2 * n + 4096, dtype=torch.float16).to(E4M3)
    views = [torch.zeros(2, 64, 2, 136, dtype=torch.float16).to(E4M3)[..., :128],       # head stride 136, row stride 272
             flat.as_strided((2, 64, 2, 128), (n + 8, 256, 128, 1)),                    # batch stride + 8
             flat.as_strided((2, 64, 2, 128), (n + 1024, 264, 128, 1))]                 # row stride 264
    for kv in views:
        assert all(s % 8 == 0 for s in kv.stride()[:3]) and any(s % 16 for s in kv.stride()[:3])
        for (kk, vv) in ((kv, kv), (k, kv), (kv, k)):
            with pytest.raises(ValueError, match="multiples of 16 elements"):
                flash_attention_decode(q, kk, vv, lens)
    off = flat[8:].as_strided((2, 64, 2, 128), (n, 256, 128, 1))                        # storage 8 bytes off a 16-byte boundary
    assert off.data_ptr() % 16 == 8
    with pytest.raises(ValueError, match="16-byte"):
        flash_attention_decode(q, off, off, lens)


TAGS = {"fa2_fwd_decode_workspace_bytes": "ws16", "fa2_fwd_decode_fp8_workspace_bytes": "ws8", "fa2_fwd_decode": "decode", "fa2_fwd_decode_fp8": "decode_fp8"}


def _brief(calls):
    """Which decode entry the operator reached and with how many arguments; the fp8 entry with its descale pointers and their stride pair.  (Another
    symbol than these four is a KeyError.)"""
    out = []
    for name, a in calls:
        row = (TAGS[name], len(a))
        if name == "fa2_fwd_decode_fp8":
            ds = dc.arg("fp8", a, "ds")
            row += (dc.arg("fp8", a, "kd"), dc.arg("fp8", a, "vd"), None if ds is None else tuple(ds))
        out.append(row)
    return out


@pytest.fixture
def recorder(monkeypatch):
    return dc.recording_lib(monkeypatch)


def test_a_16_bit_call_reaches_fa2_fwd_decode_as_before(recorder):
    """k_descale=None, v_descale=None with a 16-bit cache is the call as it was: fa2_fwd_decode with its 27 arguments, the fp8 entry untouched."""
    q, k, v, lens = _args(cache=torch.float16)
    o = flash_attention_decode(q, k, v, lens, k_descale=None, v_descale=None)
    assert o.shape == q.shape and o.dtype == q.dtype
    assert _brief(recorder.calls) == [("ws16", 9), ("decode", len(_fa2_lib.SYMBOLS["fa2_fwd_decode"][1]))]


def test_an_fp8_call_reaches_the_new_entry_with_the_descales_passed_through(recorder):
    q, k, v, lens = _args()
    wide = torch.ones(2, 6)
    kd, vd = wide[:, 0:4:2], wide[:, 1:5:2]                             # [2, 2] views, strides (6, 2)
    flash_attention_decode(q, k, v, lens, k_descale=kd, v_descale=vd)
    flash_attention_decode(q, k, v, lens, v_descale=vd)
    flash_attention_decode(q, k, v, lens)
    n = len(_fa2_lib.SYMBOLS["fa2_fwd_decode_fp8"][1])
    assert _brief(recorder.calls) == [("ws8", 9), ("decode_fp8", n, kd.data_ptr(), vd.data_ptr(), (6, 2)), ("ws8", 9), ("decode_fp8", n, None, vd.data_ptr(), (6, 2)),
                              ("ws8", 9), ("decode_fp8", n, None, None, None)]
