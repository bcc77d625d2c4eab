"""CPU tests of decode attention at head dim 256 (include/fa2_gfx950.h: fa2_fwd_decode_wide and its queries): the bindings, every validation code and
the order they are checked in (fa2_fwd_decode_window's, with D = 128 as the head-dim defect), the plan's rule for a kernel that runs one workgroup of at
most 32 rows per CU, the workspace, and the operator's routing.  Nothing here touches a device: every rejected call returns before the launch."""
import ctypes

import pytest
import torch

import decode_calls as dc
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention_decode

OK, NULLP, SHAPE, HEAD_DIM, ALIGN, DTYPE, SCALE, GRID, SOFTCAP = 0, -1, -2, -3, -4, -5, -6, -7, -10
F16, BF16 = _fa2_lib.FA2_DTYPE_F16, _fa2_lib.FA2_DTYPE_BF16
C16, C8 = _fa2_lib.FA2_CACHE_16BIT, _fa2_lib.FA2_CACHE_E4M3
P = dc.HOST                                  # 16-byte aligned host memory that no call here ever touches
DEFAULTS = dict(dtype=F16, fmt=C16, q=P, k=P, v=P, o=P, lse=P, lens=P, bt=None, B=2, H=8, Hkv=2, Nq=1, D=256, cap=256, page=0, pages=0,
                qs=_fa2_lib.strides3(2048, 256, 2048), ks=_fa2_lib.strides3(256 * 512, 256, 512), vs=_fa2_lib.strides3(256 * 512, 256, 512),
                os=_fa2_lib.strides3(2048, 256, 2048), ls=_fa2_lib.strides2(8, 1), bts=0, scale=0.1, kd=None, vd=None, ds=None, wl=31, cap_=8.0, sl=P, st=8,
                ns=1, ws=None, wsb=0)


def _call(**kw):
    return dc.host_call("wide", DEFAULTS, **kw)


def _plan(dt, B, H, Hkv, Nq, D, cap, page=0, ns=0, wl=-1):
    plan = _fa2_lib.DecodePlan()
    _fa2_lib.check(_fa2_lib.load().fa2_fwd_decode_wide_plan(dt, B, H, Hkv, Nq, D, cap, page, ns, wl, ctypes.byref(plan)))
    return plan


def _ws(dt, B, H, Hkv, Nq, D, cap, page=0, ns=0, wl=-1):
    return _fa2_lib.load().fa2_fwd_decode_wide_workspace_bytes(dt, B, H, Hkv, Nq, D, cap, page, ns, wl)


def test_every_error_code_and_their_precedence():
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    s2, s3 = _fa2_lib.strides2, _fa2_lib.strides3
    for name, nargs in (("fa2_fwd_decode_wide", 35), ("fa2_fwd_decode_wide_plan", 11), ("fa2_fwd_decode_wide_workspace_bytes", 10)):      # bound as declared
        assert len(_fa2_lib.SYMBOLS[name][1]) == nargs and getattr(_fa2_lib.load(), name).argtypes == _fa2_lib.SYMBOLS[name][1], name
    assert _fa2_lib.SYMBOLS["fa2_fwd_decode_wide"] == _fa2_lib.SYMBOLS["fa2_fwd_decode_window"]
    for D in (128, 64, 96, 512, 8, 257):            # 64 and 128 belong to the older entries
        assert _call(D=D) == HEAD_DIM, D
    assert _call(page=64, pages=4, bt=None) == NULLP and _call(fmt=C8, kd=p, ds=None) == NULLP and _call(H=128, Hkv=1) == SHAPE
    assert _call(qs=s3(2048, 260, 2048)) == ALIGN and _call(fmt=C8, ks=s3(131072, 256, 520)) == ALIGN
    need = _ws(F16, 2, 8, 2, 1, 256, 256, 0, 2, 31)
    assert need == 2 * 2 * 2 * 4 * 257 * 4
    assert _call(ns=2, ws=None) == NULLP and _call(ns=2, ws=p + 4, wsb=need) == ALIGN and _call(ns=2, ws=p, wsb=need - 1) == SHAPE
    assert _call(wl=-1, cap_=0.0, sl=None, st=0, ns=2, ws=p, wsb=need - 1) == SHAPE
    # null pointer, sizes, head dim, alignment, dtype, scale, softcap, grid, workspace: a call with two defects reports the earlier one
    chains = [
        [(NULLP, dict(q=None)), (SHAPE, dict(wl=-2)), (HEAD_DIM, dict(D=128)), (ALIGN, dict(sl=p + 2)), (DTYPE, dict(fmt=3)), (SCALE, dict(scale=float("nan"))),
         (SOFTCAP, dict(cap_=-1.0)), (GRID, dict(B=65536)), (NULLP, dict(ns=2, ws=None))],
        [(NULLP, dict(lens=None)), (SHAPE, dict(st=-4)), (HEAD_DIM, dict(D=128)), (ALIGN, dict(k=p + 8)), (DTYPE, dict(kd=p, ds=s2(2, 1))),
         (SCALE, dict(scale=float("inf"))), (SOFTCAP, dict(cap_=float("nan"))), (GRID, dict(B=65536)), (NULLP, dict(ns=2, ws=None))],
    ]
    for defects in chains:
        for i, (code, kw) in enumerate(defects):
            assert _call(**kw) == code, kw
            for (_, later) in defects[i + 1:]:
                assert _call(**dict(later, **kw)) == code, (kw, later)
    assert _call(D=128, wl=-2) == SHAPE and _call(D=128, ns=17) == SHAPE
    plan = _fa2_lib.DecodePlan()                     # the queries answer with the call's codes / with 0
    assert _fa2_lib.load().fa2_fwd_decode_wide_plan(7, 2, 8, 2, 1, 128, 256, 0, 0, 5, ctypes.byref(plan)) == HEAD_DIM and _ws(F16, 2, 8, 2, 1, 128, 256, 0, 4) == 0


# (B, H, Hkv, Nq, capacity, page size, window_left) -> (parts, row tiles per workgroup), by the header's rule at the 256 CUs the library answers for without a
# device: one workgroup per CU over B * Hkv * ceil(rows / 32) items, at most 16 parts, at most one per 8 key tiles of the span a sequence can sweep
PLANS = [((32, 16, 8, 1, 4096, 0, -1), (1, 1)), ((1, 16, 8, 1, 32768, 0, -1), (16, 1)), ((1, 16, 8, 1, 32768, 0, 1023), (4, 1)),      # 33 tiles of span
         ((3, 17, 1, 1, 2048, 0, -1), (8, 2)), ((20, 32, 1, 1, 8192, 0, -1), (12, 2)), ((20, 64, 1, 1, 8192, 0, -1), (6, 2)),         # 17, 32, 64 rows
         ((5, 11, 1, 3, 64, 64, -1), (16, 2)), ((5, 11, 1, 3, 64, 64, 31), (1, 2))]                                                 # 33 rows, paged


@pytest.mark.parametrize("shape,want", PLANS)
def test_plan_and_workspace(shape, want):
    B, H, Hkv, Nq, cap, page, wl = shape
    plan = _plan(BF16, B, H, Hkv, Nq, 256, cap, page, 0, wl)
    assert (plan.nsplit, plan.row_tiles) == want and plan.key_tile == 32 and plan.kernel == _fa2_lib.FA2_KERNEL_HIP_DECODE
    assert _ws(BF16, B, H, Hkv, Nq, 256, cap, page, 0, wl) == (0 if want[0] == 1 else B * Hkv * want[0] * Nq * (H // Hkv) * 257 * 4)
    assert _plan(F16, B, H, Hkv, Nq, 256, cap, page, 5, wl).nsplit == 5       # a forced split is honoured


def test_operator_routes_256_to_the_wide_entry(monkeypatch):
    z = lambda *s: torch.zeros(*s, dtype=torch.float16)      # noqa: E731
    lens = torch.ones(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="ROCm device"):    # CPU tensors get past the head-dim check
        flash_attention_decode(z(2, 1, 8, 256), z(2, 128, 2, 256), z(2, 128, 2, 256), lens)
    with pytest.raises(ValueError, match="head dims 64 and 128.*flash_attention_varlen"):
        flash_attention_decode(z(2, 1, 8, 96), z(2, 128, 2, 96), z(2, 128, 2, 96), lens)
    seen = dc.recording_lib(monkeypatch).calls
    flash_attention_decode(z(2, 1, 8, 256), z(2, 128, 2, 256), z(2, 128, 2, 256), lens)
    flash_attention_decode(z(2, 1, 8, 256), z(2, 128, 2, 256), z(2, 128, 2, 256), lens, window=5, softcap=8.0)
    flash_attention_decode(z(2, 1, 8, 128), z(2, 128, 2, 128), z(2, 128, 2, 128), lens)
    assert [n for n, _ in seen] == ["fa2_fwd_decode_wide_workspace_bytes", "fa2_fwd_decode_wide"] * 2 + ["fa2_fwd_decode_workspace_bytes", "fa2_fwd_decode"]
    assert all(len(a) == len(_fa2_lib.SYMBOLS[n][1]) for n, a in seen)
    assert seen[1][1][27:29] == (-1, 0.0) and seen[3][1][27:29] == (5, 8.0) and seen[2][1][-1] == 5 and seen[1][1][13] == 256
