"""CPU tests of decode attention with a sliding window, soft-capping and ALiBi slopes (include/fa2_gfx950.h: fa2_fwd_decode_window and its queries): the
part range the kernel and the host share (fa2_decode_window_part_range, csrc/fa2_decode.hip.h) exhaustively against its definition, the plan's span rule
and the workspace, every validation code of the new entry and the order they are checked in, the operator's argument checks — and the feature margin of
every parity case of tests/test_decode_window_gpu.py, computed on float64 alone before any GPU exists.  Nothing here touches a device: every rejected
call returns before the launch, and the Python checks run before any device work."""
import ctypes
import os
import re

import pytest
import torch

import decode_window_refs as wr
import decode_calls as dc
from conftest import ROOT
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention_decode

HEADER = os.path.join(ROOT, "include", "fa2_gfx950.h")
SYMBOLS = ("fa2_fwd_decode_window", "fa2_fwd_decode_window_plan", "fa2_fwd_decode_window_workspace_bytes", "fa2_decode_window_part_range")
OK, NULLP, SHAPE, HEAD_DIM, ALIGN, DTYPE, SCALE, GRID, SOFTCAP = 0, -1, -2, -3, -4, -5, -6, -7, -10
F16, BF16 = _fa2_lib.FA2_DTYPE_F16, _fa2_lib.FA2_DTYPE_BF16
C16, C8 = _fa2_lib.FA2_CACHE_16BIT, _fa2_lib.FA2_CACHE_E4M3
WINDOWS = (-1, 0, 1, 31, 32, 33, 100, 1000)
TILE = 32


def test_symbols_are_declared_exported_and_bound():
    lib = _fa2_lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _fa2_lib.SYMBOLS, name
        assert getattr(lib, name).argtypes == _fa2_lib.SYMBOLS[name][1]


def test_part_range_exhaustive():
    """len 0 .. 300, Nq 1 .. 4, eight windows, 1 .. 16 parts of 32-key tiles: the parts are disjoint, ordered and cover exactly [lo / 32, ceil(len / 32));
    every key some row keeps lies in a swept tile, no swept tile lies wholly below lo, and window_left = -1 is fa2_decode_part_range."""
    assert _fa2_lib.decode_window_plan(F16, 1, 8, 8, 1, 128, 1024).key_tile == TILE
    pr, old = _fa2_lib.decode_window_part_range, _fa2_lib.decode_part_range
    for wl in WINDOWS:
        for Nq in range(1, 5):
            for length in range(0, 301):
                lo = wr.window_lo(length, Nq, wl)
                t0, t1 = lo // TILE, -(-length // TILE)
                # the keys some row keeps: row i at pos = length - Nq + i keeps [max(0, pos - wl), pos]
                kept = set()
                for i in range(Nq):
                    pos = length - Nq + i
                    if pos >= 0:
                        kept.update(range(max(0, pos - wl) if wl >= 0 else 0, pos + 1))
                assert not kept or min(kept) == lo
                for nsplit in range(1, 17):
                    per = -(-(t1 - t0) // nsplit)
                    nxt, swept = t0, set()
                    for part in range(nsplit):
                        first, n = pr(length, 4096, Nq, wl, TILE, nsplit, part)
                        assert 0 <= n <= per
                        if n:
                            assert first == nxt == t0 + part * per, (wl, Nq, length, nsplit, part, first, n)
                            nxt = first + n
                            swept.update(range(first, first + n))
                        else:
                            assert t0 + part * per >= t1, (wl, Nq, length, nsplit, part)
                        if wl == -1:
                            assert (first, n) == old(length, 4096, Nq, TILE, nsplit, part)
                    assert nxt == max(t0, t1) and swept == set(range(t0, t1)), (wl, Nq, length, nsplit)
                    assert all(j // TILE in swept for j in kept)
                    assert all((t + 1) * TILE > lo for t in swept)


def test_part_range_clamps_the_length():
    pr = _fa2_lib.decode_window_part_range
    for wl in (-1, 0, 31, 100):
        for nsplit in (1, 3, 16):
            for part in range(nsplit):
                assert pr(10 ** 9, 200, 1, wl, TILE, nsplit, part) == pr(200, 200, 1, wl, TILE, nsplit, part)       # above the capacity
                assert pr(2 ** 40, 200, 3, wl, TILE, nsplit, part) == pr(200, 200, 3, wl, TILE, nsplit, part)
                assert pr(-5, 200, 1, wl, TILE, nsplit, part) == (0, 0) == pr(-2 ** 40, 200, 1, wl, TILE, nsplit, part)    # negative
                assert pr(300, 0, 1, wl, TILE, nsplit, part) == (0, 0)
    # a clamped sweep never passes the capacity's last tile, and under a window it starts at the clamped length's window
    for cap in (1, 63, 64, 65, 1000):
        first, n = pr(2 ** 31 - 1, cap, 1, 10, TILE, 1, 0)
        assert (first + n) * TILE < cap + TILE and first == max(0, cap - 1 - 10) // TILE
    # the largest legal window and capacity: no overflow
    assert pr(2 ** 31 - 1, 2 ** 31 - 1, 1, 2 ** 31 - 1, TILE, 1, 0) == (0, 2 ** 26)


def test_part_range_argument_codes():
    lib = _fa2_lib.load()
    a, b = ctypes.c_int(), ctypes.c_int()
    ra, rb = ctypes.byref(a), ctypes.byref(b)
    assert lib.fa2_decode_window_part_range(100, 200, 1, 5, 32, 2, 0, None, rb) == NULLP
    assert lib.fa2_decode_window_part_range(100, 200, 1, 5, 32, 2, 0, ra, None) == NULLP
    for args in ((100, -1, 1, 5, 32, 2, 0), (100, 200, 0, 5, 32, 2, 0), (100, 200, 1, 5, 0, 2, 0), (100, 200, 1, 5, 32, 0, 0), (100, 200, 1, 5, 32, 17, 0),
                 (100, 200, 1, 5, 32, 2, 2), (100, 200, 1, 5, 32, 2, -1), (100, 200, 1, -2, 32, 2, 0)):
        assert lib.fa2_decode_window_part_range(*args, ra, rb) == SHAPE, args
    assert lib.fa2_decode_window_part_range(100, 200, 1, -1, 32, 16, 15, ra, rb) == OK
    assert lib.fa2_decode_window_part_range(100, 200, 1, 0, 32, 16, 15, ra, rb) == OK


def _ws(dt, B, H, Hkv, Nq, D, cap, page=0, ns=0, wl=-1):
    return _fa2_lib.load().fa2_fwd_decode_window_workspace_bytes(dt, B, H, Hkv, Nq, D, cap, page, ns, wl)


GRID_SHAPES = [(1, 32, 8, 1, 128, 8192, 0), (32, 32, 8, 1, 128, 4096, 0), (4, 8, 8, 1, 64, 16384, 0), (8, 32, 8, 4, 128, 8192, 0), (1, 32, 1, 1, 128, 32, 256),
               (3, 12, 4, 3, 64, 100, 0), (1, 8, 8, 1, 128, 700, 0), (2, 16, 1, 4, 128, 64, 64)]


def test_plan_and_workspace_without_a_window_are_the_plain_ones():
    lib = _fa2_lib.load()
    for (B, H, Hkv, Nq, D, cap, page) in GRID_SHAPES:
        for dt in (F16, BF16):
            for ns in (0, 1, 2, 7, 16):
                a = _fa2_lib.decode_plan(dt, B, H, Hkv, Nq, D, cap, page, ns).as_dict()
                assert _fa2_lib.decode_window_plan(dt, B, H, Hkv, Nq, D, cap, page, ns, -1).as_dict() == a
                assert _ws(dt, B, H, Hkv, Nq, D, cap, page, ns) == lib.fa2_fwd_decode_workspace_bytes(dt, B, H, Hkv, Nq, D, cap, page, ns)
                # a window wider than the capacity changes nothing
                keys = cap * page if page else cap
                for wl in (keys - 1, keys, keys + 5, 2 ** 31 - 1):
                    assert _fa2_lib.decode_window_plan(dt, B, H, Hkv, Nq, D, cap, page, ns, wl).as_dict() == a, (B, H, Hkv, Nq, D, cap, page, ns, wl)
                    assert _ws(dt, B, H, Hkv, Nq, D, cap, page, ns, wl) == lib.fa2_fwd_decode_workspace_bytes(dt, B, H, Hkv, Nq, D, cap, page, ns)


def _rule(B, Hkv, row_tiles, cap_keys, Nq, wl, cus=256):
    """The split rule of the header, computed here: the part cap follows the span a sequence can sweep."""
    work = B * Hkv * row_tiles
    if work >= cus:
        return 1
    span = -(-cap_keys // TILE)
    if wl >= 0:
        span = min(span, -(-(wl + Nq) // TILE) + 1)
    return max(1, min(2 * cus // work, 16, span // 8))


def test_plan_part_cap_follows_the_span_of_the_window():
    """(Without a device the library answers for 256 CUs, as tests/test_decode.py relies on.)"""
    # B1 Hkv8, a 32k cache, a 1 024-key window: 33 tiles of span -> 4 parts, not 16 parts of two tiles each
    plan = _fa2_lib.decode_window_plan(F16, 1, 32, 8, 1, 128, 32768, 0, 0, 1023)
    assert plan.nsplit == _rule(1, 8, 1, 32768, 1, 1023) == 4 and plan.row_tiles == 1 and plan.key_tile == TILE
    assert _fa2_lib.decode_plan(F16, 1, 32, 8, 1, 128, 32768).nsplit == 16
    assert _ws(F16, 1, 32, 8, 1, 128, 32768, 0, 0, 1023) == 1 * 8 * 4 * 4 * 129 * 4
    for (B, H, Hkv, Nq, D, cap, page) in GRID_SHAPES:
        keys = cap * page if page else cap
        for wl in (0, 1, 31, 100, 223, 224, 255, 256, 1023, 4095, 100000):
            plan = _fa2_lib.decode_window_plan(BF16, B, H, Hkv, Nq, D, cap, page, 0, wl)
            assert plan.nsplit == _rule(B, Hkv, plan.row_tiles, keys, Nq, wl), (B, H, Hkv, Nq, D, cap, page, wl)
            rows = Nq * (H // Hkv)
            assert _ws(BF16, B, H, Hkv, Nq, D, cap, page, 0, wl) == (0 if plan.nsplit == 1 else B * Hkv * plan.nsplit * rows * (D + 1) * 4)
            for ns in (1, 5, 16):                       # a forced split is honoured under a window too
                assert _fa2_lib.decode_window_plan(BF16, B, H, Hkv, Nq, D, cap, page, ns, wl).nsplit == ns
    # the queries answer with the call's codes / with 0
    plan, lib = _fa2_lib.DecodePlan(), _fa2_lib.load()
    assert lib.fa2_fwd_decode_window_plan(F16, 2, 8, 2, 1, 128, 256, 0, 0, 5, None) == NULLP
    assert lib.fa2_fwd_decode_window_plan(F16, 2, 8, 2, 1, 128, 256, 0, 0, -2, ctypes.byref(plan)) == SHAPE
    assert lib.fa2_fwd_decode_window_plan(F16, 2, 8, 2, 17, 96, 256, 0, 0, 5, ctypes.byref(plan)) == SHAPE
    assert lib.fa2_fwd_decode_window_plan(7, 2, 8, 2, 1, 96, 256, 0, 0, 5, ctypes.byref(plan)) == HEAD_DIM
    assert lib.fa2_fwd_decode_window_plan(7, 2, 8, 2, 1, 128, 256, 0, 0, 5, ctypes.byref(plan)) == DTYPE
    assert _ws(F16, 2, 8, 2, 1, 128, 256, 0, 4, -2) == 0 and _ws(7, 2, 8, 2, 1, 128, 256, 0, 4, 5) == 0


P = dc.HOST                                  # 16-byte aligned host memory that no call here ever touches
DEFAULTS = dict(dtype=F16, fmt=C16, q=P, k=P, v=P, o=P, lse=P, lens=P, bt=None, B=2, H=8, Hkv=2, Nq=1, D=128, cap=256, page=0, pages=0,
                qs=_fa2_lib.strides3(1024, 128, 1024), ks=_fa2_lib.strides3(256 * 256, 128, 256), vs=_fa2_lib.strides3(256 * 256, 128, 256),
                os=_fa2_lib.strides3(1024, 128, 1024), ls=_fa2_lib.strides2(8, 1), bts=0, scale=0.1, kd=None, vd=None, ds=None, wl=31, cap_=8.0, sl=P, st=8,
                ns=1, ws=None, wsb=0)


def _call(**kw):
    """fa2_fwd_decode_window on host memory that is never touched: every call here is refused before the launch."""
    return dc.host_call("window", DEFAULTS, **kw)


def test_every_error_code():
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    s2 = _fa2_lib.strides2
    for name in ("q", "k", "v", "o", "lse", "lens", "qs", "ks", "vs", "os", "ls"):
        assert _call(**{name: None}) == NULLP, name
    assert _call(page=64, pages=4, bt=None) == NULLP                     # a paged call needs its block table
    assert _call(fmt=C8, kd=p, ds=None) == NULLP and _call(fmt=C8, vd=p, ds=None) == NULLP     # a descale needs the strides
    for kw in (dict(B=0), dict(H=0), dict(Hkv=0), dict(Nq=0), dict(D=0), dict(cap=0), dict(H=8, Hkv=3), dict(H=2, Hkv=4), dict(Nq=17), dict(H=128, Hkv=1),
               dict(page=48, pages=4, bt=p), dict(page=-64, pages=4, bt=p), dict(page=32, pages=4, bt=p), dict(ns=17), dict(ns=-1),
               dict(page=64, pages=0, bt=p), dict(ls=s2(-8, 1)), dict(wl=-2), dict(wl=-2 ** 31), dict(st=-1), dict(st=-8, sl=None),
               dict(fmt=C8, kd=p, ds=s2(-2, 1))):
        assert _call(**kw) == SHAPE, kw
    for D in (96, 32, 256, 8, 129):
        assert _call(D=D) == HEAD_DIM, D
    for kw in (dict(q=p + 8), dict(k=p + 2), dict(v=p + 8), dict(o=p + 4), dict(lse=p + 2), dict(lens=p + 1), dict(page=64, pages=4, bt=p + 2),
               dict(qs=_fa2_lib.strides3(1024, 132, 1024)), dict(ks=_fa2_lib.strides3(65536, 128, 0)), dict(vs=_fa2_lib.strides3(65536, 128, 260)),
               dict(os=_fa2_lib.strides3(-1024, 128, 1024)), dict(page=64, pages=4, bt=p, bts=-4), dict(sl=p + 2), dict(sl=p + 1),
               dict(fmt=C8, ks=_fa2_lib.strides3(65536, 128, 264)), dict(fmt=C8, kd=p + 2, ds=s2(2, 1))):
        assert _call(**kw) == ALIGN, kw
    assert _call(dtype=2) == DTYPE and _call(dtype=-1) == DTYPE
    assert _call(fmt=2) == DTYPE and _call(fmt=-1) == DTYPE                                  # a cache format that is neither constant
    assert _call(kd=p, ds=s2(2, 1)) == DTYPE and _call(vd=p, ds=s2(2, 1)) == DTYPE           # descales with a 16-bit cache
    assert _call(scale=float("nan")) == SCALE and _call(scale=float("inf")) == SCALE
    for bad in (-1.0, float("nan"), float("inf"), -float("inf"), 1e-39):
        assert _call(cap_=bad) == SOFTCAP, bad
    assert _call(B=65536) == GRID
    # the workspace of a split call: checked last
    need = _ws(F16, 2, 8, 2, 1, 128, 256, 0, 2, 31)
    assert need == 2 * 2 * 2 * 4 * 129 * 4
    assert _call(ns=2, ws=None) == NULLP
    assert _call(ns=2, ws=p + 4, wsb=need) == ALIGN
    assert _call(ns=2, ws=p, wsb=need - 1) == SHAPE
    # ... also of a call that runs the plain kernels (no window, no cap, no slopes)
    assert _call(wl=-1, cap_=0.0, sl=None, st=0, ns=2, ws=p, wsb=need - 1) == SHAPE


def test_error_precedence():
    """null pointer, sizes, head dim, alignment, dtype, scale, softcap, grid, workspace: a call with two defects reports the earlier one."""
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    s2 = _fa2_lib.strides2
    chains = [
        [(NULLP, dict(q=None)), (SHAPE, dict(wl=-2)), (HEAD_DIM, dict(D=96)), (ALIGN, dict(sl=p + 2)), (DTYPE, dict(fmt=3)), (SCALE, dict(scale=float("nan"))),
         (SOFTCAP, dict(cap_=-1.0)), (GRID, dict(B=65536)), (NULLP, dict(ns=2, ws=None))],
        [(NULLP, dict(lens=None)), (SHAPE, dict(st=-4)), (HEAD_DIM, dict(D=32)), (ALIGN, dict(k=p + 8)), (DTYPE, dict(kd=p, ds=s2(2, 1))),
         (SCALE, dict(scale=float("inf"))), (SOFTCAP, dict(cap_=float("nan"))), (GRID, dict(B=65536)), (NULLP, dict(ns=2, ws=None))],
        [(SHAPE, dict(Nq=17)), (HEAD_DIM, dict(D=96)), (ALIGN, dict(q=p + 8)), (DTYPE, dict(dtype=7)), (SOFTCAP, dict(cap_=1e-39))],
    ]
    for defects in chains:
        for i, (code, kw) in enumerate(defects):
            assert _call(**kw) == code, kw
            for (_, later) in defects[i + 1:]:
                assert _call(**dict(later, **kw)) == code, (kw, later)
    # inside the size class: the window and the slope stride are refused before the head dim is looked at
    assert _call(D=96, wl=-2) == SHAPE and _call(D=96, st=-1) == SHAPE and _call(D=96, ns=17) == SHAPE


def _args(B=2, Nq=1, H=8, Hkv=2, D=128, Nmax=128, dt=torch.float16):
    return torch.zeros(B, Nq, H, D, dtype=dt), torch.zeros(B, Nmax, Hkv, D, dtype=dt), torch.zeros(B, Nmax, Hkv, D, dtype=dt), torch.ones(B, dtype=torch.int32)


def test_python_argument_checks():
    """Raised before any device work: CPU tensors reach the checks."""
    q, k, v, lens = _args()
    for bad in (-2, -1, (1, 2, 3), (-2, 0), 1.5, True, "3", (3, -2), 2 ** 31):
        with pytest.raises(ValueError, match="window is None"):
            flash_attention_decode(q, k, v, lens, window=bad)
    for bad in (-1.0, float("nan"), float("inf"), "x", True, 1e-39, None):
        with pytest.raises(ValueError, match="softcap must be 0"):
            flash_attention_decode(q, k, v, lens, softcap=bad)
    for bad in (torch.ones(8, dtype=torch.float16), torch.ones(8, dtype=torch.float64), torch.ones(7), torch.ones(3, 8), torch.ones(2, 8, 1), [0.5] * 8, 0.5,
                torch.ones(8, device="meta")):
        with pytest.raises(ValueError, match="alibi_slopes must be a float32 tensor on q's device"):
            flash_attention_decode(q, k, v, lens, alibi_slopes=bad)
    with pytest.raises(ValueError, match="k_descale / v_descale belong to float8_e4m3fn caches"):     # descales with a 16-bit cache, keywords or not
        flash_attention_decode(q, k, v, lens, window=5, k_descale=torch.ones(2, 2))
    # legal values get as far as the device check: a legal `right` is accepted and has no effect
    for kw in (dict(window=5), dict(window=(5, 0)), dict(window=(5, 7)), dict(window=(5, None)), dict(window=(None, 3)), dict(window=0), dict(softcap=30.0),
               dict(alibi_slopes=torch.ones(8)), dict(alibi_slopes=torch.ones(2, 8)), dict(window=(7, -1), softcap=8.0, alibi_slopes=torch.ones(2, 8)[:, :])):
        with pytest.raises(RuntimeError, match="ROCm device"):
            flash_attention_decode(q, k, v, lens, **kw)


def test_plain_call_reaches_the_old_entries(monkeypatch):
    """With none of the three keywords the operator calls fa2_fwd_decode with its old argument list; with one of them the new entry.  (CPU tensors that
    claim a ROCm device and a stand-in for the loaded library, as tests/test_decode_fp8.py does.)"""
    seen = dc.recording_lib(monkeypatch).calls
    q, k, v, lens = _args()
    flash_attention_decode(q, k, v, lens)
    flash_attention_decode(q, k, v, lens, window=None, softcap=0.0, alibi_slopes=None)
    flash_attention_decode(q, k, v, lens, window=(None, 0))
    assert [n for n, _ in seen] == ["fa2_fwd_decode_workspace_bytes", "fa2_fwd_decode"] * 3
    assert all(len(a) == len(_fa2_lib.SYMBOLS[n][1]) for n, a in seen)
    del seen[:]
    sl = torch.ones(8)
    flash_attention_decode(q, k, v, lens, window=(5, 0), softcap=8.0, alibi_slopes=sl)
    assert [n for n, _ in seen] == ["fa2_fwd_decode_window_workspace_bytes", "fa2_fwd_decode_window"]
    assert all(len(a) == len(_fa2_lib.SYMBOLS[n][1]) for n, a in seen)
    a = seen[1][1]
    assert a[:2] == (F16, C16) and a[24:31] == (None, None, None, 5, 8.0, sl.data_ptr(), 0) and seen[0][1][-1] == 5
    del seen[:]
    flash_attention_decode(q, k, v, lens, alibi_slopes=torch.ones(2, 8))
    assert seen[1][0] == "fa2_fwd_decode_window" and seen[1][1][27:29] == (-1, 0.0) and seen[1][1][30] == 8 and seen[0][1][-1] == -1


@pytest.mark.parametrize("shape", wr.SHAPES, ids=wr.IDS)
def test_feature_margin_of_every_parity_case(shape):
    """Not vacuous: float64 WITH the keywords differs from float64 WITHOUT them by at least 5 bars, in O and in the LSE, over the case's batch — a kernel
    that ignored a keyword would fail the GPU file's check by that margin."""
    for name in wr.CASES:
        mo, ml = wr.margins(wr.case_refs(shape, name))
        print(wr.IDS[wr.SHAPES.index(shape)], name, "margins: O %.1f bars, lse %.1f bars" % (mo, ml))
        assert mo >= 5 and ml >= 5, (name, mo, ml)


@pytest.mark.parametrize("shape", wr.EDGE_SHAPES, ids=wr.EDGE_IDS)
def test_feature_margin_of_the_nearly_cache_wide_windows(shape):
    """... and of the GPU file's windows between NMAX - Nq and NMAX - 2, which reach across the cache for row 0 only: the few keys the later rows drop
    are loud, so float64 with the window still differs from float64 without it by at least 5 bars."""
    for name, wl in wr.edge_windows(shape[2]):
        mo, ml = wr.margins(wr.edge_refs(shape, wl))
        print(wr.EDGE_IDS[wr.EDGE_SHAPES.index(shape)], name, "margins: O %.1f bars, lse %.1f bars" % (mo, ml))
        assert mo >= 5 and ml >= 5, (name, mo, ml)
