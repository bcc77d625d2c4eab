"""CPU tests of KV-cache decode attention (include/fa2_gfx950.h: fa2_fwd_decode and its queries): the part-range arithmetic the kernel and the host share
(fa2_decode_part_range, csrc/fa2_decode.hip.h) exhaustively against its definition, the plan and the workspace size, every validation code and the
order they are checked in, and the argument checks of flash_attention_decode.  Nothing here touches a device: every rejected call returns before the
launch, and the Python checks run before any device work."""
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
DECODE_SYMBOLS = ("fa2_fwd_decode", "fa2_fwd_decode_plan", "fa2_fwd_decode_workspace_bytes", "fa2_decode_part_range")
OK, NULLP, SHAPE, HEAD_DIM, ALIGN, DTYPE, SCALE, GRID = 0, -1, -2, -3, -4, -5, -6, -7
F16, BF16 = _fa2_lib.FA2_DTYPE_F16, _fa2_lib.FA2_DTYPE_BF16


def test_symbols_are_declared_exported_and_bound():
    lib = _fa2_lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in DECODE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _fa2_lib.SYMBOLS, name
        assert getattr(lib, name).argtypes == _fa2_lib.SYMBOLS[name][1]
    assert re.search(r"FA2_KERNEL_HIP_DECODE\s*=\s*%d\b" % _fa2_lib.FA2_KERNEL_HIP_DECODE, text)


def _kernel_tile():
    return _fa2_lib.decode_plan(F16, 1, 8, 8, 1, 128, 1024).key_tile


@pytest.mark.parametrize("tile", sorted({64, 32}))
def test_part_range_exhaustive(tile):
    """len 0 .. 300, nsplit 1 .. 16: the parts are disjoint, ordered, each at most per = ceil(tiles / nsplit) long, and cover exactly ceil(len / tile) tiles."""
    assert 64 % _kernel_tile() == 0 and _kernel_tile() in (64, 32), "the kernel's key tile divides 64 and is one of the tiles swept here"
    for length in range(0, 301):
        tiles = -(-length // tile)
        for nsplit in range(1, 17):
            per = -(-tiles // nsplit)
            nxt = 0
            for part in range(nsplit):
                first, n = _fa2_lib.decode_part_range(length, 4096, 1, tile, nsplit, part)
                assert 0 <= n <= per
                if n:
                    assert first == nxt == part * per, (length, nsplit, part, first, n)
                    nxt = first + n
                else:
                    assert part * per >= tiles, (length, nsplit, part)
            assert nxt == tiles, (length, nsplit)


def test_part_range_clamps_the_length():
    pr = _fa2_lib.decode_part_range
    for tile in (32, 64):
        for nsplit in (1, 3, 16):
            for part in range(nsplit):
                assert pr(10 ** 9, 200, 1, tile, nsplit, part) == pr(200, 200, 1, tile, nsplit, part)       # above the capacity
                assert pr(2 ** 40, 200, 3, tile, nsplit, part) == pr(200, 200, 3, tile, nsplit, part)
                assert pr(-5, 200, 1, tile, nsplit, part) == (0, 0) == pr(-2 ** 40, 200, 1, tile, nsplit, part)    # negative
                assert pr(300, 0, 1, tile, nsplit, part) == (0, 0)
    # a clamped sweep never passes the capacity's last tile
    for cap in (1, 63, 64, 65, 1000):
        first, n = pr(2 ** 31 - 1, cap, 1, 32, 1, 0)
        assert (first + n) * 32 < cap + 32


def test_part_range_argument_codes():
    lib = _fa2_lib.load()
    a, b = ctypes.c_int(), ctypes.c_int()
    ra, rb = ctypes.byref(a), ctypes.byref(b)
    assert lib.fa2_decode_part_range(100, 200, 1, 32, 2, 0, None, rb) == NULLP
    assert lib.fa2_decode_part_range(100, 200, 1, 32, 2, 0, ra, None) == NULLP
    for args in ((100, -1, 1, 32, 2, 0), (100, 200, 0, 32, 2, 0), (100, 200, 1, 0, 2, 0), (100, 200, 1, 32, 0, 0), (100, 200, 1, 32, 17, 0),
                 (100, 200, 1, 32, 2, 2), (100, 200, 1, 32, 2, -1)):
        assert lib.fa2_decode_part_range(*args, ra, rb) == SHAPE, args
    assert lib.fa2_decode_part_range(100, 200, 1, 32, 16, 15, ra, rb) == OK


def _ws(dt, B, H, Hkv, Nq, D, cap, page=0, ns=0):
    return _fa2_lib.load().fa2_fwd_decode_workspace_bytes(dt, B, H, Hkv, Nq, D, cap, page, ns)


def test_plan_is_deterministic_and_honours_a_forced_split():
    shapes = [(1, 32, 8, 1, 128, 8192, 0), (32, 32, 8, 1, 128, 4096, 0), (4, 8, 8, 1, 64, 16384, 0), (8, 32, 8, 4, 128, 8192, 0), (1, 32, 1, 1, 128, 32, 256),
              (3, 12, 4, 3, 64, 100, 0)]
    for (B, H, Hkv, Nq, D, cap, page) in shapes:
        for dt in (F16, BF16):
            a = _fa2_lib.decode_plan(dt, B, H, Hkv, Nq, D, cap, page).as_dict()
            assert a == _fa2_lib.decode_plan(dt, B, H, Hkv, Nq, D, cap, page).as_dict()
            rows = Nq * (H // Hkv)
            assert a["kernel"] == _fa2_lib.FA2_KERNEL_HIP_DECODE and a["key_tile"] == _kernel_tile()
            assert a["row_tiles"] == {1: 1, 2: 2, 3: 4, 4: 4}[-(-rows // 16)]      # row tiles of 16; three run the four-tile kernel
            assert 1 <= a["nsplit"] <= 16
            for ns in range(1, 17):
                f = _fa2_lib.decode_plan(dt, B, H, Hkv, Nq, D, cap, page, ns).as_dict()
                assert f["nsplit"] == ns and f["row_tiles"] == a["row_tiles"]
                assert _ws(dt, B, H, Hkv, Nq, D, cap, page, ns) == (0 if ns == 1 else B * Hkv * ns * rows * (D + 1) * 4)
            assert _ws(dt, B, H, Hkv, Nq, D, cap, page) == (0 if a["nsplit"] == 1 else B * Hkv * a["nsplit"] * rows * (D + 1) * 4)


def test_plan_does_not_split_a_grid_that_covers_the_chip():
    """B * Hkv * row_tiles >= the CU count (256 on an MI355X, and the library's answer without a device): split 1, no workspace."""
    for (B, H, Hkv, Nq) in ((32, 32, 8, 1), (256, 8, 1, 1), (64, 16, 1, 4), (1024, 8, 8, 1)):
        plan = _fa2_lib.decode_plan(F16, B, H, Hkv, Nq, 128, 8192)
        assert B * Hkv * plan.row_tiles >= 256
        assert plan.nsplit == 1, plan.as_dict()
        assert _ws(F16, B, H, Hkv, Nq, 128, 8192) == 0
    # ... and an underfilled one is split, but never into parts shorter than 8 key tiles of the capacity
    assert _fa2_lib.decode_plan(F16, 1, 32, 8, 1, 128, 8192).nsplit > 1
    tile = _kernel_tile()
    for cap in (1, tile, 8 * tile, 16 * tile - 1, 16 * tile, 40 * tile):
        assert _fa2_lib.decode_plan(F16, 1, 8, 8, 1, 128, cap).nsplit == max(1, min(16, -(-cap // tile) // 8)), cap


P = dc.HOST                                  # 16-byte aligned host memory that no call here ever touches
DEFAULTS = dict(dtype=F16, q=P, k=P, v=P, o=P, lse=P, lens=P, bt=None, B=2, H=8, Hkv=2, Nq=1, D=128, cap=256, page=0, pages=0,
                qs=_fa2_lib.strides3(1024, 128, 1024), ks=_fa2_lib.strides3(256 * 256, 128, 256), vs=_fa2_lib.strides3(256 * 256, 128, 256),
                os=_fa2_lib.strides3(1024, 128, 1024), ls=_fa2_lib.strides2(8, 1), bts=0, scale=0.1, ns=1, ws=None, wsb=0)


def _call(**kw):
    """fa2_fwd_decode on host memory that is never touched: every call here is refused before the launch."""
    return dc.host_call("plain", DEFAULTS, **kw)


def test_every_error_code():
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    for name in ("q", "k", "v", "o", "lse", "lens", "qs", "ks", "vs", "os", "ls"):
        assert _call(**{name: None}) == NULLP, name
    assert _call(page=64, pages=4, bt=None) == NULLP                     # a paged call needs its block table
    for kw in (dict(B=0), dict(H=0), dict(Hkv=0), dict(Nq=0), dict(D=0), dict(cap=0), dict(H=8, Hkv=3), dict(H=2, Hkv=4), dict(Nq=17), dict(H=128, Hkv=1),
               dict(page=48, pages=4, bt=p), dict(page=-64, pages=4, bt=p), dict(page=32, pages=4, bt=p), dict(ns=17), dict(ns=-1),
               dict(page=64, pages=0, bt=p), dict(ls=_fa2_lib.strides2(-8, 1))):
        assert _call(**kw) == SHAPE, kw
    for D in (96, 32, 256, 8, 129):
        assert _call(D=D) == HEAD_DIM, D
    for kw in (dict(q=p + 8), dict(k=p + 2), dict(v=p + 8), dict(o=p + 4), dict(lse=p + 2), dict(lens=p + 1), dict(page=64, pages=4, bt=p + 2),
               dict(qs=_fa2_lib.strides3(1024, 132, 1024)), dict(ks=_fa2_lib.strides3(65536, 128, 0)), dict(vs=_fa2_lib.strides3(65536, 128, 260)),
               dict(os=_fa2_lib.strides3(-1024, 128, 1024)), dict(page=64, pages=4, bt=p, bts=-4)):
        assert _call(**kw) == ALIGN, kw
    assert _call(dtype=2) == DTYPE and _call(dtype=-1) == DTYPE
    assert _call(scale=float("nan")) == SCALE and _call(scale=float("inf")) == SCALE
    assert _call(B=65536) == GRID
    # the workspace of a split call: checked last
    need = _ws(F16, 2, 8, 2, 1, 128, 256, 0, 2)
    assert need == 2 * 2 * 2 * 4 * 129 * 4
    assert _call(ns=2, ws=None) == NULLP
    assert _call(ns=2, ws=p + 4, wsb=need) == ALIGN
    assert _call(ns=2, ws=p, wsb=need - 1) == SHAPE


def test_error_precedence():
    """null pointer, shape, head dim, alignment, dtype, scale, grid, workspace: a call with two defects reports the earlier one."""
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    defects = [(NULLP, dict(q=None)), (SHAPE, dict(Nq=17)), (HEAD_DIM, dict(D=96)), (ALIGN, dict(k=p + 8)), (DTYPE, dict(dtype=7)),
               (SCALE, dict(scale=float("nan"))), (GRID, dict(B=65536)), (NULLP, dict(ns=2, ws=None))]
    for i, (code, kw) in enumerate(defects):
        assert _call(**kw) == code
        for (_, later) in defects[i + 1:]:
            assert _call(**dict(later, **kw)) == code, (kw, later)
    # inside the shape class: the row count and the split are refused before the head dim is looked at
    assert _call(D=96, ns=17) == SHAPE and _call(D=96, page=48, pages=4, bt=p) == SHAPE
    # the plan and size queries answer with the same codes / with 0
    plan = _fa2_lib.DecodePlan()
    lib = _fa2_lib.load()
    assert lib.fa2_fwd_decode_plan(F16, 2, 8, 2, 1, 128, 256, 0, 0, None) == NULLP
    assert lib.fa2_fwd_decode_plan(F16, 2, 8, 2, 17, 96, 256, 0, 0, ctypes.byref(plan)) == SHAPE
    assert lib.fa2_fwd_decode_plan(7, 2, 8, 2, 1, 96, 256, 0, 0, ctypes.byref(plan)) == HEAD_DIM
    assert lib.fa2_fwd_decode_plan(7, 2, 8, 2, 1, 128, 256, 0, 0, ctypes.byref(plan)) == DTYPE
    assert _ws(F16, 2, 8, 2, 17, 128, 256, 0, 4) == 0 and _ws(7, 2, 8, 2, 1, 128, 256, 0, 4) == 0


def _args(B=2, Nq=1, H=8, Hkv=2, D=128, Nmax=128, dt=torch.float16):
    return torch.zeros(B, Nq, H, D, dtype=dt), torch.zeros(B, Nmax, Hkv, D, dtype=dt), torch.zeros(B, Nmax, Hkv, D, dtype=dt), torch.ones(B, dtype=torch.int32)


def test_python_argument_checks():
    """Raised before any device work: CPU tensors reach the checks."""
    q, k, v, lens = _args()
    with pytest.raises(ValueError, match="inference only"):
        flash_attention_decode(q.clone().requires_grad_(True), k, v, lens)
    with pytest.raises(ValueError, match="inference only"):
        flash_attention_decode(q, k.clone().requires_grad_(True), v, lens)
    with pytest.raises(ValueError, match="inference only"):
        flash_attention_decode(q, k, v.clone().requires_grad_(True), lens)
    with torch.no_grad():                                                # grad mode off: the call gets as far as the device check
        with pytest.raises(RuntimeError, match="ROCm device"):
            flash_attention_decode(q.clone().requires_grad_(True), k, v, lens)
    with pytest.raises(ValueError, match="flash_attention_varlen"):      # H % Hkv != 0
        flash_attention_decode(*_args(H=8, Hkv=3))
    with pytest.raises(ValueError, match="<= 64 query rows.*flash_attention_varlen"):
        flash_attention_decode(*_args(Nq=9, H=16, Hkv=2))
    flash_err = pytest.raises(ValueError, match="head dims 64 and 128.*flash_attention_varlen")
    with flash_err:
        flash_attention_decode(*_args(D=96))
    with pytest.raises(ValueError, match="int32"):
        flash_attention_decode(q, k, v, lens.long())
    with pytest.raises(ValueError, match="cache_seqlens"):
        flash_attention_decode(q, k, v, torch.ones(3, dtype=torch.int32))
    bt = torch.zeros(2, 4, dtype=torch.int32)
    pool = torch.zeros(8, 48, 2, 128, dtype=torch.float16)
    with pytest.raises(ValueError, match="multiple of 64"):              # page_size = 48
        flash_attention_decode(q, pool, pool, lens, block_table=bt)
    # a block table whose batch dimension contradicts q's, with a cache shaped like a contiguous one
    with pytest.raises(ValueError, match="block_table"):
        flash_attention_decode(q, k, v, lens, block_table=torch.zeros(3, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="block_table"):
        flash_attention_decode(q, k, v, lens, block_table=bt.long())
    # ... and a contiguous cache whose batch dimension contradicts q's, without one
    q3 = torch.zeros(3, 1, 8, 128, dtype=torch.float16)
    with pytest.raises(ValueError, match="block_table"):
        flash_attention_decode(q3, k, v, torch.ones(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="num_splits"):
        flash_attention_decode(q, k, v, lens, num_splits=17)
    with pytest.raises(ValueError, match="one dtype"):
        flash_attention_decode(q, k.bfloat16(), v.bfloat16(), lens)
    with pytest.raises(RuntimeError, match="ROCm device"):               # everything else in order: only the device is missing
        flash_attention_decode(q, k, v, lens)
