"""Chunked prefill against a KV cache, without a device: the tile arithmetic the kernel calls (fa2_prefill_tile) against brute force, the plan query,
the C-ABI's error codes and their order on host memory that is never touched, the operator's argument checks, and the exported symbols."""
import ctypes

import pytest
import torch

import decode_calls as dc
from rocwmma_fattn import FlashAttn, _fa2_lib

TILE = 64


def _tiles(length, capacity, page):
    cap = capacity * page if page else capacity
    return [_fa2_lib.prefill_tile(length, capacity, page, t) for t in range(-(-cap // TILE))], cap


LAYOUTS = [(7, 64), (4, 128), (3, 192), (1, 0), (63, 0), (333, 0), (400, 0)]        # (capacity, page_size)


@pytest.mark.parametrize("capacity,page", LAYOUTS)
def test_tiles_partition_the_valid_keys_in_order_and_never_cross_a_page(capacity, page):
    for length in range(0, 401):
        tiles, cap = _tiles(length, capacity, page)
        n = min(length, cap)
        covered = 0
        for t, (slot, row, rows) in enumerate(tiles):
            key0 = t * TILE
            assert rows == max(0, min(TILE, n - key0)), (length, t)
            if rows:
                assert key0 == covered, (length, t)
                covered += rows
            if page:
                assert slot * page + row == key0 and 0 <= slot < capacity and row % TILE == 0 and row + TILE <= page, (length, t, slot, row)
            else:
                assert (slot, row) == (0, key0) and row + rows <= capacity, (length, t, slot, row)
        assert covered == n, (length, covered)


@pytest.mark.parametrize("capacity,page", LAYOUTS)
def test_lengths_outside_the_cache_behave_as_their_clamp(capacity, page):
    cap = capacity * page if page else capacity
    assert _tiles(cap + 1, capacity, page)[0] == _tiles(cap, capacity, page)[0] == _tiles(2 ** 40, capacity, page)[0]
    assert _tiles(-1, capacity, page)[0] == _tiles(0, capacity, page)[0] == _tiles(-2 ** 40, capacity, page)[0]


def test_tile_query_refuses_bad_arguments():
    lib = _fa2_lib.load()
    i = [ctypes.c_int() for _ in range(3)]
    ok = [ctypes.byref(x) for x in i]
    assert lib.fa2_prefill_tile(10, 4, 64, 0, None, ok[1], ok[2]) == -1
    assert lib.fa2_prefill_tile(10, 4, 64, 0, *ok) == 0
    for capacity, page, tile in ((0, 64, 0), (4, 96, 0), (4, -64, 0), (4, 64, 4), (4, 64, -1), (100, 0, 2), (2 ** 25, 64, 0)):
        assert lib.fa2_prefill_tile(10, capacity, page, tile, *ok) == -2, (capacity, page, tile)


def test_plan_reports_the_prefill_kernel_and_follows_option_rows():
    f16 = _fa2_lib.FA2_DTYPE_F16
    before = _fa2_lib.load().fa2_get_option(b"rows")
    try:
        for rows in (128, 256):
            _fa2_lib.set_option("rows", rows)
            for D in (64, 80, 128):
                plan = _fa2_lib.prefill_plan(f16, 2, 4, 2, 300, D, 8, 64)
                assert (plan["kernel"], plan["contract"], plan["rows"], plan["heads_main"]) == (_fa2_lib.FA2_KERNEL_HIP_PREFILL, 0, rows, 8)
            for D in (136, 256, 512):          # above head dim 128: the 128-row shape
                assert _fa2_lib.prefill_plan(f16, 2, 4, 2, 300, D, 717, 0)["rows"] == 128
        _fa2_lib.set_option("rows", 0)
        assert _fa2_lib.prefill_plan(f16, 1, 2, 1, 256, 128, 64, 64)["rows"] == 128             # a small grid
        assert _fa2_lib.prefill_plan(f16, 8, 32, 8, 1024, 128, 64, 64)["rows"] == 256
    finally:
        _fa2_lib.set_option("rows", before)
    lib = _fa2_lib.load()
    plan = _fa2_lib.FwdPlan()
    assert lib.fa2_fwd_prefill_plan(f16, 2, 4, 2, 300, 128, 8, 64, None) == -1
    for bad, rc in ((dict(B=0), -2), (dict(Hkv=3), -2), (dict(max_q=0), -2), (dict(page=96), -2), (dict(capacity=0), -2), (dict(D=12), -3), (dict(D=520), -3),
                    (dict(dtype=7), -5)):
        a = dict(dtype=f16, B=2, H=4, Hkv=2, max_q=300, D=128, capacity=8, page=64)
        a.update(bad)
        assert lib.fa2_fwd_prefill_plan(a["dtype"], a["B"], a["H"], a["Hkv"], a["max_q"], a["D"], a["capacity"], a["page"], ctypes.byref(plan)) == rc, bad


# ---------------------------------------------------------------------------------------------------------------- error codes on host memory
_HOST = ctypes.create_string_buffer(4096 + 16)
HOST = (ctypes.addressof(_HOST) + 15) & ~15          # 16-byte aligned host memory that no call here ever touches
NULL, BAD_SHAPE, HEAD_DIM, ALIGN, DTYPE, SCALE, GRID, SOFTCAP = -1, -2, -3, -4, -5, -6, -7, -10


def _call(**kw):
    s2, s3 = _fa2_lib.strides2, _fa2_lib.strides3
    a = dict(dtype=_fa2_lib.FA2_DTYPE_F16, fmt=_fa2_lib.FA2_CACHE_16BIT, q=HOST, k=HOST, v=HOST, o=HOST, lse=HOST, cu=HOST, lens=HOST, bt=HOST, B=2, H=4, Hkv=2,
             max_q=300, D=128, cap=8, page=64, pages=20, qs=s2(128, 512), ks=s3(64 * 256, 128, 256), vs=s3(64 * 256, 128, 256), os=s2(128, 512),
             lss=1024, bts=8, scale=0.125, wl=-1, cap_=0.0, sl=None, st=0, stream=None)
    return dc.host_call("prefill", a, **kw)


BAD = {      # one defect per class, in the order the classes are checked
    NULL: [dict(q=None), dict(k=None), dict(o=None), dict(lse=None), dict(cu=None), dict(lens=None), dict(bt=None), dict(qs=None), dict(ks=None), dict(os=None)],
    BAD_SHAPE: [dict(B=0), dict(H=0), dict(Hkv=3), dict(max_q=0), dict(page=96), dict(page=-64), dict(cap=0), dict(pages=0), dict(wl=-2),
                dict(lss=-1), dict(st=-1), dict(cap=2 ** 25), dict(ks=_fa2_lib.strides3(8, 8, 2 ** 24))],
    HEAD_DIM: [dict(D=12), dict(D=520)],
    ALIGN: [dict(q=HOST + 8), dict(k=HOST + 2), dict(o=HOST + 4), dict(lse=HOST + 2), dict(cu=HOST + 2), dict(lens=HOST + 1), dict(bt=HOST + 2),
            dict(sl=HOST + 2), dict(qs=_fa2_lib.strides2(4, 512)), dict(ks=_fa2_lib.strides3(64 * 256, 128, 4)), dict(os=_fa2_lib.strides2(128, 0)), dict(bts=-8)],
    DTYPE: [dict(dtype=5), dict(fmt=_fa2_lib.FA2_CACHE_E4M3), dict(fmt=9)],
    SCALE: [dict(scale=float("nan")), dict(scale=float("inf"))],
    SOFTCAP: [dict(cap_=-1.0), dict(cap_=float("nan"))],
    GRID: [dict(B=2 ** 15, H=2 ** 15, Hkv=2 ** 15, max_q=2 ** 20)],
}
CLASSES = (NULL, BAD_SHAPE, HEAD_DIM, ALIGN, DTYPE, SCALE, SOFTCAP, GRID)


def test_every_error_code_is_returned():
    for rc, cases in BAD.items():
        for kw in cases:
            assert _call(**kw) == rc, kw
    # the contiguous layout takes no block table and no pool size
    assert _call(bt=None, page=0, cap=717, pages=0, q=None) == NULL
    assert _call(bt=None, page=0, cap=717, pages=0, D=12) == HEAD_DIM


def test_error_classes_are_checked_in_decode_order():
    for i, first in enumerate(CLASSES):
        for later in CLASSES[i + 1:]:
            kw = dict(BAD[later][0])
            kw.update(BAD[first][0])
            if set(BAD[later][0]) & set(BAD[first][0]):
                continue
            assert _call(**kw) == first, (first, later, kw)


# ---------------------------------------------------------------------------------------------------------------- the operator
def _op_args(dtype=torch.float16, page=64):
    q = torch.zeros(10, 4, 64, dtype=dtype)
    kc = torch.zeros(6, page, 2, 64, dtype=dtype)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    lens = torch.tensor([70, 100], dtype=torch.int32)
    bt = torch.zeros(2, 3, dtype=torch.int32)
    return q, kc, kc.clone(), cu, lens, bt


def test_operator_refuses_before_any_device_work():
    prefill = FlashAttn.flash_attention_prefill
    q, kc, vc, cu, lens, bt = _op_args()
    e4m3 = getattr(torch, "float8_e4m3fn", None)
    if e4m3 is not None:
        with pytest.raises(ValueError, match="flash_attention_prefill.*16-bit caches only"):
            prefill(q, kc.to(e4m3), vc.to(e4m3), cu, lens, bt)
    for kw in (dict(k_descale=torch.ones(2, 2)), dict(v_descale=torch.ones(2, 2))):
        with pytest.raises(ValueError, match="flash_attention_prefill.*16-bit caches only"):
            prefill(q, kc, vc, cu, lens, bt, **kw)
    with pytest.raises(ValueError, match="inference only"):
        prefill(q.clone().requires_grad_(), kc, vc, cu, lens, bt)
    with torch.no_grad(), pytest.raises(ValueError, match="multiple of 64"):        # (grad mode off: requires_grad is not the reason)
        q96 = _op_args(page=96)
        prefill(q96[0].clone().requires_grad_(), *q96[1:])
    with pytest.raises(ValueError, match="block_table must be int32"):
        prefill(q, kc, vc, cu, lens, bt.long())
    with pytest.raises(ValueError, match=r"cache_seqlens must be .* \[B\] = \[2\]"):
        prefill(q, kc, vc, cu, torch.tensor([70, 100, 3], dtype=torch.int32), bt)
    with pytest.raises(ValueError, match="cu_seqlens_q"):
        prefill(q, kc, vc, cu.long(), lens, bt)
    with pytest.raises(ValueError, match="contiguous cache is"):
        prefill(q, kc, vc, cu, lens)                     # six "sequences" in the cache, two in cu_seqlens_q
    with pytest.raises(ValueError, match="fp16 or bf16"):
        prefill(q.float(), kc.float(), vc.float(), cu, lens, bt)
    with pytest.raises(ValueError, match="max_seqlen_q"):
        prefill(q, kc, vc, cu, lens, bt, max_seqlen_q=-1)


def test_symbols_are_exported_and_the_operator_is_public():
    lib = _fa2_lib.load()
    for name in ("fa2_fwd_prefill", "fa2_fwd_prefill_plan", "fa2_prefill_tile"):
        assert name in _fa2_lib.SYMBOLS and getattr(lib, name) is not None
    assert "flash_attention_prefill" in FlashAttn.__all__ and callable(FlashAttn.flash_attention_prefill)
    assert _fa2_lib.FA2_KERNEL_HIP_PREFILL == 8
