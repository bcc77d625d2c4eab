"""Packed, variable-length attention, the parts that need no GPU: the symbols of the C-ABI, their validation codes, the per-sequence range arithmetic
(fa2_varlen_tile_range / fa2_varlen_row_range, negative bottom-right offsets included) against brute force, the plan query, and the operator's
argument handling."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from rocwmma_fattn import FlashAttn, _fa2_lib

HEADER = os.path.join(ROOT, "include", "fa2_gfx950.h")
VARLEN_SYMBOLS = ("fa2_fwd_varlen", "fa2_bwd_varlen", "fa2_fwd_varlen_plan", "fa2_varlen_tile_range", "fa2_varlen_row_range")
CAUSAL, EXACT, BOTTOM_RIGHT = _fa2_lib.FA2_FLAG_CAUSAL, _fa2_lib.FA2_FLAG_EXACT_SCALE, _fa2_lib.FA2_FLAG_BOTTOM_RIGHT


def _codes():
    text = open(HEADER).read()
    return {m[0]: int(m[1]) for m in re.findall(r"#define\s+(FA2_\w+)\s+(-?\d+)", text)}


def test_varlen_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _fa2_lib.load()
    for name in VARLEN_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _fa2_lib.SYMBOLS
        assert getattr(lib, name) is not None
    assert re.search(r"enum\s*\{\s*FA2_KERNEL_HIP_VARLEN\s*=\s*%d\s*\}" % _fa2_lib.FA2_KERNEL_HIP_VARLEN, text)
    assert _fa2_lib.FA2_KERNEL_HIP_VARLEN == 6
    assert _codes()["FA2_FLAG_BOTTOM_RIGHT"] == BOTTOM_RIGHT == 4
    assert hasattr(FlashAttn, "flash_attention_varlen") and hasattr(FlashAttn.flash_attn_wmma, "forward_varlen")
    assert hasattr(FlashAttn.flash_attn_wmma, "backward_varlen") and hasattr(FlashAttn, "_VarlenAttentionFunction")


def test_validation_codes_of_the_plan_and_of_both_launching_entry_points():
    """Every bad argument is refused by the plan query and by both launching entry points — the latter with null tensors, so nothing touches a device."""
    lib = _fa2_lib.load()
    c = _codes()
    plan = _fa2_lib.FwdPlan()
    good = _fa2_lib.strides2(64, 8 * 64)

    def calls(dtype=0, B=3, H=8, Hkv=2, mq=256, mk=256, D=64, qs=good, ks=good, scale=0.125, flags=0, left=64, right=0, out=plan):
        """(plan, forward, backward) return codes; the backward is the multi-head one (no Hkv)."""
        po = ctypes.byref(out) if out is not None else None
        return (lib.fa2_fwd_varlen_plan(dtype, B, H, Hkv, mq, mk, D, qs, ks, scale, flags, left, right, po),
                lib.fa2_fwd_varlen(dtype, None, None, None, None, None, B, H, Hkv, mq, mk, D, None, None, qs, ks, ks, qs, 0, scale, flags, left, right, None),
                lib.fa2_bwd_varlen(dtype, *([None] * 10), B, H, mq, mk, D, None, None, qs, ks, ks, qs, qs, qs, ks, ks, 0, scale, flags, left, right, None))

    # good arguments: the plan answers; the launching entry points get as far as their null tensors
    assert calls() == (0, c["FA2_ERR_NULL_POINTER"], c["FA2_ERR_NULL_POINTER"])
    shape = c["FA2_ERR_BAD_SHAPE"]
    for bad in (dict(B=0), dict(H=0), dict(D=0), dict(mq=0), dict(mk=0), dict(mq=-5), dict(left=-2), dict(right=-2), dict(left=2 ** 31 - 1),
                dict(right=2 ** 31 - 1), dict(flags=8), dict(flags=16 | CAUSAL), dict(mq=2 ** 31 - 1000)):
        assert calls(**bad) == (shape, shape, shape), bad
    for bad in (dict(Hkv=3), dict(Hkv=9), dict(Hkv=0)):            # (the backward has no Hkv argument)
        assert calls(**bad)[:2] == (shape, shape), bad
    assert calls(D=520) == (c["FA2_ERR_HEAD_DIM"],) * 3 and calls(D=12) == (c["FA2_ERR_HEAD_DIM"],) * 3
    assert calls(dtype=2) == (c["FA2_ERR_DTYPE"],) * 3
    assert calls(scale=float("nan")) == (c["FA2_ERR_SCALE"],) * 3
    assert calls(qs=_fa2_lib.strides2(64, 8 * 64 + 4)) == (c["FA2_ERR_ALIGNMENT"],) * 3
    assert calls(ks=_fa2_lib.strides2(12, 8 * 64))[:2] == (c["FA2_ERR_ALIGNMENT"],) * 2
    # a stated maximum whose span (max_seqlen * row pitch) reaches 2 GiB
    assert calls(mk=2 ** 21, ks=_fa2_lib.strides2(64, 512))[:2] == (shape, shape)
    assert calls(mk=2 ** 21 - 128, ks=_fa2_lib.strides2(64, 512))[0] == 0
    assert calls(mq=2 ** 21, mk=2 ** 21)[2] == shape
    # grids beyond 2^31 - 1
    assert calls(B=2 ** 20, H=64, Hkv=64, mq=2 ** 16, mk=64) == (c["FA2_ERR_GRID"],) * 3
    assert calls(out=None)[0] == c["FA2_ERR_NULL_POINTER"]
    # every documented flag combination is accepted by the varlen plan; bit 2 stays refused by the windowed plan
    for flags in range(8):
        assert calls(flags=flags)[0] == 0, flags
    assert lib.fa2_fwd_window_plan(0, 1, 8, 2, 256, 256, 64, None, None, 0.125, BOTTOM_RIGHT, 64, 0, 0, 0, ctypes.byref(plan)) == shape
    assert calls(qs=None, ks=None)[0] == 0                       # NULL strides in the plan query: contiguous tensors
    s2 = _fa2_lib.strides2(64, 512)
    assert lib.fa2_fwd_varlen(0, None, None, None, None, None, 3, 8, 2, 256, 256, 64, None, None, None, s2, s2, s2, 0, 0.125, 0, -1, -1, None) == c["FA2_ERR_NULL_POINTER"]
    # the range queries
    first, n = ctypes.c_int(), ctypes.c_int()
    f, nn = ctypes.byref(first), ctypes.byref(n)
    for fn in (lib.fa2_varlen_tile_range, lib.fa2_varlen_row_range):
        assert fn(64, 32, 8, 0, BOTTOM_RIGHT, 0, 32, 64, f, nn) == 0
        assert fn(0, 32, -1, -1, 0, 0, 32, 64, f, nn) == 0 and n.value == 0          # zero-length sides are legal and empty
        assert fn(64, 0, -1, -1, CAUSAL | BOTTOM_RIGHT, 0, 32, 64, f, nn) == 0 and n.value == 0
        assert fn(64, 32, 8, 0, 0, 0, 32, 64, None, nn) == c["FA2_ERR_NULL_POINTER"]
        assert fn(64, 32, 8, 0, 0, 0, 32, 64, f, None) == c["FA2_ERR_NULL_POINTER"]
        for args in ((-1, 64, 8, 0, 0, 0, 32, 64), (64, -1, 8, 0, 0, 0, 32, 64), (64, 64, -2, 0, 0, 0, 32, 64), (64, 64, 8, -3, 0, 0, 32, 64),
                     (64, 64, 8, 0, 8, 0, 32, 64), (64, 64, 8, 0, 0, -1, 32, 64), (64, 64, 8, 0, 0, 0, 0, 64), (64, 64, 8, 0, 0, 0, 32, 0),
                     (2 ** 31 - 1, 1, 8, 0, BOTTOM_RIGHT, 0, 32, 64)):
            assert fn(*args, f, nn) == shape, args
    # the windowed queries keep refusing a negative offset
    assert lib.fa2_window_tile_range(64, 32, 8, 0, -32, 0, 0, 32, 64, f, nn) == shape
    assert lib.fa2_window_row_range(64, 32, 8, 0, -32, 0, 0, 32, 64, f, nn) == shape


def _band(Nq, Nkv, left, right, off):
    """Brute force: the boolean [Nq, Nkv] visibility matrix of the contract in include/fa2_gfx950.h (right already carries the causal flag)."""
    pos = np.arange(Nq)[:, None] + off
    j = np.arange(Nkv)[None, :]
    keep = np.ones((Nq, Nkv), dtype=bool)
    if left >= 0:
        keep &= j >= pos - left
    if right >= 0:
        keep &= j <= pos + right
    return keep


LENGTHS = (1, 63, 64, 65, 129, 640, 1000)          # (the grid of tests/test_window.py)
WINDOWS = (-1, 0, 1, 63, 64, 100, 4096)
TILE = 64


@pytest.mark.parametrize("Nq", LENGTHS)
def test_tile_and_row_ranges_against_brute_force(Nq):
    """Every (Nq_s, Nkv_s, left, right, causal, bottom-right, block size) of the grid — every pair with Nkv_s < Nq_s included under bottom-right, where
    the offset is negative and the dead rows of a block sit at its top: the range holds every tile with a visible pair, its first and last tile each
    hold one, an empty band gives ntiles = 0 and nothing else does."""
    lib = _fa2_lib.load()
    first, n = ctypes.c_int(), ctypes.c_int()
    f, nn = ctypes.byref(first), ctypes.byref(n)
    checked = negative = 0
    for Nkv in LENGTHS:
        for left, right, causal, br in itertools.product(WINDOWS, WINDOWS, (0, 1), (0, 1)):
            if causal and right != WINDOWS[0]:
                continue                               # (the flag overrides window_right: one representative is enough)
            off = Nkv - Nq if br else 0
            flags = (CAUSAL if causal else 0) | (BOTTOM_RIGHT if br else 0)
            keep = _band(Nq, Nkv, left, 0 if causal else right, off)
            nkt, nqt = (Nkv + TILE - 1) // TILE, (Nq + TILE - 1) // TILE
            kv_any = np.zeros((Nq, nkt), dtype=bool)
            for t in range(nkt):
                kv_any[:, t] = keep[:, t * TILE:(t + 1) * TILE].any(1)
            q_any = np.zeros((nqt, Nkv), dtype=bool)
            for t in range(nqt):
                q_any[t] = keep[t * TILE:(t + 1) * TILE].any(0)
            for rows in (32, 128, 256):
                for fn, live, total in ((lib.fa2_varlen_tile_range, kv_any, Nq), (lib.fa2_varlen_row_range, q_any.T, Nkv)):
                    for row0 in range(0, total, rows):
                        assert fn(Nq, Nkv, left, right, flags, row0, rows, TILE, f, nn) == 0
                        want = np.nonzero(live[row0:row0 + rows].any(0))[0]
                        case = (fn is lib.fa2_varlen_row_range, Nq, Nkv, left, right, flags, row0, rows, first.value, n.value)
                        if want.size == 0:
                            assert n.value == 0, case
                        else:
                            assert (first.value, first.value + n.value - 1) == (int(want[0]), int(want[-1])), case
                        checked += 1
                        negative += off < 0
    assert checked > 1000 and (negative > 100 or Nq == LENGTHS[0])


def test_ranges_of_empty_sequences_and_agreement_with_the_windowed_queries():
    first, n = ctypes.c_int(), ctypes.c_int()
    for Nq, Nkv in ((0, 0), (0, 100), (100, 0)):
        for flags, rows in itertools.product(range(8), (32, 128)):
            assert _fa2_lib.varlen_tile_range(Nq, Nkv, -1, -1, flags, 0, rows) == (0, 0)
            assert _fa2_lib.varlen_tile_range(Nq, Nkv, 5, 7, flags, 0, rows, transpose=True) == (0, 0)
    # offsets >= 0: the same implementation answers both families of queries
    for Nq, Nkv, left, right, causal in ((100, 300, 17, 5, 0), (64, 64, -1, -1, 1), (129, 1000, 64, -1, 1)):
        for row0 in range(0, Nq, 32):
            want = _fa2_lib.window_tile_range(Nq, Nkv, left, right, Nkv - Nq, causal, row0, 32)
            assert _fa2_lib.varlen_tile_range(Nq, Nkv, left, right, BOTTOM_RIGHT | (CAUSAL if causal else 0), row0, 32) == want
        for key0 in range(0, Nkv, 128):
            want = _fa2_lib.window_tile_range(Nq, Nkv, left, right, 0, causal, key0, 128, transpose=True)
            assert _fa2_lib.varlen_tile_range(Nq, Nkv, left, right, CAUSAL if causal else 0, key0, 128, transpose=True) == want


@pytest.mark.parametrize("D", [64, 128, 256, 512])
def test_plan_names_the_varlen_kernel(D):
    for dt in (torch.float16, torch.bfloat16):
        for B, H, Hkv, mq, mk, flags, left, right in ((8, 16, 16, 8192, 8192, 0, -1, -1), (8, 16, 4, 8192, 8192, CAUSAL, -1, -1),
                                                      (16, 32, 8, 4096, 4096, CAUSAL | BOTTOM_RIGHT, 127, -1), (3, 4, 1, 1, 1000, EXACT, 5, 9),
                                                      (1, 2, 2, 100, 1, CAUSAL | BOTTOM_RIGHT | EXACT, -1, -1)):
            q = torch.empty((10, H, D), dtype=dt, device="meta")
            k = torch.empty((10, Hkv, D), dtype=dt, device="meta")
            pl = _fa2_lib.varlen_plan(q, k, mq, mk, B, flags, left, right)
            assert pl.kernel == _fa2_lib.FA2_KERNEL_HIP_VARLEN and pl.contract == 0, pl.as_dict()
            assert pl.rows in (128, 256) and (D <= 256 or pl.rows == 128) and pl.heads_main == B * H
            assert pl.kernel_tail == 0 and pl.nsplit == 0 and pl.split_items == 0
        q, k = torch.empty((10, 16, D), dtype=dt, device="meta"), torch.empty((10, 4, D), dtype=dt, device="meta")
        for rows in (128, 256):
            with _fa2_lib.options(rows=rows):
                assert _fa2_lib.varlen_plan(q, k, 4096, 4096, 8, CAUSAL).rows == (128 if D > 256 else rows)


def test_plan_of_head_dims_below_the_padded_ones():
    for D, dt in itertools.product((8, 40, 80, 192, 264, 504), (torch.float16, torch.bfloat16)):
        q, k = torch.empty((10, 8, D), dtype=dt, device="meta"), torch.empty((10, 2, D), dtype=dt, device="meta")
        pl = _fa2_lib.varlen_plan(q, k, 1000, 1000, 4)
        assert pl.kernel == _fa2_lib.FA2_KERNEL_HIP_VARLEN and (D <= 256 or pl.rows == 128)


def test_operator_argument_handling_on_cpu_tensors():
    q = torch.zeros((48, 4, 64), dtype=torch.float16)
    k = torch.zeros((48, 2, 64), dtype=torch.float16)
    cu = torch.tensor([0, 16, 48], dtype=torch.int32)
    fa = FlashAttn.flash_attention_varlen
    bad = (
        (dict(q=q[0]), "3-D"), (dict(k=k.unsqueeze(0), v=k.unsqueeze(0)), "3-D"),
        (dict(cu_seqlens_k=cu[:2]), "same length"), (dict(cu_seqlens_q=cu[:1], cu_seqlens_k=cu[:1]), "same length"),
        (dict(cu_seqlens_q=cu.long()), "int32"), (dict(cu_seqlens_k=cu.float()), "int32"),
        (dict(cu_seqlens_q=cu.to("meta")), "device of q"), (dict(cu_seqlens_k=cu.to("meta")), "device of q"),
        (dict(cu_seqlens_q=[0, 16, 48]), "1-D int32"),
        (dict(k=torch.zeros((48, 3, 64), dtype=torch.float16), v=torch.zeros((48, 3, 64), dtype=torch.float16)), "must divide"),
        (dict(v=torch.zeros((48, 4, 64), dtype=torch.float16)), "inconsistent"),
    )
    for kw, words in bad:
        args = dict(q=q, k=k, v=k, cu_seqlens_q=cu, cu_seqlens_k=cu)
        args.update(kw)
        with pytest.raises((ValueError, RuntimeError), match="fa2: .*" + words):
            fa(**args)
    for w in (-3, (4, -2), (1, 2, 3), "x"):
        with pytest.raises(ValueError, match="fa2: window is None, an int W"):
            fa(q, k, k, cu, cu, window=w)
    # good arguments on CPU tensors reach the device check — with and without the maxima, the window, the flags
    for kw in (dict(), dict(max_seqlen_q=32, max_seqlen_k=32), dict(causal=True, bottom_right=True, window=(8, None)), dict(window=4, scale=0.5)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            fa(q, k, k, cu, cu, **kw)
    with pytest.raises(RuntimeError, match="ROCm device"):
        FlashAttn.flash_attn_wmma.forward_varlen(q, k, k, cu, cu, 32, 32, 0, 0.125, (-1, -1))
    with pytest.raises(RuntimeError, match="ROCm device"):
        FlashAttn.flash_attn_wmma.backward_varlen(q, q, q, q, q, torch.zeros((4, 48)), cu, cu, 32, 32, 64, 0, 0.125, (-1, -1))
