"""Sliding-window (local) attention, the parts that need no GPU: the symbols of the C-ABI, their validation codes, the tile-range arithmetic the
kernels and launchers share (fa2_window_tile_range / fa2_window_row_range) against brute force, the plan query, and the operator's argument handling."""
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
WINDOW_SYMBOLS = ("fa2_fwd_window", "fa2_bwd_window", "fa2_fwd_window_plan", "fa2_window_tile_range", "fa2_window_row_range")


def _codes():
    text = open(HEADER).read()
    return {m[0]: int(m[1]) for m in re.findall(r"#define\s+(FA2_\w+)\s+(-?\d+)", text)}


def test_window_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _fa2_lib.load()
    for name in WINDOW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _fa2_lib.SYMBOLS
        assert getattr(lib, name) is not None
    assert re.search(r"FA2_KERNEL_HIP_WINDOW\s*=\s*%d\b" % _fa2_lib.FA2_KERNEL_HIP_WINDOW, text)


def test_validation_codes_of_windows_offsets_and_head_counts():
    lib = _fa2_lib.load()
    c = _codes()
    plan = _fa2_lib.FwdPlan()

    def p(H=8, Hkv=2, Nq=256, Nkv=256, left=64, right=0, off=0, flags=0, out=plan):
        return lib.fa2_fwd_window_plan(0, 1, H, Hkv, Nq, Nkv, 64, None, None, 0.125, flags, left, right, off, 0, ctypes.byref(out) if out is not None else None)

    assert p() == 0
    for bad in (dict(left=-2), dict(right=-2), dict(off=-1), dict(left=2 ** 31 - 1), dict(right=2 ** 31 - 1), dict(off=2 ** 31 - 1),
                dict(Hkv=3), dict(Hkv=9), dict(Hkv=0), dict(flags=4), dict(Nq=0), dict(Nkv=0)):
        assert p(**bad) == c["FA2_ERR_BAD_SHAPE"], bad
    assert p(out=None) == c["FA2_ERR_NULL_POINTER"]
    assert p(left=-1, right=-1) == 0 and p(left=0, right=0) == 0 and p(off=10 ** 6) == 0
    # the launching entry points refuse bad windows before they look at anything else (no GPU is touched)
    s3, s2 = _fa2_lib.strides3(64, 64, 64), _fa2_lib.strides2(1, 1)
    for l, r, o in ((-2, 0, 0), (0, -2, 0), (0, 0, -1), (2 ** 31 - 1, 0, 0)):
        assert lib.fa2_fwd_window(0, None, None, None, None, None, 1, 8, 2, 256, 256, 64, s3, s3, s3, s3, s2, 0.125, 0, l, r, o, None) == c["FA2_ERR_BAD_SHAPE"]
        assert lib.fa2_bwd_window(0, *([None] * 10), 1, 8, 256, 256, 64, *([s3] * 8), s2, 0.125, 0, l, r, o, None) == c["FA2_ERR_BAD_SHAPE"]
    assert lib.fa2_fwd_window(0, None, None, None, None, None, 1, 8, 0, 256, 256, 64, s3, s3, s3, s3, s2, 0.125, 0, 8, 0, 0, None) == c["FA2_ERR_BAD_SHAPE"]
    # a valid window, null tensors: the usual code of the entry point
    assert lib.fa2_fwd_window(0, None, None, None, None, None, 1, 8, 2, 256, 256, 64, s3, s3, s3, s3, s2, 0.125, 0, 8, 0, 0, None) == c["FA2_ERR_NULL_POINTER"]
    assert lib.fa2_bwd_window(0, *([None] * 10), 1, 8, 256, 256, 64, *([s3] * 8), s2, 0.125, 0, 8, 0, 0, None) == c["FA2_ERR_NULL_POINTER"]
    first, n = ctypes.c_int(), ctypes.c_int()
    f, nn = ctypes.byref(first), ctypes.byref(n)
    assert lib.fa2_window_tile_range(64, 64, 8, 0, 0, 0, 0, 32, 64, f, nn) == 0
    assert lib.fa2_window_tile_range(64, 64, 8, 0, 0, 0, 0, 32, 64, None, nn) == c["FA2_ERR_NULL_POINTER"]
    assert lib.fa2_window_row_range(64, 64, 8, 0, 0, 0, 0, 32, 64, f, None) == c["FA2_ERR_NULL_POINTER"]
    for args in ((0, 64, 8, 0, 0, 0, 0, 32, 64), (64, 0, 8, 0, 0, 0, 0, 32, 64), (64, 64, -2, 0, 0, 0, 0, 32, 64), (64, 64, 8, -3, 0, 0, 0, 32, 64),
                 (64, 64, 8, 0, -1, 0, 0, 32, 64), (64, 64, 8, 0, 0, 0, -1, 32, 64), (64, 64, 8, 0, 0, 0, 0, 0, 64), (64, 64, 8, 0, 0, 0, 0, 32, 0)):
        assert lib.fa2_window_tile_range(*args, f, nn) == c["FA2_ERR_BAD_SHAPE"], args
        assert lib.fa2_window_row_range(*args, f, nn) == c["FA2_ERR_BAD_SHAPE"], args
    assert "window" in _fa2_lib.error_string(c["FA2_ERR_BAD_SHAPE"])


def _band(Nq, Nkv, left, right, off, causal):
    """Brute force: the boolean [Nq, Nkv] visibility matrix of the contract in include/fa2_gfx950.h."""
    if causal:
        right = 0
    pos = np.arange(Nq)[:, None] + off
    j = np.arange(Nkv)[None, :]
    keep = np.ones((Nq, Nkv), dtype=bool)
    if left >= 0:
        keep &= j >= pos - left
    if right >= 0:
        keep &= j <= pos + right
    return keep


LENGTHS = (1, 63, 64, 65, 129, 640, 1000)
WINDOWS = (-1, 0, 1, 63, 64, 100, 4096)
TILE = 64


@pytest.mark.parametrize("Nq", LENGTHS)
def test_tile_and_row_ranges_against_brute_force(Nq):
    """Every (Nq, Nkv, left, right, offset, causal, block size) of the grid: the range holds every tile with a visible pair, its first and last tile
    each hold one, an empty band gives ntiles = 0 — for the KV tiles of a block of query rows and for the Q tiles of a block of keys."""
    lib = _fa2_lib.load()
    first, n = ctypes.c_int(), ctypes.c_int()
    f, nn = ctypes.byref(first), ctypes.byref(n)
    checked = 0
    for Nkv in LENGTHS:
        offsets = sorted({0, 1, 64} | ({Nkv - Nq} if Nkv >= Nq else set()))
        for left, right, off, causal in itertools.product(WINDOWS, WINDOWS, offsets, (0, 1)):
            keep = _band(Nq, Nkv, left, right, off, causal)
            # tiles x rows / keys: does tile t hold a key that row i sees (kv_any[i, t]); does Q tile t hold a row that sees key j (q_any[t, j])
            nkt, nqt = (Nkv + TILE - 1) // TILE, (Nq + TILE - 1) // TILE
            kv_any = np.zeros((Nq, nkt), dtype=bool)
            for t in range(nkt):
                kv_any[:, t] = keep[:, t * TILE:(t + 1) * TILE].any(1)
            q_any = np.zeros((nqt, Nkv), dtype=bool)
            for t in range(nqt):
                q_any[t] = keep[t * TILE:(t + 1) * TILE].any(0)
            for rows in (32, 128, 256):
                for fn, live, total in ((lib.fa2_window_tile_range, kv_any, Nq), (lib.fa2_window_row_range, q_any.T, Nkv)):
                    for row0 in range(0, total, rows):
                        assert fn(Nq, Nkv, left, right, off, causal, row0, rows, TILE, f, nn) == 0
                        want = np.nonzero(live[row0:row0 + rows].any(0))[0]
                        case = (fn is lib.fa2_window_row_range, Nq, Nkv, left, right, off, causal, row0, rows, first.value, n.value)
                        if want.size == 0:
                            assert n.value == 0, case
                        else:
                            assert (first.value, first.value + n.value - 1) == (int(want[0]), int(want[-1])), case
                        checked += 1
    assert checked > 1000


def _meta(B, H, Hkv, Nq, Nkv, D, dt):
    return torch.empty((B, H, Nq, D), dtype=dt, device="meta"), torch.empty((B, Hkv, Nkv, D), dtype=dt, device="meta")


def test_plan_without_a_window_is_the_grouped_plan_for_every_baseline_config():
    for B, H, N, D, dt in ((1, 2, 128, 64, torch.float16), (2, 16, 4096, 128, torch.float16), (2, 16, 4096, 128, torch.bfloat16),
                           (1, 32, 8192, 128, torch.float16), (8, 16, 4096, 128, torch.float16)):
        for causal, Hkv, ws in itertools.product((False, True), (H, max(1, H // 4)), (0, 64 << 20)):
            q, k = _meta(B, H, Hkv, N, N, D, dt)
            want = _fa2_lib.gqa_plan(q, k, causal, workspace_bytes=ws).as_dict()
            assert _fa2_lib.window_plan(q, k, causal, -1, -1, 0, workspace_bytes=ws).as_dict() == want, (B, H, N, D, dt, causal, Hkv, ws)
            # windows that mask nothing for these lengths reduce to it too
            assert _fa2_lib.window_plan(q, k, causal, N, -1 if causal else N, 0, workspace_bytes=ws).as_dict() == want
            if causal:      # window_right = 0 without the flag is the flag
                assert _fa2_lib.window_plan(q, k, False, -1, 0, 0, workspace_bytes=ws).as_dict() == want


@pytest.mark.parametrize("D", [40, 64, 128, 256, 512])
def test_plan_of_a_real_window_names_the_windowed_kernel(D):
    for dt in (torch.float16, torch.bfloat16):
        for B, H, Hkv, Nq, Nkv, left, right, off, causal in (
                (2, 16, 4, 4096, 4096, 128, 0, 0, False), (2, 16, 4, 4096, 4096, 255, -1, 0, True), (2, 16, 16, 4096, 4096, -1, 17, 0, False),
                (2, 16, 4, 4096, 4096, -1, -1, 64, True), (1, 32, 8, 1, 8192, 512, 0, 8191, False), (1, 32, 8, 1, 8192, -1, -1, 100, True),
                (1, 4, 4, 129, 1153, 256, 0, 1024, False), (1, 4, 1, 129, 1153, -1, -1, 1024, True), (1, 4, 4, 640, 384, 100, 0, 0, False)):
            q, k = _meta(B, H, Hkv, Nq, Nkv, D, dt)
            pl = _fa2_lib.window_plan(q, k, causal, left, right, off, workspace_bytes=64 << 20)
            assert pl.kernel == _fa2_lib.FA2_KERNEL_HIP_WINDOW and pl.contract == 0, pl.as_dict()
            assert pl.rows in (128, 256) and (D <= 256 or pl.rows == 128) and pl.heads_main == B * H
            assert pl.kernel_tail == 0 and pl.nsplit == 0
    with _fa2_lib.options(rows=128):
        q, k = _meta(2, 16, 16, 4096, 4096, D, torch.float16)
        assert _fa2_lib.window_plan(q, k, True, 127, -1, 0).rows == 128


def test_parse_window():
    pw = _fa2_lib.parse_window
    assert pw(None) == (-1, -1, 0) and pw(7) == (7, 7, 0) and pw((3, None), 5) == (3, -1, 5) and pw((-1, 0)) == (-1, 0, 0) and pw([0, 9], 1) == (0, 9, 1)
    for w, o in ((-1, 0), (-2, 0), ((1,), 0), ((1, 2, 3), 0), ((1, -2), 0), (1.5, 0), ("8", 0), (True, 0), (4, -1), (4, 1.0), (4, None), ((2 ** 31, 0), 0)):
        with pytest.raises(ValueError, match="fa2: window is None, an int W"):
            pw(w, o)


def test_operator_without_a_window_takes_the_old_code_path(monkeypatch):
    """window=None, q_offset=0: flash_attention hands the call to FlashAttentionFunction.apply (mask=None) exactly as before; the windowed launcher is
    never entered."""
    seen = []
    monkeypatch.setattr(FlashAttn.FlashAttentionFunction, "apply", staticmethod(lambda *a, **kw: seen.append((a, kw)) or "old"))

    def boom(*a, **kw):
        raise AssertionError("the windowed launcher must not run")
    monkeypatch.setattr(FlashAttn.flash_attn_wmma, "forward_window", boom)
    monkeypatch.setattr(FlashAttn._WindowAttentionFunction, "apply", boom)
    q = torch.zeros((1, 2, 16, 64), dtype=torch.float16)
    assert FlashAttn.flash_attention(q, q, q, None, True, 0.5, False) == "old"
    assert FlashAttn.flash_attention(q, q, q, causal=True, window=None, q_offset=0) == "old"
    assert seen[0] == ((q, q, q, None, True, 0.5, False), {}) and seen[1][0][3:] == (None, True, None, False)


@pytest.mark.parametrize("frontend", ["py", "compiled"])
def test_operator_refuses_bad_windows_in_both_front_ends(frontend, monkeypatch):
    if frontend == "py":
        monkeypatch.setattr(FlashAttn, "_FRONTEND", [None])
    else:
        fe = FlashAttn._frontend()
        assert fe is not None and hasattr(fe, "forward_window") and hasattr(fe, "backward_window"), "the compiled front end was not built"
    q = torch.zeros((1, 2, 16, 64), dtype=torch.float16)
    for kw in (dict(window=-3), dict(window=(4, -2)), dict(window=(1, 2, 3)), dict(window=4, q_offset=-1), dict(q_offset=-5), dict(window="x")):
        with pytest.raises(ValueError, match="fa2: window is None, an int W"):
            FlashAttn.flash_attention(q, q, q, **kw)
    # below the operator: each front end's own forward / backward refuses the same values with the same words
    for win in ((-2, 0, 0), (0, -2, 0), (0, 0, -1)):
        with pytest.raises((ValueError, RuntimeError), match="fa2: window is None, an int W"):
            FlashAttn.flash_attn_wmma.forward_window(q, q, q, 64, 128, False, 0.125, False, win)
        with pytest.raises((ValueError, RuntimeError), match="fa2: window is None, an int W"):
            FlashAttn.flash_attn_wmma.backward_window(q, q, q, q, q, torch.zeros((1, 2, 16)), 16, 16, 64, 128, 128, False, 0.125, False, win)
    # a good window on CPU tensors reaches the device check, not the window check
    with pytest.raises(RuntimeError, match="ROCm device"):
        FlashAttn.flash_attention(q, q, q, window=(4, 0))
