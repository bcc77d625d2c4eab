"""Grouped-query / multi-query attention at the C-ABI, without a GPU: the grouped entry points exist, validate their arguments before any
launch, and plan exactly the MHA call's kernels (include/fa2_gfx950.h: fa2_fwd_gqa, fa2_bwd_gqa and their size / plan queries)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import FlashAttentionFunction, flash_attention

HEADER = os.path.join(ROOT, "include", "fa2_gfx950.h")
GQA_SYMBOLS = ("fa2_fwd_gqa", "fa2_fwd_gqa_workspace_bytes", "fa2_fwd_gqa_plan", "fa2_bwd_gqa", "fa2_bwd_gqa_workspace_bytes")


def _codes():
    text = open(HEADER).read()
    return {m[0]: int(m[1]) for m in re.findall(r"#define\s+(FA2_\w+)\s+(-?\d+)", text)}


def test_grouped_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _fa2_lib.load()
    for name in GQA_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _fa2_lib.SYMBOLS, name
        assert getattr(lib, name) is not None


def _buf():
    buf = ctypes.create_string_buffer(4096 + 16)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_forward_entry_validation_codes():
    lib = _fa2_lib.load()
    c = _codes()
    buf, p = _buf()
    s3 = _fa2_lib.strides3(8 * 16 * 64, 16 * 64, 64)
    s2 = _fa2_lib.strides2(8 * 16, 16)

    def call(H=8, Hkv=2, k=p, ks=s3, D=64, dtype=0):
        return lib.fa2_fwd_gqa(dtype, p, k, p, p, p, 1, H, Hkv, 16, 16, D, s3, ks, s3, s3, s2, 0.125, 0, None, 0, None)

    assert call(Hkv=3) == c["FA2_ERR_BAD_SHAPE"]            # 3 does not divide 8
    assert call(Hkv=0) == c["FA2_ERR_BAD_SHAPE"] and call(Hkv=-2) == c["FA2_ERR_BAD_SHAPE"]
    assert call(Hkv=16) == c["FA2_ERR_BAD_SHAPE"]           # more K / V heads than Q heads
    assert call(k=None) == c["FA2_ERR_NULL_POINTER"]
    assert call(ks=_fa2_lib.strides3(2048, 1024, 68)) == c["FA2_ERR_ALIGNMENT"]
    assert call(D=44) == c["FA2_ERR_HEAD_DIM"] and call(dtype=5) == c["FA2_ERR_DTYPE"]
    assert lib.fa2_fwd_gqa_workspace_bytes(0, 1, 8, 3, 16, 4096, 64, 0) == 0
    assert lib.fa2_fwd_gqa_workspace_bytes(0, 1, 8, 0, 16, 4096, 64, 0) == 0
    plan = _fa2_lib.FwdPlan()
    assert lib.fa2_fwd_gqa_plan(0, 1, 8, 3, 16, 16, 64, None, None, 0.125, 0, 0, ctypes.byref(plan)) == c["FA2_ERR_BAD_SHAPE"]
    assert lib.fa2_fwd_gqa_plan(0, 1, 8, 9, 16, 16, 64, None, None, 0.125, 0, 0, ctypes.byref(plan)) == c["FA2_ERR_BAD_SHAPE"]
    assert lib.fa2_fwd_gqa_plan(0, 1, 8, 2, 16, 16, 64, None, None, 0.125, 0, 0, None) == c["FA2_ERR_NULL_POINTER"]


def test_backward_entry_validation_codes():
    lib = _fa2_lib.load()
    c = _codes()
    buf, p = _buf()
    s3 = _fa2_lib.strides3(8 * 16 * 64, 16 * 64, 64)
    s2 = _fa2_lib.strides2(8 * 16, 16)

    def call(H=8, Hkv=2, dk=p, dv=p, dks=s3, D=64):
        return lib.fa2_bwd_gqa(0, p, p, p, p, p, p, p, dk, dv, p, 1, H, Hkv, 16, 16, D, s3, s3, s3, s3, s3, s3, dks, s3, s2, 0.125, 0, None, 0, None)

    assert call(Hkv=3) == c["FA2_ERR_BAD_SHAPE"] and call(Hkv=0) == c["FA2_ERR_BAD_SHAPE"] and call(Hkv=16) == c["FA2_ERR_BAD_SHAPE"]
    assert call(dk=None) == c["FA2_ERR_NULL_POINTER"] and call(dv=None) == c["FA2_ERR_NULL_POINTER"]
    assert call(dks=_fa2_lib.strides3(2048, 1024, 66)) == c["FA2_ERR_ALIGNMENT"]
    assert call(D=100) == c["FA2_ERR_HEAD_DIM"]
    assert lib.fa2_bwd_gqa_workspace_bytes(0, 1, 8, 3, 16, 4096, 64, 0) == 0
    assert lib.fa2_bwd_gqa_workspace_bytes(0, 1, 8, 0, 16, 4096, 64, 0) == 0


def test_grouped_cross_attention_backward_asks_for_a_workspace():
    """B2 H10 Hkv2 N4096 x 77 D64: 2 x 2 KV owners sweep 5 x 64 Q tiles each — the split of the dK / dV pass divides that virtual sweep."""
    lib = _fa2_lib.load()
    assert lib.fa2_bwd_gqa_workspace_bytes(0, 2, 10, 2, 4096, 77, 64, 0) > 0
    assert lib.fa2_bwd_gqa_workspace_bytes(1, 2, 10, 2, 4096, 77, 64, 0) > 0
    # Hkv == H asks what fa2_bwd_ws asks
    for shape in ((2, 10, 4096, 77, 64), (1, 16, 4096, 4096, 64), (1, 4, 4096, 4096, 128)):
        B, H, Nq, Nkv, D = shape
        assert lib.fa2_bwd_gqa_workspace_bytes(0, B, H, H, Nq, Nkv, D, 0) == lib.fa2_bwd_workspace_bytes(0, *shape, 0)
        assert lib.fa2_fwd_gqa_workspace_bytes(0, B, H, H, Nq, Nkv, D, 0) == lib.fa2_fwd_workspace_bytes(0, *shape, 0)


def _plans(B, H, Hkv, Nq, Nkv, D, dt, causal, ws=0):
    q = torch.empty((B, H, Nq, D), dtype=dt, device="meta")
    k = torch.empty((B, Hkv, Nkv, D), dtype=dt, device="meta")
    km = torch.empty((B, H, Nkv, D), dtype=dt, device="meta")
    return _fa2_lib.gqa_plan(q, k, causal, workspace_bytes=ws).as_dict(), _fa2_lib.fwd_plan(q, km, causal, workspace_bytes=ws).as_dict()


def test_plan_with_equal_head_counts_is_the_mha_plan_for_every_baseline_config():
    for B, H, N, D, dt, causal in ((1, 2, 128, 64, torch.float16, False), (2, 16, 4096, 128, torch.float16, False),
                                   (2, 16, 4096, 128, torch.bfloat16, True), (1, 32, 8192, 128, torch.float16, True),
                                   (8, 16, 4096, 128, torch.float16, False)):
        for ws in (0, 64 << 20):
            g, m = _plans(B, H, H, N, N, D, dt, causal, ws)
            assert g == m, (B, H, N, D, dt, causal, ws)


@pytest.mark.parametrize("D", [40, 64, 128, 256, 512])
@pytest.mark.parametrize("causal", [False, True])
def test_grouped_plan_names_the_mha_kernel_and_contract(D, causal):
    for B, H, Hkv, Nq, Nkv in ((2, 16, 4, 4096, 4096), (1, 32, 8, 1, 8192), (2, 10, 2, 4096, 77), (1, 16, 1, 1024, 2048)):
        for dt in (torch.float16, torch.bfloat16):
            for ws in (0, 64 << 20):
                g, m = _plans(B, H, Hkv, Nq, Nkv, D, dt, causal, ws)
                assert g == m, (B, H, Hkv, Nq, Nkv, D, dt, causal, ws, g, m)


def test_operator_refuses_a_head_count_that_does_not_divide():
    """Both operator entries refuse k / v whose head count does not divide q's, naming both counts, before any device work (meta tensors here)."""
    q = torch.empty((1, 8, 16, 64), dtype=torch.float16, device="meta")
    k = torch.empty((1, 3, 16, 64), dtype=torch.float16, device="meta")
    kb = torch.empty((1, 16, 3, 64), dtype=torch.float16, device="meta")
    qb = torch.empty((1, 16, 8, 64), dtype=torch.float16, device="meta")
    for call in (lambda: FlashAttentionFunction.apply(q, k, k, None, False),
                 lambda: FlashAttentionFunction.apply(qb, kb, kb, None, True, None, True),
                 lambda: flash_attention(q, k, k, mask=torch.ones((16, 16), dtype=torch.bool, device="meta")),
                 lambda: flash_attention(qb, kb, kb, causal=True, BNHD_fmt=True)):
        with pytest.raises(RuntimeError, match=r"k / v \(3\).*q \(8\)"):
            call()
