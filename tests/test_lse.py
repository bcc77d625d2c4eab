"""The differentiable LSE and the merge of partial attention results, checks that need no GPU: the C-ABI's new symbols (declared in
include/fa2_gfx950.h, exported by the library, bound in _fa2_lib.SYMBOLS), the validation codes of their own arguments and the order they are checked in
(every rejected call returns before any launch: the tensors are host buffers that are never read), the plan query, and the operator's argument handling."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention, flash_attention_varlen, merge_attention

HEADER = os.path.join(ROOT, "include", "fa2_gfx950.h")
NEW = ("fa2_bwd_lse", "fa2_bwd_window_lse", "fa2_bwd_varlen_lse", "fa2_bwd_lse_plan", "fa2_merge_fwd", "fa2_merge_bwd")
ERR_NULL, ERR_SHAPE, ERR_HEAD_DIM, ERR_ALIGN, ERR_DROPOUT, ERR_SOFTCAP = -1, -2, -3, -4, -9, -10


def _buf():
    buf = ctypes.create_string_buffer(8192 + 16)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(fa2_\w+)\s*\(", text))
    lib = _fa2_lib.load()
    for name in NEW:
        assert name in declared, name
        assert name in _fa2_lib.SYMBOLS, name
        assert getattr(lib, name).argtypes == _fa2_lib.SYMBOLS[name][1]
    assert re.search(r"enum\s*\{\s*FA2_MERGE_NATURAL_LSE\s*=\s*1\s*\}", text)          # an enumerator, like FA2_KERNEL_HIP_WINDOW
    assert _fa2_lib.FA2_MERGE_NATURAL_LSE == 1


def test_dlse_arguments_are_validated_last():
    lib = _fa2_lib.load()
    keep, p = _buf()
    s3 = _fa2_lib.strides3(2 * 16 * 64, 16 * 64, 64)
    s2 = _fa2_lib.strides2(32, 16)
    neg = _fa2_lib.strides2(-32, 16)
    base = (0, p, p, p, p, p, p, p, p, p, p, 1, 2, 16, 16, 64, s3, s3, s3, s3, s3, s3, s3, s3, s2, 0.125)

    def dense(dlse=p + 2, dls=s2, D=64, q=p):
        a = list(base)
        a[1], a[15] = q, D
        return lib.fa2_bwd_lse(*a, 0, None, 0, None, None, 0, None, dlse, dls)

    assert dense() == ERR_ALIGN and dense(dlse=p + 4, dls=neg) == ERR_SHAPE
    assert dense(D=44) == ERR_HEAD_DIM and dense(q=None) == ERR_NULL               # another defect wins: the dlse pair is checked last
    assert dense(dlse=p + 4, dls=None) == ERR_NULL

    def window(dlse=p + 2, dls=s2, p_drop=0.0, cap=0.0, slopes=None, left=3, D=64):
        a = list(base)
        a[15] = D
        return lib.fa2_bwd_window_lse(*a, 0, left, 0, 0, None, p_drop, 7, cap, slopes, 0, dlse, dls)

    assert window() == ERR_ALIGN and window(dlse=p + 4, dls=neg) == ERR_SHAPE
    assert window(p_drop=1.5) == ERR_DROPOUT and window(cap=-1.0) == ERR_SOFTCAP     # today's codes, ahead of everything else
    assert window(p_drop=1.5, cap=-1.0) == ERR_DROPOUT                                # ... dropout_p first
    assert window(p_drop=0.25, cap=30.0) == ERR_DROPOUT and window(p_drop=0.25, slopes=p) == ERR_DROPOUT      # never both
    assert window(left=-2) == ERR_SHAPE and window(D=44) == ERR_HEAD_DIM

    cu = p + 4096
    s2p = _fa2_lib.strides2(64, 128)

    def packed(dlse=p + 2, stride=16, p_drop=0.0, cap=0.0, D=64):
        return lib.fa2_bwd_varlen_lse(0, p, p, p, p, p, p, p, p, p, p, 1, 2, 16, 16, D, cu, cu, s2p, s2p, s2p, s2p, s2p, s2p, s2p, s2p, 16, 0.125, 0, -1, -1, None,
                                      p_drop, 7, cap, None, 0, dlse, stride)

    assert packed() == ERR_ALIGN and packed(dlse=p + 4, stride=-1) == ERR_SHAPE
    assert packed(p_drop=0.25, cap=30.0) == ERR_DROPOUT and packed(D=44) == ERR_HEAD_DIM
    del keep


def test_merge_validation_codes():
    lib = _fa2_lib.load()
    keep, p = _buf()
    s3 = _fa2_lib.strides3(2 * 16 * 64, 16 * 64, 64)
    s2 = _fa2_lib.strides2(32, 16)

    def arr(n, ptr=p):
        return (ctypes.c_void_p * max(n, 1))(*([ptr] * max(n, 1)))

    def fwd(n=2, D=64, parts=None, ps=s3, flags=0, o=p):
        return lib.fa2_merge_fwd(0, n, parts if parts is not None else arr(n), arr(n), o, p, 1, 2, 16, D, ps, s2, s3, s2, flags, None)

    def bwd(n=2, D=64, dparts=None):
        return lib.fa2_merge_bwd(0, n, arr(n), arr(n), p, p, None, dparts if dparts is not None else arr(n), arr(n), 1, 2, 16, D, s3, s2, s2, s3, None, s3, s2,
                                 0, None)

    for call in (fwd, bwd):
        assert call(n=0) == ERR_SHAPE and call(n=17) == ERR_SHAPE
        assert call(D=44) == ERR_HEAD_DIM and call(D=520) == ERR_HEAD_DIM
    assert fwd(flags=2) == ERR_SHAPE
    assert fwd(parts=arr(2, p + 2)) == ERR_ALIGN and fwd(ps=_fa2_lib.strides3(2048, 1024, 68)) == ERR_ALIGN
    assert fwd(o=None) == ERR_NULL and bwd(dparts=arr(2, None)) == ERR_NULL
    assert lib.fa2_merge_fwd(7, 2, arr(2), arr(2), p, p, 1, 2, 16, 64, s3, s2, s3, s2, 0, None) == -5
    del keep


def test_plan_query_reports_the_fallback_of_a_call_with_dlse():
    lib = _fa2_lib.load()
    HIP, ASM = _fa2_lib.FA2_BWD_KERNEL_HIP, _fa2_lib.FA2_BWD_KERNEL_ASM

    def plans(dt, B, H, Nq, Nkv, D, causal, has):
        a, b = _fa2_lib.BwdPlan(), _fa2_lib.BwdPlan()
        args = (dt, B, H, H, Nq, Nkv, D, None, None, None, None, None, D ** -0.5, causal, 0, None)
        assert lib.fa2_bwd_plan(*args, ctypes.byref(a)) == 0
        assert lib.fa2_bwd_lse_plan(*args, has, ctypes.byref(b)) == 0
        return (a.dq_kernel, a.dkv_kernel), (b.dq_kernel, b.dkv_kernel)

    for shape in ((0, 1, 2, 128, 128, 64, 0), (1, 2, 16, 4096, 4096, 128, 0), (0, 2, 4, 256, 256, 128, 1), (1, 1, 8, 4096, 77, 64, 0), (0, 1, 2, 200, 333, 320, 0),
                  (0, 2, 4, 250, 256, 128, 0)):
        old, new = plans(*shape, 0)
        assert old == new, shape
    old, new = plans(0, 2, 4, 256, 256, 128, 0, 1)
    assert old == (ASM, ASM), "the hand-scheduled passes serve this shape without a dlse"
    assert ASM not in new and new == (HIP, HIP)
    assert lib.fa2_bwd_lse_plan(0, 1, 1, 1, 16, 16, 64, None, None, None, None, None, 0.125, 0, 0, None, 1, None) == ERR_NULL


def test_operator_surface_without_a_gpu():
    q = torch.rand(1, 2, 16, 64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        flash_attention(q, q, q, return_lse=True)
    with pytest.raises(RuntimeError, match="ROCm device"):
        flash_attention(q, q, q, causal=True, window=(3, 0), return_lse=True)
    cu = torch.tensor([0, 16], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="ROCm device"):
        flash_attention_varlen(q[0].transpose(0, 1), q[0].transpose(0, 1), q[0].transpose(0, 1), cu, cu, 16, 16, return_lse=True)
    with pytest.raises(RuntimeError, match="ROCm device"):
        merge_attention([q, q], [torch.zeros(1, 2, 16), torch.zeros(1, 2, 16)])
    with pytest.raises(ValueError):
        merge_attention([q, q], [torch.zeros(1, 2, 16)])
