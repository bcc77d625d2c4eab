"""Packed attention with V narrower than K (fa2_fwd_varlen_dv, the non-absorbed MLA prefill), the parts that need no GPU: the symbols of the C-ABI, every
validation code and the order of the checks on host memory that is never touched, the plan query, the operator's refusals, and the new unit compiled for
gfx950 without a private segment."""
import concurrent.futures
import ctypes
import importlib.util
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT
from rocwmma_fattn import FlashAttn, _fa2_lib

HEADER = os.path.join(ROOT, "include", "fa2_gfx950.h")
PKG = os.path.join(ROOT, "flash-attention-v2-rdna3-minimal_amd")
CAUSAL, EXACT, BOTTOM_RIGHT = _fa2_lib.FA2_FLAG_CAUSAL, _fa2_lib.FA2_FLAG_EXACT_SCALE, _fa2_lib.FA2_FLAG_BOTTOM_RIGHT


def _codes():
    text = open(HEADER).read()
    return {m[0]: int(m[1]) for m in re.findall(r"#define\s+(FA2_\w+)\s+(-?\d+)", text)}


def test_symbols_are_declared_bound_and_exported_with_their_argument_counts():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _fa2_lib.load()
    for name, twin, nargs in (("fa2_fwd_varlen_dv", "fa2_fwd_varlen", 25), ("fa2_fwd_varlen_dv_plan", "fa2_fwd_varlen_plan", 15)):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, (name, decl.group(1))
        assert name in _fa2_lib.SYMBOLS and getattr(lib, name) is not None
        assert len(_fa2_lib.SYMBOLS[name][1]) == nargs == len(_fa2_lib.SYMBOLS[twin][1]) + 1        # the twin's list with Dv after D
        assert re.search(r"\bint D, int Dv\b", decl.group(1)), name
    # an enumerator, not a #define: tests/test_boundary.py pins the macro list
    assert re.search(r"enum\s*\{\s*FA2_KERNEL_HIP_VARLEN_DV\s*=\s*%d\s*\}" % _fa2_lib.FA2_KERNEL_HIP_VARLEN_DV, text)
    assert _fa2_lib.FA2_KERNEL_HIP_VARLEN_DV == 10 and "FA2_KERNEL_HIP_VARLEN_DV" not in _codes()
    assert hasattr(FlashAttn.flash_attn_wmma, "forward_varlen_dv")


def test_every_validation_code_and_the_order_of_the_checks():
    """The plan query and the launching entry point (null tensors: nothing touches a device) refuse every bad argument with fa2_fwd_varlen's code, and a
    call with two defects gets the code of the one that fa2_fwd_varlen's order reaches first."""
    lib = _fa2_lib.load()
    c = _codes()
    plan = _fa2_lib.FwdPlan()
    good = _fa2_lib.strides2(192, 8 * 192)

    def calls(dtype=0, B=3, H=8, Hkv=2, mq=256, mk=256, D=192, Dv=128, qs=good, ks=good, vs=None, scale=0.07, flags=0, left=64, right=0, out=plan):
        po = ctypes.byref(out) if out is not None else None
        vs = ks if vs is None else vs
        return (lib.fa2_fwd_varlen_dv_plan(dtype, B, H, Hkv, mq, mk, D, Dv, qs, ks, scale, flags, left, right, po),
                lib.fa2_fwd_varlen_dv(dtype, None, None, None, None, None, B, H, Hkv, mq, mk, D, Dv, None, None, qs, ks, vs, qs, 0, scale, flags, left, right, None))

    null, shape, hd, align = c["FA2_ERR_NULL_POINTER"], c["FA2_ERR_BAD_SHAPE"], c["FA2_ERR_HEAD_DIM"], c["FA2_ERR_ALIGNMENT"]
    # good arguments: the plan answers; the launching entry point gets as far as its null tensors
    assert calls() == (0, null)
    for bad in (dict(B=0), dict(H=0), dict(D=0), dict(Dv=0), dict(Dv=-8), dict(mq=0), dict(mk=0), dict(mq=-5), dict(left=-2), dict(right=-2),
                dict(left=2 ** 31 - 1), dict(flags=8), dict(flags=16 | CAUSAL), dict(mq=2 ** 31 - 1000), dict(Hkv=3), dict(Hkv=9), dict(Hkv=0)):
        assert calls(**bad) == (shape, shape), bad
    # the head dim: fa2_fwd_varlen's rule, then the served pairs
    for bad in (dict(D=520), dict(D=196), dict(D=128), dict(D=64, Dv=32), dict(D=264), dict(D=192, Dv=136), dict(D=192, Dv=192), dict(D=192, Dv=100),
                dict(D=256, Dv=256), dict(D=136, Dv=4), dict(D=512, Dv=128)):
        assert calls(**bad) == (hd, hd), bad
    for ok in (dict(D=192, Dv=128), dict(D=256, Dv=128), dict(D=136, Dv=8), dict(D=192, Dv=64), dict(D=136, Dv=72), dict(D=200, Dv=120)):
        s = _fa2_lib.strides2(ok["D"], 8 * ok["D"])
        assert calls(qs=s, ks=s, **ok) == (0, null), ok
    assert calls(dtype=2) == (c["FA2_ERR_DTYPE"],) * 2
    assert calls(scale=float("nan")) == (c["FA2_ERR_SCALE"],) * 2 and calls(scale=float("inf")) == (c["FA2_ERR_SCALE"],) * 2
    assert calls(qs=_fa2_lib.strides2(192, 8 * 192 + 4)) == (align, align)
    assert calls(ks=_fa2_lib.strides2(12, 8 * 192)) == (align, align)
    assert calls(vs=_fa2_lib.strides2(128, 2 * 128 + 4))[1] == align                 # v's strides are its own
    assert calls(vs=_fa2_lib.strides2(256, 2 * 256))[1] == null                      # ... a slice of a 256-wide buffer is fine
    # a stated maximum whose K span reaches 2 GiB; V's span rule counts Dv columns in its last row
    assert calls(mk=2 ** 21, ks=_fa2_lib.strides2(192, 512)) == (shape, shape)
    assert calls(mk=2 ** 21 - 128, ks=_fa2_lib.strides2(192, 512))[0] == 0
    edge = (2 ** 31 - 1 - 2 * 128) // (2 * 512) - 63              # the largest mk whose V span, Dv = 128 columns in the last row plus 64 rows of slack, fits
    assert calls(mk=edge, ks=_fa2_lib.strides2(192, 256), vs=_fa2_lib.strides2(128, 512))[1] == null
    assert calls(mk=edge + 1, ks=_fa2_lib.strides2(192, 256), vs=_fa2_lib.strides2(128, 512))[1] == shape
    assert calls(B=2 ** 20, H=64, Hkv=64, mq=2 ** 16, mk=64) == (c["FA2_ERR_GRID"],) * 2
    assert calls(out=None)[0] == null
    for flags in range(8):
        assert calls(flags=flags) == (0, null), flags
    assert calls(qs=None, ks=None)[0] == 0                       # NULL strides in the plan query: contiguous tensors
    assert lib.fa2_fwd_varlen_dv(0, None, None, None, None, None, 3, 8, 2, 256, 256, 192, 128, None, None, None, good, good, good, 0, 0.07, 0, -1, -1, None) == null
    # the order, on calls with two defects: sizes (Dv among them), flags, window, null stride arrays — then dtype, head dim and pair, scale, alignment,
    # span, grid — then the tensors
    assert calls(Dv=0, D=196) == (shape, shape) and calls(Dv=0, dtype=2) == (shape, shape) and calls(Dv=0, flags=8) == (shape, shape)
    assert lib.fa2_fwd_varlen_dv(0, None, None, None, None, None, 3, 8, 2, 256, 256, 192, 0, None, None, None, good, good, good, 0, 0.07, 0, -1, -1, None) == shape
    assert lib.fa2_fwd_varlen_dv(2, None, None, None, None, None, 3, 8, 2, 256, 256, 192, 100, None, None, None, good, good, good, 0, 0.07, 0, -1, -1, None) == null
    assert calls(dtype=2, Dv=100) == (c["FA2_ERR_DTYPE"],) * 2               # dtype ahead of the head dim
    assert calls(Dv=100, scale=float("nan")) == (hd, hd)                    # the pair ahead of the scale, as the head dim is
    assert calls(D=196, scale=float("nan")) == (hd, hd)
    assert calls(Hkv=3, Dv=100) == (shape, shape)                           # the head grouping ahead of the head dim
    assert calls(scale=float("nan"), qs=_fa2_lib.strides2(192, 8 * 192 + 4)) == (c["FA2_ERR_SCALE"],) * 2
    assert calls(Dv=100, ks=_fa2_lib.strides2(12, 8 * 192)) == (hd, hd)
    assert calls(ks=_fa2_lib.strides2(12, 512), mk=2 ** 21) == (align, align)                   # alignment ahead of the span
    # fa2_fwd_varlen itself is untouched by the new field: equal widths only, its codes as they were
    s64 = _fa2_lib.strides2(64, 8 * 64)
    assert lib.fa2_fwd_varlen(0, None, None, None, None, None, 3, 8, 2, 256, 256, 64, None, None, s64, s64, s64, s64, 0, 0.125, 0, 64, 0, None) == null
    assert lib.fa2_fwd_varlen_plan(0, 3, 8, 2, 256, 256, 192, None, None, 0.07, 0, 64, 0, ctypes.byref(plan)) == 0 and plan.kernel == _fa2_lib.FA2_KERNEL_HIP_VARLEN


@pytest.mark.parametrize("D,Dv", [(192, 128), (256, 128), (136, 8), (192, 64)])
def test_plan_names_the_kernel_contract_zero_and_the_rows_as_launched(D, Dv):
    lib = _fa2_lib.load()
    plan = _fa2_lib.FwdPlan()
    for dt in (_fa2_lib.FA2_DTYPE_F16, _fa2_lib.FA2_DTYPE_BF16):
        for B, H, Hkv, mq, mk, flags, left, right in ((8, 16, 16, 8192, 8192, 0, -1, -1), (4, 128, 128, 4096, 4096, CAUSAL, -1, -1),
                                                      (16, 32, 8, 4096, 4096, CAUSAL | BOTTOM_RIGHT, 127, -1), (3, 4, 1, 1, 1000, EXACT, 5, 9),
                                                      (1, 2, 2, 100, 1, CAUSAL | BOTTOM_RIGHT | EXACT, -1, -1)):
            assert lib.fa2_fwd_varlen_dv_plan(dt, B, H, Hkv, mq, mk, D, Dv, None, None, D ** -0.5, flags, left, right, ctypes.byref(plan)) == 0
            assert plan.kernel == _fa2_lib.FA2_KERNEL_HIP_VARLEN_DV and plan.contract == 0, plan.as_dict()
            assert plan.rows in (128, 256) and plan.heads_main == B * H
            assert plan.kernel_tail == 0 and plan.contract_tail == 0 and plan.rows_tail == 0 and plan.nsplit == 0 and plan.split_items == 0
        for rows in (128, 256):             # (both workgroup shapes are compiled without scratch: option "rows" is honoured)
            with _fa2_lib.options(rows=rows):
                assert lib.fa2_fwd_varlen_dv_plan(dt, 8, 16, 4, 4096, 4096, D, Dv, None, None, D ** -0.5, CAUSAL, -1, -1, ctypes.byref(plan)) == 0
                assert plan.rows == rows and plan.kernel == _fa2_lib.FA2_KERNEL_HIP_VARLEN_DV


def test_operator_refusals_on_cpu_tensors():
    f16 = torch.float16
    q, k, v = torch.zeros((48, 4, 192), dtype=f16), torch.zeros((48, 2, 192), dtype=f16), torch.zeros((48, 2, 128), dtype=f16)
    cu = torch.tensor([0, 16, 48], dtype=torch.int32)
    fa = FlashAttn.flash_attention_varlen
    z = lambda *shape: torch.zeros(shape, dtype=f16)      # noqa: E731
    # pairs outside the served set
    for qq, kk, vv in ((z(48, 4, 128), z(48, 2, 128), z(48, 2, 64)), (q, k, z(48, 2, 136)), (q, k, z(48, 2, 100)), (q, k, z(48, 2, 256)),
                       (z(48, 4, 264), z(48, 2, 264), v), (z(48, 4, 196), z(48, 2, 196), v), (z(48, 4, 64), z(48, 2, 64), z(48, 2, 128))):
        with pytest.raises(ValueError, match="fa2: .*136 .. 256.*8 .. 128"):
            fa(qq, kk, vv, cu, cu)
    # dropout, softcap, ALiBi slopes
    for kw in (dict(dropout_p=0.1), dict(dropout_p=0.5, dropout_seed=3), dict(softcap=30.0), dict(alibi_slopes=torch.ones(4))):
        with pytest.raises(ValueError, match="fa2: .*no dropout_p > 0, softcap or alibi_slopes"):
            fa(q, k, v, cu, cu, **kw)
    # forward only
    for which in range(3):
        t = [q.clone(), k.clone(), v.clone()]
        t[which].requires_grad_(True)
        with pytest.raises(ValueError, match="fa2: .*forward only"):
            fa(*t, cu, cu)
        with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm device"):
            fa(*t, cu, cu)
    # a v whose token count or head count differs from k's stays the "inconsistent" error it is
    for vv in (z(47, 2, 128), z(48, 4, 128), z(48, 1, 128), z(48, 4, 192)):
        with pytest.raises(RuntimeError, match="fa2: inconsistent"):
            fa(q, k, vv, cu, cu)
    with pytest.raises(ValueError, match="fa2: window is None, an int W"):
        fa(q, k, v, cu, cu, window=-3)
    with pytest.raises(ValueError, match="fa2: .*int32"):
        fa(q, k, v, cu.long(), cu)
    # good arguments reach the device check — with and without the maxima, the window, the flags, the LSE
    for kw in (dict(), dict(max_seqlen_q=32, max_seqlen_k=32), dict(causal=True, bottom_right=True, window=(8, None)), dict(window=4, scale=0.5),
               dict(return_lse=True), dict(dropout_p=0.0, softcap=0.0)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            fa(q, k, v, cu, cu, **kw)
    with pytest.raises(RuntimeError, match="ROCm device"):
        FlashAttn.flash_attn_wmma.forward_varlen_dv(q, k, v, cu, cu, 32, 32, 0, 0.07, (-1, -1))
    # Dv == D still reaches it, on the path it always took; the other packed entry points keep refusing unequal widths
    for kw in (dict(), dict(return_lse=True), dict(causal=True)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            fa(q, k, k, cu, cu, **kw)
    with pytest.raises(RuntimeError, match="fa2: inconsistent"):
        FlashAttn.flash_attn_wmma.forward_varlen(q, k, v, cu, cu, 32, 32, 0, 0.07, (-1, -1))


def test_no_kernel_of_the_new_unit_has_a_private_segment():
    """varlen_dv_hip.cpp compiled for gfx950 with the product build's flags, both dtypes: eight kernels — 128- and 256-row workgroups, 12 and 16 Q.K^T
    k-steps, twice — none with scratch, none with a dynamic stack."""
    spec = importlib.util.spec_from_file_location("_fa2_build_varlen_dv", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    units = [u for u in build.UNITS if u[1] == "varlen_dv_hip.cpp"]
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
                           int(re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", body).group(1)),
                           int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)))
    assert len(found) == 8 and all("fwd_varlen_dv_kernelILi256ELi128E" in n for n in found), sorted(found)
    for nw, ksq in ((4, 12), (4, 16), (8, 12), (8, 16)):
        assert sum(("Lb0ELi%dELi1ELi0ELi%dELi4ELb1EEE" % (nw, ksq)) in n for n in found) == 2, (nw, ksq, sorted(found))
    assert all(v == (0, 0, 0) for v in found.values()), found         # (the LDS is dynamic: 96 KiB at launch)
