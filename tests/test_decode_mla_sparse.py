"""CPU tests of sparse (top-k indexed) MLA decode (include/fa2_gfx950.h: fa2_fwd_decode_mla_sparse and its queries).  Nothing here touches a device."""
import re
import subprocess

import pytest
import torch

import decode_calls as dc
from rocwmma_fattn import FlashAttn, _fa2_lib
from test_decode_mla import ALIGN, BAD_ALIGN, BAD_SCALE, BF16, DEFAULTS, DTYPE, F16, GRID, HEAD_DIM, HEADER, NULLP, OK, SCALE, SHAPE

P, I32_MIN, I32_MAX = dc.HOST, -2 ** 31, 2 ** 31 - 1


def test_symbols_plan_and_workspace():
    lib = _fa2_lib.load()
    for name in ("fa2_fwd_decode_mla_sparse", "fa2_fwd_decode_mla_sparse_plan", "fa2_fwd_decode_mla_sparse_workspace_bytes", "fa2_decode_mla_sparse_entry"):
        assert name + "(" in open(HEADER).read() and getattr(lib, name).argtypes == _fa2_lib.SYMBOLS[name][1], name
    ws = lib.fa2_fwd_decode_mla_sparse_workspace_bytes
    for (dt, B, H, Nq, cap, page, topk) in ((BF16, 1, 128, 1, 65536, 0, 2048), (F16, 32, 16, 1, 1024, 64, 2048), (F16, 2, 17, 3, 320, 0, 69), (F16, 1, 1, 1, 1, 0, 1),
                                            (BF16, 1, 65, 2, 300, 0, 1 << 20), (F16, 256, 16, 1, 4096, 0, 2048)):
        blocks = Nq * -(-H // 64)
        want = 1 if B * blocks >= 256 else max(1, min(256 // (B * blocks), 128, -(-topk // 32) // 8))
        assert _fa2_lib.decode_mla_sparse_plan(dt, B, H, Nq, cap, topk, page).as_dict() == dict(
            kernel=_fa2_lib.FA2_KERNEL_HIP_DECODE_MLA_SPARSE, nsplit=want, row_blocks=blocks, key_tile=32, max_split=128), (B, H, Nq, cap, topk)
        assert ws(dt, B, H, Nq, 576, 512, cap, page, 0, topk) == (0 if want == 1 else B * want * Nq * H * 513 * 4)
        assert ws(dt, B, H, Nq, 576, 512, cap, page, 5, topk) == B * 5 * Nq * H * 513 * 4
    plan, ok = _fa2_lib.DecodeMlaPlan(), dict(dt=F16, B=1, H=16, Nq=1, D=576, Dv=512, cap=256, page=0, ns=2, topk=64)
    rc = lambda **kw: lib.fa2_fwd_decode_mla_sparse_plan(*dict(ok, **kw).values(), plan)      # noqa: E731
    assert rc() == OK and rc(topk=I32_MAX - 64) == OK and lib.fa2_fwd_decode_mla_sparse_plan(*ok.values(), None) == NULLP
    for kw, code in ((dict(topk=0), SHAPE), (dict(topk=-1), SHAPE), (dict(topk=I32_MAX - 63), SHAPE), (dict(topk=0, D=512), SHAPE), (dict(D=512), HEAD_DIM), (dict(dt=2), DTYPE)):
        assert rc(**kw) == code and ws(*dict(ok, **kw).values()) == 0, kw                  # (sizes before the head dim; a refused call: no workspace)


def test_the_new_codes_and_their_place_in_the_order():
    def _call(idx=P, topk=64, ids=_fa2_lib.strides2(64, 64), **kw):
        return _fa2_lib.load().fa2_fwd_decode_mla_sparse(*dc.c_args("mla", **dict(DEFAULTS, stream=None, **kw)), idx, topk, ids)
    neg = _fa2_lib.strides2(-1, 64)
    assert _call(B=65536) == GRID                                                       # well-formed but for the grid: everything before it passed
    assert _call(idx=None) == NULLP and _call(ids=None) == NULLP and _call(idx=None, topk=0, D=512, ks=BAD_ALIGN, dtype=2) == NULLP
    for kw in (dict(topk=0), dict(topk=-3), dict(topk=I32_MAX - 63), dict(ids=neg), dict(ids=_fa2_lib.strides2(64, -64)), dict(topk=0, D=512, ks=BAD_ALIGN, dtype=2)):
        assert _call(**kw) == SHAPE, kw
    assert _call(ids=neg, D=512) == HEAD_DIM and _call(D=512, idx=P + 2, dtype=2) == HEAD_DIM          # the sizes, the head dim, then the strides' signs
    assert _call(ids=neg, idx=P + 2, dtype=2) == SHAPE
    assert _call(idx=P + 2, dtype=2, scale=BAD_SCALE) == ALIGN and _call(idx=P + 1) == ALIGN and _call(idx=P + 4, B=65536) == GRID      # 4 bytes are enough
    assert _call(dtype=2, scale=BAD_SCALE, B=65536) == DTYPE and _call(scale=BAD_SCALE, B=65536, ns=2) == SCALE
    assert _call(B=65536, ns=2) == GRID and _call(ns=2) == NULLP and _call(ns=2, ws=P, wsb=2 * 2 * 16 * 513 * 4 - 1) == SHAPE      # the grid, then the workspace


def test_python_argument_checks():
    q, kv, lens = torch.zeros(2, 3, 16, 576, dtype=torch.float16), torch.zeros(2, 128, 576, dtype=torch.float16), torch.full((2,), 5, dtype=torch.int32)
    good = torch.zeros(2, 3, 8, dtype=torch.int32)
    for bad in (good.long(), good.float(), good[:, :2], good[:1], good[0], good[:, :, :0], good[:, :, ::2], good.transpose(0, 2).contiguous().transpose(0, 2), good.tolist(), 7):
        with pytest.raises(ValueError, match="indices"):
            FlashAttn.flash_attention_decode_mla(q, kv, lens, indices=bad)


def test_entry_arithmetic_against_brute_force():
    for capacity, page in ((1, 0), (33, 0), (100, 0), (1, 64), (3, 64), (2, 128)):
        keys = capacity * page if page else capacity
        for length in sorted({-70, 0, 1, 2, 33, 64, 65, keys - 1, keys, keys + 1, 2 ** 40}):
            for Nq, i in ((1, 0), (3, 0), (3, 2)):
                pos = min(max(length, 0), keys) - Nq + i
                for j in {I32_MIN, I32_MIN + 1, -64, -1, 0, 1, 31, 32, 63, 64, 65, 127, 128, pos - 1, pos, pos + 1, pos + Nq, keys - 1, keys, keys + 64, I32_MAX - 1,
                          I32_MAX} | set(range(0, keys, 7)):
                    want = (1, j // page if page else 0, j % page if page else j) if 0 <= j <= pos else (0, 0, 0)
                    assert _fa2_lib.decode_mla_sparse_entry(j, length, Nq, i, capacity, page) == want, (capacity, page, length, Nq, i, j)


def test_no_kernel_of_the_new_unit_has_a_private_segment():
    build, found = _fa2_lib._build_module(), {}
    assert "fa2_decode_mla_sparse.hip.h" in build.HEADERS
    for u in [u for u in build.UNITS if u[1] == "decode_mla_sparse_hip.cpp"]:
        cmd = [build._hipcc()] + [f for f in build.HIPCC_FLAGS if f != "--offload-compress"] + list(u[2]) + ["-I", build.INCLUDE, "-I", build.CSRC]
        text = subprocess.run(cmd + ["--cuda-device-only", "-S", build.CSRC + "/" + u[1], "-o", "-"], capture_output=True, text=True, check=True).stdout
        for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
            found[name] = [int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1)) for k in ("private_segment_fixed_size", "uses_dynamic_stack")]
    assert len(found) == 4 and sum("decode_mla_sparse_kernel" in n for n in found) == 2 and sum("decode_combine_kernelILi512" in n for n in found) == 2, sorted(found)
    assert all(v == [0, 0] for v in found.values()), found
