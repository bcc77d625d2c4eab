"""CPU tests of MLA decode on an e4m3 latent cache of 656-byte rows (include/fa2_gfx950.h: fa2_fwd_decode_mla_fp8, fa2_fwd_decode_mla_sparse_fp8): the
symbols, the new refusals in their place, the operator's argument checks, the two conversion helpers against the contract in float64, and the private
segment of the new units.  Nothing here touches a device."""
import concurrent.futures
import re
import subprocess

import pytest
import torch

import decode_calls as dc
from rocwmma_fattn import FlashAttn, _fa2_lib
from test_decode_mla import ALIGN, DEFAULTS, GRID, HEAD_DIM, HEADER, NULLP, SHAPE

P = dc.HOST
ROW = 656


def ks(row, page=None):
    return _fa2_lib.strides3(256 * row if page is None else page, ROW, row)


def _call(sparse, **kw):
    args = dc.c_args("mla", **dict(DEFAULTS, stream=None, **dict(dict(ks=ks(ROW)), **kw)))
    if sparse:
        return _fa2_lib.load().fa2_fwd_decode_mla_sparse_fp8(*args, P, 64, _fa2_lib.strides2(64, 64))
    return _fa2_lib.load().fa2_fwd_decode_mla_fp8(*args)


@pytest.mark.parametrize("sparse", [False, True])
def test_symbols_and_the_new_refusals_in_their_place(sparse):
    name = "fa2_fwd_decode_mla_sparse_fp8" if sparse else "fa2_fwd_decode_mla_fp8"
    assert name + "(" in open(HEADER).read() and getattr(_fa2_lib.load(), name).argtypes == _fa2_lib.SYMBOLS[name][1] == _fa2_lib.SYMBOLS[name[:-4]][1]
    assert _call(sparse, B=65536) == GRID                                                 # well-formed but for the grid: 656-byte rows pass every check
    assert _call(sparse, ks=ks(672), B=65536) == GRID and _call(sparse, ks=ks(ROW, 8), B=65536) == ALIGN      # a pitch of 672; a page stride of 8 bytes
    assert _call(sparse, k=None) == NULLP and _call(sparse, k=None, ks=ks(640)) == NULLP
    for row in (640, 664, 0, -656):                                                       # below 656; no multiple of 16
        assert _call(sparse, ks=ks(row)) == SHAPE and _call(sparse, ks=ks(row), k=P + 8, dtype=2) == SHAPE, row
        assert _call(sparse, ks=ks(row), D=512) == HEAD_DIM, row                          # ... with the strides' signs, after the head dim
    assert _call(sparse, k=P + 8) == ALIGN and _call(sparse, k=P + 8, dtype=2) == ALIGN   # the base: before the dtype


def test_python_argument_checks(monkeypatch):
    f = FlashAttn.flash_attention_decode_mla
    q, lens = torch.zeros(2, 1, 16, 576, dtype=torch.float16), torch.full((2,), 5, dtype=torch.int32)
    c8, new = torch.zeros(2, 128, ROW, dtype=torch.uint8), dict(kv_c=torch.zeros(2, 1, 512, dtype=torch.float16), k_pe=torch.zeros(2, 1, 64, dtype=torch.float16))
    cos = torch.zeros(8, 32)
    for kv, kw, match in ((torch.zeros(2, 128, ROW, dtype=torch.float16), {}, "576"), (torch.zeros(2, 128, 576, dtype=torch.uint8), {}, "656"),
                          (c8.view(torch.float8_e4m3fn)[..., :576], {}, "656"), (c8.view(torch.float8_e5m2), {}, "e5m2"),
                          (c8.view(torch.float8_e4m3fnuz), {}, "fnuz"), (c8, new, "quantising append is not served yet"),
                          (c8.view(torch.float8_e4m3fn), dict(new, rotary_cos=cos, rotary_sin=cos), "quantising append is not served yet"),
                          (c8, dict(rotary_cos=cos, rotary_sin=cos), "quantising append is not served yet")):
        with pytest.raises(ValueError, match=match):
            f(q, kv, lens, **kw)
    for kv in (c8, c8.view(torch.float8_e4m3fn), c8.unsqueeze(2)):                        # every check passed: CPU tensors stop at the device check
        with pytest.raises(RuntimeError, match="ROCm device"):
            f(q, kv, lens)
    rec = dc.recording_lib(monkeypatch)                                                   # CPU tensors claim a device; the library is a recorder
    with pytest.raises(ValueError, match="multiples of 16"):                             # a view the kernel cannot address raises: never copied
        f(q, torch.zeros(2, 128, ROW + 8, dtype=torch.uint8)[..., :ROW], lens)
    pool, bt, idx = torch.zeros(6, 64, 672, dtype=torch.uint8)[..., :ROW], torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 1, 8, dtype=torch.int32)
    f(q, pool.view(torch.float8_e4m3fn), lens, block_table=bt, num_splits=3)
    f(q, pool.unsqueeze(2), lens, block_table=bt, indices=idx)
    (_, (n1, a1), _, (n2, a2)) = rec.calls                                                # (each call asks the twin's workspace query first)
    assert [c[0] for c in rec.calls[0::2]] == ["fa2_fwd_decode_mla_workspace_bytes", "fa2_fwd_decode_mla_sparse_workspace_bytes"]
    assert (n1, n2, len(a1), len(a2)) == ("fa2_fwd_decode_mla_fp8", "fa2_fwd_decode_mla_sparse_fp8", 25, 28)
    for a in (a1, a2):                                                                    # the view itself, strides in bytes
        got = dict(zip(dc.ENTRIES["mla"][1], a))
        assert got["k"] == pool.data_ptr() and tuple(got["ks"])[0::2] == (64 * 672, 672) and (got["cap"], got["page"], got["pages"]) == (3, 64, 6)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_helpers_against_the_contract_in_float64(dtype):
    g = torch.Generator().manual_seed(3)
    x = torch.randn((3, 5, 576), generator=g) * torch.tensor([1.0, 4.0, 0.25, 16.0, 1.0]).repeat_interleave(128)[:576]
    x[0, 1, 128:256] = 0.0                                                                # an all-zero group: scale 1
    x = x.to(dtype)
    c = FlashAttn.mla_cache_to_fp8(x)
    assert c.dtype == torch.uint8 and tuple(c.shape) == (3, 5, ROW) and FlashAttn.mla_cache_to_fp8 is __import__("rocwmma_fattn").mla_cache_to_fp8
    xs = x[..., :512].double().reshape(3, 5, 4, 128)
    scale = c[..., 512:528].contiguous().view(torch.float32)
    amax = xs.abs().amax(-1)
    assert torch.equal(scale, torch.where(amax > 0, amax.float() / 448.0, torch.ones(()))) and scale[0, 1, 1] == 1.0
    codes = c[..., :512].contiguous().view(torch.float8_e4m3fn)
    assert torch.equal(codes.view(torch.uint8), (xs.float() / scale[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).reshape(3, 5, 512))
    assert torch.equal(c[..., 528:].contiguous().view(dtype), x[..., 512:])
    # the contract, straight line: the product of a 4-bit and a 24-bit significand is exact in float64; the f32 multiply rounds it once, the I/O dtype once
    want = (codes.double().reshape(3, 5, 4, 128) * scale.double()[..., None]).float().to(dtype).reshape(3, 5, 512)
    for cache in (c, c.view(torch.float8_e4m3fn)):
        back = FlashAttn.mla_cache_from_fp8(cache, dtype)
        assert back.dtype == dtype and torch.equal(back[..., :512].view(torch.int16), want.view(torch.int16)) and torch.equal(back[..., 512:], x[..., 512:])
    # e4m3 keeps 3 fraction bits (half an ulp: 2^-4 relative; below the normals 2^-10 of the scale), then the I/O dtype rounds once more (bf16: 2^-9)
    err, ref = (back[..., :512].double() - x[..., :512].double()).abs().reshape(3, 5, 4, 128), xs.abs()
    assert bool((err <= ref * (2.0 ** -4 + 2.0 ** -8) + scale.double()[..., None] * 2.0 ** -10).all()) and bool(torch.isfinite(back).all())


def test_no_kernel_of_the_new_units_has_a_private_segment():
    build, found = _fa2_lib._build_module(), {}
    units = [u for u in build.UNITS if u[1] in ("decode_mla_fp8_hip.cpp", "decode_mla_sparse_fp8_hip.cpp")]
    assert len(units) == 4 and {"fa2_decode_mla_sweep.h", "fa2_decode_mla_sparse_sweep.h"} <= set(build.HEADERS)

    def asm(u):
        cmd = [build._hipcc()] + [f for f in build.HIPCC_FLAGS if f != "--offload-compress"] + list(u[2]) + ["-I", build.INCLUDE, "-I", build.CSRC]
        return subprocess.run(cmd + ["--cuda-device-only", "-S", build.CSRC + "/" + u[1], "-o", "-"], capture_output=True, text=True, check=True).stdout
    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        texts = list(ex.map(asm, units))
    for u, text in zip(units, texts):
        for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
            found[u[0], name] = [int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1)) for k in ("private_segment_fixed_size", "uses_dynamic_stack")]
    names = [n for _, n in found]
    assert len(found) == 8 and sum("decode_mla_fp8_kernel" in n for n in names) == 2 and sum("decode_mla_sparse_fp8_kernel" in n for n in names) == 2, sorted(found)
    assert all(v == [0, 0] for v in found.values()), found
