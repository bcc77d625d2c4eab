"""CPU tests of the quantising append for an e4m3 latent (MLA) cache of 656-byte rows (include/fa2_gfx950.h: fa2_kvcache_append_mla_fp8,
fa2_kvcache_append_mla_varlen_fp8; kvcache_append_mla / kvcache_append_mla_varlen on a uint8 / float8_e4m3fn cache): the symbols, the new refusals in
their place, the operator's argument checks and the calls it makes through a stand-in library, the private segment of the new unit's kernels and the
sanitizer run of the kernel's addressing as a stand-alone program.  Nothing here touches a device."""
import concurrent.futures
import os
import re
import shutil
import subprocess

import pytest
import torch

import decode_calls as dc
from conftest import PKG, ROOT
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import kvcache_append_mla, kvcache_append_mla_varlen
from test_kvappend_mla import ALIGN, BF16, COS, F32, HEAD_DIM, HEADER, NULLP, OK, PACKED, SHAPE, SIN, UNIFORM, _plain

P = dc.HOST
ROW = 656
TWIN = {"fa2_kvcache_append_mla_fp8": ("append_mla", UNIFORM), "fa2_kvcache_append_mla_varlen_fp8": ("append_mla_varlen", PACKED)}


def ks(row):
    return _fa2_lib.strides3(256 * row, ROW, row)


def _call(name, **kw):
    """The entry on host memory that is never touched: its twin's well-formed call with 656-byte rows, `kw` laid over it"""
    entry, defaults = TWIN[name]
    return getattr(_fa2_lib.load(), name)(*dc.c_args(entry, **dict(dict(defaults, ks=ks(ROW), stream=None), **kw)))


@pytest.mark.parametrize("name", sorted(TWIN))
def test_symbols_and_the_new_refusals_in_their_place(name):
    assert name + "(" in open(HEADER).read() and getattr(_fa2_lib.load(), name).argtypes == _fa2_lib.SYMBOLS[name][1] == _fa2_lib.SYMBOLS[name[:-4]][1]
    big = dict(total=2 ** 31) if "varlen" in name else dict(B=65536, N=32768)        # well-formed but for the grid: 656-byte rows pass every check
    assert _call(name, **big) == -7 and _call(name, ks=ks(672), **big) == -7
    for row in (640, 664, 0, -656):                                                   # below 656; no multiple of 16
        assert _call(name, ks=ks(row)) == SHAPE and _call(name, ks=ks(row), k=P + 8, dtype=2) == SHAPE, row
        assert _call(name, ks=ks(row), D=512) == HEAD_DIM, row                        # ... after the head dim
    assert _call(name, k=P + 8) == ALIGN and _call(name, k=P + 8, dtype=2) == ALIGN   # the base: before the dtype
    assert _call(name, ks=_fa2_lib.strides3(8, ROW, ROW)) == ALIGN                    # a batch stride of 8 bytes
    assert _call(name, k=None) == NULLP and _call(name, k=None, ks=ks(640)) == NULLP
    if "varlen" in name:
        assert _call(name, total=0) == OK and _call(name, total=0, ks=ks(640)) == SHAPE


def test_operator_argument_checks_and_the_calls_it_makes(monkeypatch):
    dt = torch.bfloat16
    proj = torch.zeros(2, 3, 584, dtype=dt)
    kv_c, k_pe, q = proj[..., :512], proj[..., 512:576], torch.zeros(2, 3, 16, 576, dtype=dt)
    lens, bt = torch.tensor([70, 100], dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32)
    c8 = torch.zeros(6, 64, ROW, dtype=torch.uint8)
    for kv, match in ((torch.zeros(6, 64, 576, dtype=torch.uint8), "656"), (c8.view(torch.float8_e4m3fn)[..., :576], "656"), (c8.view(torch.float8_e5m2), "e5m2"),
                      (c8.view(torch.float8_e4m3fnuz), "fnuz"), (torch.zeros(6, 64, ROW, dtype=dt), "576")):
        with pytest.raises(ValueError, match=match):
            kvcache_append_mla(kv, kv_c, k_pe, lens, bt)
    with pytest.raises(ValueError, match="656"):
        kvcache_append_mla_varlen(c8[..., :640], kv_c[0], k_pe[0], torch.tensor([0, 1, 3], dtype=torch.int32), lens, bt)
    with pytest.raises(ValueError):                                                   # kv_c stays fp16 / bf16
        kvcache_append_mla(c8, kv_c.float(), k_pe.float(), lens, bt)
    for kv in (c8, c8.view(torch.float8_e4m3fn), c8.unsqueeze(2)):                    # every check passed: CPU tensors stop at the device check
        with pytest.raises(RuntimeError, match="ROCm device"):
            kvcache_append_mla(kv, kv_c, k_pe, lens, bt)
    rec = dc.recording_lib(monkeypatch)
    with pytest.raises(ValueError, match="multiples of 16"):                         # a view the kernel cannot address raises: never copied
        kvcache_append_mla(torch.zeros(6, 64, ROW + 8, dtype=torch.uint8)[..., :ROW], kv_c, k_pe, lens, bt)
    assert rec.calls == []
    pool = torch.zeros(6, 64, 672, dtype=torch.uint8)[..., :ROW]                      # a strided byte view: uncopied, strides in bytes
    q_out = kvcache_append_mla(pool.view(torch.float8_e4m3fn), kv_c, k_pe, lens, bt, rotary_cos=COS, rotary_sin=SIN, rotary_interleaved=False, q=q)
    kvcache_append_mla_varlen(pool.unsqueeze(2), kv_c[0], k_pe[0], torch.tensor([0, 1, 3], dtype=torch.int32), lens, bt)
    (n1, a1), (n2, a2) = rec.calls
    assert (n1, n2, len(a1), len(a2)) == ("fa2_kvcache_append_mla_fp8", "fa2_kvcache_append_mla_varlen_fp8", 31, 31)
    got = dict(zip(dc.ENTRIES["append_mla"][1], _plain(a1)))
    assert (got["dtype"], got["kn"], got["vn"], got["k"], got["ks"], got["cap"], got["page"], got["pages"], got["kns"], got["D"], got["Dv"]) == \
        (BF16, kv_c.data_ptr(), k_pe.data_ptr(), pool.data_ptr(), (64 * 672, ROW, 672), 3, 64, 6, (3 * 584, 584), 576, 512)
    assert (got["q"], got["qo"], got["H"], got["Nq"], got["rdt"], got["rot"], got["inter"]) == (q.data_ptr(), q_out.data_ptr(), 16, 3, F32, 64, 0)
    got = dict(zip(dc.ENTRIES["append_mla_varlen"][1], _plain(a2)))
    assert (got["k"], got["ks"], got["total"], got["kns"], got["q"]) == (pool.data_ptr(), (64 * 672, ROW, 672), 3, (584,), None)
    del rec.calls[:]
    pool16 = torch.zeros(6, 64, 584, dtype=dt)[..., :576]                             # a 16-bit cache: the old entry, the old arguments
    kvcache_append_mla(pool16, kv_c, k_pe, lens, bt)
    (name, args), = rec.calls
    got = dict(zip(dc.ENTRIES["append_mla"][1], _plain(args)))
    assert name == "fa2_kvcache_append_mla" and len(args) == 31 and (got["k"], got["ks"]) == (pool16.data_ptr(), (64 * 584, 576, 584))


def test_no_kernel_of_the_new_unit_has_a_private_segment():
    build, found = _fa2_lib._build_module(), {}
    units = [u for u in build.UNITS if u[1] == "kvappend_mla_fp8_hip.cpp"]
    assert len(units) == 2 and all("-fhonor-nans" in u[2] for u in units) and "fa2_kvappend_mla_fp8.hip.h" in build.HEADERS

    def asm(u):
        cmd = [build._hipcc()] + [f for f in build.HIPCC_FLAGS if f != "--offload-compress"] + list(u[2]) + ["-I", build.INCLUDE, "-I", build.CSRC]
        return subprocess.run(cmd + ["--cuda-device-only", "-S", build.CSRC + "/" + u[1], "-o", "-"], capture_output=True, text=True, check=True).stdout
    with concurrent.futures.ThreadPoolExecutor(2) as ex:
        texts = list(ex.map(asm, units))
    for u, text in zip(units, texts):
        for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
            found[u[0], name] = [int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1)) for k in ("private_segment_fixed_size", "uses_dynamic_stack", "group_segment_fixed_size")]
    names = [n for _, n in found]
    assert len(found) == 4 and sum("kvappend_mla_fp8_kernel" in n for n in names) == 2 and sum("kvappend_mla_varlen_fp8_kernel" in n for n in names) == 2, sorted(found)
    assert all(v == [0, 0, 0] for v in found.values()), found                        # no scratch, no dynamic stack, no LDS


def test_the_addressing_under_asan_and_ubsan(tmp_path):
    """tools/kvappend_mla_fp8_sanitize.cpp: a stand-alone program with its own main that walks every lane of every group through the functions the kernels
    call, on sources and a byte cache allocated to the byte, with hostile lengths, tables and cu_seqlens."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the host program cannot be compiled")
    exe = str(tmp_path / "kvappend_mla_fp8_sanitize")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(PKG, "csrc"), "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "kvappend_mla_fp8_sanitize.cpp"), "-o", exe], check=True, capture_output=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok:"), (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
