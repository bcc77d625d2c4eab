"""CPU tests of decode attention on a latent (MLA) KV cache (include/fa2_gfx950.h: fa2_fwd_decode_mla and its queries): the symbols, the plan and the
workspace size, every validation code and the order they are checked in on host memory that is never touched, the argument checks of
flash_attention_decode_mla, the tile / part arithmetic the kernel and the host share against brute force, the power of the check the GPU tests use
(float64 mutants of the formula must fail it while the oracle passes), the sanitizer run of that arithmetic as a stand-alone program, and the
private segment of the new unit's kernels.  Nothing here touches a device."""
import concurrent.futures
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import pytest
import torch

import decode_calls as dc
import decode_refs as dr
import mla_refs as mr
from conftest import PKG, ROOT
from rocwmma_fattn import FlashAttn, _fa2_lib

HEADER = os.path.join(ROOT, "include", "fa2_gfx950.h")
MLA_SYMBOLS = ("fa2_fwd_decode_mla", "fa2_fwd_decode_mla_plan", "fa2_fwd_decode_mla_workspace_bytes", "fa2_decode_mla_part_range", "fa2_decode_mla_tile")
OK, NULLP, SHAPE, HEAD_DIM, ALIGN, DTYPE, SCALE, GRID = 0, -1, -2, -3, -4, -5, -6, -7
F16, BF16 = _fa2_lib.FA2_DTYPE_F16, _fa2_lib.FA2_DTYPE_BF16
TILE, BLOCK, MAX_SPLIT, MIN_PART = 32, 64, 128, 8


def test_symbols_are_declared_exported_and_bound_and_the_operator_is_public():
    lib = _fa2_lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in MLA_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _fa2_lib.SYMBOLS, name
        assert getattr(lib, name).argtypes == _fa2_lib.SYMBOLS[name][1]
    assert re.search(r"FA2_KERNEL_HIP_DECODE_MLA\s*=\s*%d\b" % _fa2_lib.FA2_KERNEL_HIP_DECODE_MLA, text)
    assert callable(FlashAttn.flash_attention_decode_mla) and "flash_attention_decode_mla" in FlashAttn.__all__
    assert dc.ENTRIES["mla"][0] == "fa2_fwd_decode_mla" and len(dc.ENTRIES["mla"][1]) == len(_fa2_lib.SYMBOLS["fa2_fwd_decode_mla"][1]) == 25


# ---------------------------------------------------------------------------------------------------------------- plan and workspace
def _ws(dt, B, H, Nq, cap, page=0, ns=0, D=576, Dv=512):
    return _fa2_lib.load().fa2_fwd_decode_mla_workspace_bytes(dt, B, H, Nq, D, Dv, cap, page, ns)


def test_plan_and_workspace():
    """Without a device the library counts 256 CUs (an MI355X's): a workgroup fills a CU, so split = min(256 / (B * row blocks), 128, capacity tiles / 8)."""
    for (B, H, Nq, cap, page) in ((1, 128, 1, 8192, 0), (32, 128, 1, 4096, 0), (32, 16, 1, 4096, 0), (8, 128, 2, 8192, 0), (1, 16, 1, 300, 0), (3, 5, 3, 4, 128),
                                  (1, 1, 1, 1, 0), (2, 13, 5, 70000, 0), (256, 16, 1, 4096, 0), (1, 16, 1, 1 << 20, 0)):
        for dt in (F16, BF16):
            a = _fa2_lib.decode_mla_plan(dt, B, H, Nq, cap, page).as_dict()
            assert a == _fa2_lib.decode_mla_plan(dt, B, H, Nq, cap, page).as_dict()
            rows, keys = Nq * H, cap * page if page else cap
            blocks = -(-rows // BLOCK)
            assert a["kernel"] == _fa2_lib.FA2_KERNEL_HIP_DECODE_MLA and a["key_tile"] == TILE and a["row_blocks"] == blocks and a["max_split"] == MAX_SPLIT
            want = 1 if B * blocks >= 256 else max(1, min(256 // (B * blocks), MAX_SPLIT, -(-keys // TILE) // MIN_PART))
            assert a["nsplit"] == want, (B, H, Nq, cap, page, a)
            assert _ws(dt, B, H, Nq, cap, page) == (0 if want == 1 else B * want * rows * 513 * 4)
            for ns in (1, 2, 3, 16, 17, MAX_SPLIT):
                f = _fa2_lib.decode_mla_plan(dt, B, H, Nq, cap, page, ns).as_dict()
                assert f["nsplit"] == ns and f["row_blocks"] == blocks
                assert _ws(dt, B, H, Nq, cap, page, ns) == (0 if ns == 1 else B * ns * rows * 513 * 4)
    # the B = 1 call on all 128 heads reaches every CU where decode's cap of 16 would stop at 32
    assert _fa2_lib.decode_mla_plan(BF16, 1, 128, 1, 1 << 20).nsplit * 2 == 256
    # arguments the call would refuse: no workspace
    assert _ws(F16, 1, 129, 1, 256) == 0 and _ws(F16, 1, 16, 1, 256, D=512) == 0 and _ws(F16, 1, 16, 1, 4, page=48) == 0 and _ws(F16, 1, 16, 1, 256, ns=129) == 0


def test_plan_argument_codes():
    lib = _fa2_lib.load()
    plan = _fa2_lib.DecodeMlaPlan()
    ok = dict(dt=F16, B=1, H=16, Nq=1, D=576, Dv=512, cap=256, page=0, ns=0)

    def rc(**kw):
        a = dict(ok, **kw)
        return lib.fa2_fwd_decode_mla_plan(a["dt"], a["B"], a["H"], a["Nq"], a["D"], a["Dv"], a["cap"], a["page"], a["ns"], ctypes.byref(plan))
    assert rc() == OK
    assert lib.fa2_fwd_decode_mla_plan(F16, 1, 16, 1, 576, 512, 256, 0, 0, None) == NULLP
    for kw in (dict(B=0), dict(H=0), dict(H=129), dict(Nq=0), dict(H=128, Nq=5), dict(H=103, Nq=5), dict(cap=0), dict(page=48, cap=4), dict(page=-64), dict(ns=-1),
               dict(ns=MAX_SPLIT + 1), dict(D=0)):
        assert rc(**kw) == SHAPE, kw
    for kw in (dict(D=512), dict(D=584), dict(Dv=576), dict(Dv=256), dict(D=128, Dv=128)):
        assert rc(**kw) == HEAD_DIM, kw
    assert rc(dt=2) == DTYPE and rc(dt=-1) == DTYPE
    assert rc(H=129, D=512) == SHAPE and rc(D=512, dt=7) == HEAD_DIM             # sizes before the head dim before the dtype
    assert rc(H=128, Nq=4) == OK and rc(H=102, Nq=5) == OK


# ---------------------------------------------------------------------------------------------------------------- the entry's codes and their order
P = dc.HOST                                  # 16-byte aligned host memory that no call here ever touches
DEFAULTS = dict(dtype=F16, q=P, k=P, o=P, lse=P, lens=P, bt=None, B=2, H=16, Nq=1, D=576, Dv=512, cap=256, page=0, pages=0,
                qs=_fa2_lib.strides3(16 * 576, 576, 16 * 576), ks=_fa2_lib.strides3(256 * 576, 576, 576), os=_fa2_lib.strides3(16 * 512, 512, 16 * 512),
                ls=_fa2_lib.strides2(16, 1), bts=0, scale=0.1, ns=1, ws=None, wsb=0)
BAD_ALIGN, BAD_SCALE = _fa2_lib.strides3(256 * 576, 576, 580), float("nan")


def _call(**kw):
    """fa2_fwd_decode_mla on host memory that is never touched: every call here is refused before the launch."""
    return dc.host_call("mla", DEFAULTS, **kw)


def test_every_error_code():
    for n in ("q", "k", "o", "lse", "lens", "qs", "ks", "os", "ls"):
        assert _call(**{n: None}) == NULLP, n
    assert _call(page=64, cap=4, pages=3, bt=None) == NULLP                       # a paged call needs its block table
    for kw in (dict(B=0), dict(H=0), dict(H=129), dict(Nq=0), dict(Nq=33), dict(cap=0), dict(page=48, bt=P, pages=2), dict(page=-64), dict(ns=-1), dict(ns=129),
               dict(page=64, cap=4, bt=P, pages=0), dict(ls=_fa2_lib.strides2(-1, 1)), dict(page=64, bt=P, pages=2, cap=(1 << 31) // 64)):
        assert _call(**kw) == SHAPE, kw
    for kw in (dict(D=512), dict(D=640), dict(Dv=576), dict(D=128, Dv=128)):
        assert _call(**kw) == HEAD_DIM, kw
    for kw in (dict(q=P + 8), dict(k=P + 2), dict(o=P + 4), dict(lse=P + 2), dict(lens=P + 1), dict(ks=BAD_ALIGN), dict(qs=_fa2_lib.strides3(1, 576, 4)),
               dict(os=_fa2_lib.strides3(7, 512, 512)), dict(ks=_fa2_lib.strides3(256 * 576, 576, 0)), dict(page=64, cap=4, pages=2, bt=P + 2), dict(bts=-1)):
        assert _call(**kw) == ALIGN, kw
    assert _call(dtype=2) == DTYPE and _call(dtype=9) == DTYPE
    assert _call(scale=BAD_SCALE) == SCALE and _call(scale=float("inf")) == SCALE
    assert _call(B=65536) == GRID
    assert _call(ns=2) == NULLP and _call(ns=2, ws=P + 4, wsb=1 << 30) == ALIGN           # the workspace: null, alignment, size
    need = _ws(F16, 2, 16, 1, 256, ns=2)
    assert need == 2 * 2 * 16 * 513 * 4 and _call(ns=2, ws=P, wsb=need - 1) == SHAPE


def test_the_order_of_the_codes():
    assert _call(q=None, H=129, D=512, ks=BAD_ALIGN, dtype=2) == NULLP
    assert _call(H=129, D=512, ks=BAD_ALIGN, dtype=2, scale=BAD_SCALE) == SHAPE
    assert _call(ns=129, D=512) == SHAPE and _call(page=48, bt=P, pages=2, D=512) == SHAPE and _call(Nq=33, Dv=500) == SHAPE     # rows, paging, split: before the head dim
    assert _call(D=512, ks=BAD_ALIGN, dtype=2, scale=BAD_SCALE) == HEAD_DIM
    assert _call(ks=BAD_ALIGN, dtype=2, scale=BAD_SCALE, B=65536) == ALIGN
    assert _call(dtype=2, scale=BAD_SCALE, B=65536) == DTYPE
    assert _call(scale=BAD_SCALE, B=65536, ns=2) == SCALE
    assert _call(B=65536, ns=2) == GRID


# ---------------------------------------------------------------------------------------------------------------- the operator's argument checks
def _tensors(B=2, Nq=1, H=16, nmax=128, dtype=torch.float16, D=576):
    return torch.zeros(B, Nq, H, D, dtype=dtype), torch.zeros(B, nmax, D, dtype=dtype), torch.full((B,), 5, dtype=torch.int32)


def test_python_argument_checks():
    f = FlashAttn.flash_attention_decode_mla
    q, kv, lens = _tensors()
    bad = [
        (_tensors(D=512)[0], kv, lens, {}),                                            # wrong widths
        (q, _tensors(D=512)[1], lens, {}),
        (q, torch.zeros(2, 128, 640, dtype=torch.float16), lens, {}),
        (q, kv, lens, dict(head_dim_v=576)), (q, kv, lens, dict(head_dim_v=256)), (q, kv, lens, dict(head_dim_v=True)),
        (_tensors(H=129)[0], kv, lens, {}),                                            # H > 128
        (_tensors(Nq=5, H=128)[0], kv, lens, {}), (_tensors(Nq=33)[0], kv, lens, {}),  # Nq * H > 512
        (q, kv.bfloat16(), lens, {}), (q.float(), kv.float(), lens, {}),               # dtypes
        (q, torch.zeros(6, 48, 576, dtype=torch.float16), lens, dict(block_table=torch.zeros(2, 3, dtype=torch.int32))),      # page size 48
        (q, torch.zeros(6, 64, 576, dtype=torch.float16), lens, dict(block_table=torch.zeros(2, 3, dtype=torch.int64))),
        (q, torch.zeros(6, 64, 576, dtype=torch.float16), lens, dict(block_table=torch.zeros(3, 3, dtype=torch.int32))),
        (q, kv, lens.long(), {}), (q, kv, lens[:1], {}),                               # int64 lengths, a wrong count
        (q, kv[:1], lens, {}),                                                         # a contiguous cache of another batch
        (q, kv.unsqueeze(2).expand(2, 128, 2, 576), lens, {}),                         # a head axis that is not 1
        (q[0], kv, lens, {}), (q, kv[0], lens, {}),
        (q, kv, lens, dict(num_splits=129)), (q, kv, lens, dict(num_splits=-1)), (q, kv, lens, dict(num_splits=1.0)), (q, kv, lens, dict(num_splits=True)),
    ]
    for qq, kk, ll, kw in bad:
        with pytest.raises(ValueError):
            f(qq, kk, ll, **kw)
    for t in (q, kv):                                                                  # inference only
        r = t.clone().requires_grad_(True)
        with pytest.raises(ValueError, match="inference only"):
            f(r if t is q else q, r if t is kv else kv, lens)
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm device"):            # ... under no_grad the call goes on, to the device check
        f(q.clone().requires_grad_(True), kv, lens)
    with pytest.raises(RuntimeError, match="ROCm device"):                             # every check above passed: CPU tensors stop at the device check
        f(q, kv.unsqueeze(2), lens)


def test_the_operator_hands_the_entry_what_the_tensors_say(monkeypatch):
    """CPU tensors under the recording library: a strided cache view and its block table reach fa2_fwd_decode_mla as they are (never copied), a q that
    cannot be addressed is copied, the default scale is 576 ** -0.5."""
    rec = dc.recording_lib(monkeypatch)
    big = torch.zeros(6, 64, 640, dtype=torch.bfloat16)
    pool = big[:, :, 32:608]
    q = torch.zeros(2, 2, 16, 580, dtype=torch.bfloat16)[..., :576]                    # row stride 580: no multiple of 8 -> copied
    lens = torch.tensor([3, 70], dtype=torch.int32)
    bt = torch.zeros(2, 4, dtype=torch.int32)[:, :3]
    o = FlashAttn.flash_attention_decode_mla(q, pool, lens, block_table=bt, num_splits=3)
    (qname, qargs), (name, args) = rec.calls
    assert qname == "fa2_fwd_decode_mla_workspace_bytes" and qargs == (BF16, 2, 16, 2, 576, 512, 3, 64, 3)
    got = dict(zip(dc.ENTRIES["mla"][1], args))
    assert name == "fa2_fwd_decode_mla" and len(args) == 25
    assert got["k"] == pool.data_ptr() and tuple(got["ks"])[0::2] == (64 * 640, 640) and got["q"] not in (q.data_ptr(), None)
    assert tuple(got["qs"]) == (2 * 16 * 576, 576, 16 * 576) and tuple(got["os"]) == (2 * 16 * 512, 512, 16 * 512) and tuple(got["ls"]) == (32, 2)
    assert (got["B"], got["H"], got["Nq"], got["D"], got["Dv"], got["cap"], got["page"], got["pages"], got["bts"], got["ns"]) == (2, 16, 2, 576, 512, 3, 64, 6, 4, 3)
    assert got["bt"] == bt.data_ptr() and got["lens"] == lens.data_ptr() and got["o"] == o.data_ptr() and tuple(o.shape) == (2, 2, 16, 512)
    assert got["scale"] == 576 ** -0.5 and isinstance(got["scale"], float)


# ---------------------------------------------------------------------------------------------------------------- the shared arithmetic against brute force
def test_tile_and_part_arithmetic_exhaustive():
    """Small (len, capacity, page, nsplit, part), lengths below 0 and above the capacity included: the tiles of all parts of a split, walked through
    fa2_decode_mla_tile, name every key of [0, clamp(len)) once — at the block-table slot and row where a brute-force walk over the keys finds it."""
    pr, tl = _fa2_lib.decode_mla_part_range, _fa2_lib.decode_mla_tile
    for capacity, page in ((1, 0), (31, 0), (32, 0), (33, 0), (100, 0), (1, 64), (3, 64), (2, 128)):
        keys = capacity * page if page else capacity
        ntiles = -(-keys // TILE)
        for length in sorted({-70, -1, 0, 1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, keys - 1, keys, keys + 1, keys + 1000, 2 ** 40}):
            n = min(max(length, 0), keys)
            where = {}
            for t in range(ntiles):
                slot, row, rows = tl(length, capacity, page, t)
                assert rows == min(max(n - t * TILE, 0), TILE), (capacity, page, length, t)
                for kk in range(rows):
                    where[t * TILE + kk] = (slot, row + kk)
            assert where == {j: ((j // page, j % page) if page else (0, j)) for j in range(n)}, (capacity, page, length)
            for nsplit in (1, 2, 3, 5, 16, 17, MAX_SPLIT):
                tiles, per, nxt = -(-n // TILE), -(-(-(-n // TILE)) // nsplit), 0
                for part in range(nsplit):
                    first, cnt = pr(length, keys, nsplit, part)
                    assert 0 <= cnt <= per
                    if cnt:
                        assert first == nxt == part * per, (capacity, page, length, nsplit, part)
                        assert all(tl(length, capacity, page, t)[2] >= 1 for t in range(first, first + cnt))      # every tile of a part holds a key
                        nxt = first + cnt
                    else:
                        assert part * per >= tiles
                assert nxt == tiles, (capacity, page, length, nsplit)


def test_tile_and_part_argument_codes():
    lib = _fa2_lib.load()
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ra, rb, rc = ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)
    assert lib.fa2_decode_mla_part_range(100, 200, 2, 0, None, rb) == NULLP and lib.fa2_decode_mla_part_range(100, 200, 2, 0, ra, None) == NULLP
    for args in ((100, -1, 2, 0), (100, 200, 0, 0), (100, 200, MAX_SPLIT + 1, 0), (100, 200, 2, 2), (100, 200, 2, -1), (100, 2 ** 31, 2, 0)):
        assert lib.fa2_decode_mla_part_range(*args, ra, rb) == SHAPE, args
    assert lib.fa2_decode_mla_part_range(100, 200, MAX_SPLIT, MAX_SPLIT - 1, ra, rb) == OK
    assert lib.fa2_decode_mla_tile(5, 100, 0, 0, None, rb, rc) == NULLP
    for args in ((5, 0, 0, 0), (5, 4, 48, 0), (5, 100, 0, 4), (5, 100, 0, -1), (5, 2, 64, 4), (5, (1 << 31) // 64, 64, 0)):
        assert lib.fa2_decode_mla_tile(*args, ra, rb, rc) == SHAPE, args
    assert lib.fa2_decode_mla_tile(5, 100, 0, 3, ra, rb, rc) == OK and (a.value, b.value, c.value) == (0, 96, 0)


# ---------------------------------------------------------------------------------------------------------------- the power of the check
MUTANTS = (("k512", 1), ("v64", 1), ("rowmap", 1), ("dropkey", 1), ("diag", 1), ("norescale", 2))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_the_check_refuses_every_mutant_and_passes_the_oracle(dtype):
    """On the N(0, 1) cases the bars were derived on: float64 of the formula and the oracle's own result pass decode_refs.check; each mutant of the
    float64 formula fails it on every case the mutation can show in (a row map needs Nq > 1 and H > 1, the diagonal Nq > 1)."""
    code = dc.code(dtype)
    applies = {"rowmap": lambda H, Nq: Nq > 1 and H > 1, "diag": lambda H, Nq: Nq > 1}
    failed = {m: 0 for m, _ in MUTANTS}
    for seed, (H, Nq, n) in enumerate(mr.CPU_CASES):
        q, kv = mr.inputs(1, H, Nq, n + 5, [n], dtype, 100 + seed)
        refs = mr.refs(q, kv, [n], code)                                               # (asserts the oracle against float64 itself)
        tag = (H, Nq, n)
        dr.check(*mr.mla_f64(q, kv, [n]), refs, [n], code, tag)
        dr.check(*mr.mla_f64(q, kv, [n], parts=2), refs, [n], code, tag)
        o_ref, lse_ref = refs[0][0], refs[0][1]
        dr.check(torch.from_numpy(o_ref[0]).transpose(0, 1).unsqueeze(0), torch.from_numpy(lse_ref), refs, [n], code, tag)
        for m, parts in MUTANTS:
            if not applies.get(m, lambda H, Nq: True)(H, Nq):
                continue
            if m == "norescale" and n < 2:
                continue
            with pytest.raises(AssertionError):
                dr.check(*mr.mla_f64(q, kv, [n], mutant=m, parts=parts), refs, [n], code, tag + (m,))
            failed[m] += 1
    assert all(failed[m] >= 3 for m in failed), failed


# ---------------------------------------------------------------------------------------------------------------- sanitizers, on host code
def test_the_shared_arithmetic_under_asan_and_ubsan(tmp_path):
    """tools/decode_mla_tile_sanitize.cpp: a stand-alone program with its own main that walks the kernel's addressing over caches allocated to the byte."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the host program cannot be compiled")
    exe = str(tmp_path / "decode_mla_tile_sanitize")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(PKG, "csrc"), "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "decode_mla_tile_sanitize.cpp"), "-o", exe], check=True, capture_output=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok:"), (res.returncode, res.stdout[-2000:], res.stderr[-4000:])


# ---------------------------------------------------------------------------------------------------------------- the new unit, compiled
def test_no_kernel_of_the_new_unit_has_a_private_segment():
    """decode_mla_hip.cpp compiled for gfx950 with the product build's flags, both dtypes: four kernels (the sweep and the 512-wide combine, twice), none
    with scratch, none with a dynamic stack."""
    spec = importlib.util.spec_from_file_location("_fa2_build_mla", os.path.join(PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    units = [u for u in build.UNITS if u[1] == "decode_mla_hip.cpp"]
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
                           int(re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", body).group(1)))
    assert len(found) == 4 and sum("decode_mla_kernel" in n for n in found) == 2 and sum("decode_combine_kernelILi512" in n for n in found) == 2, sorted(found)
    assert all(v == (0, 0) for v in found.values()), found
