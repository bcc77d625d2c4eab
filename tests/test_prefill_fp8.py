"""Chunked prefill on e4m3 KV caches, without a device: the two new symbols, every error code of fa2_fwd_prefill_fp8 and their class order on host memory that
is never touched, the plan query against the 16-bit one, the operator's refusals, and the power of the float64 checker for descale mistakes — on the GPU
test's own inputs a reference that drops or misindexes a descale must fail prefill_calls.check_float64, and the true one must pass it."""
import ctypes
import os

import pytest
import torch

import decode_calls as dc
import prefill_calls as pc
import prefill_fp8_calls as p8
from conftest import ROOT
from rocwmma_fattn import FlashAttn, _fa2_lib

E4M3 = p8.E4M3


def test_symbols_are_declared_exported_and_bound_and_the_operator_is_public():
    lib = _fa2_lib.load()
    with open(os.path.join(ROOT, "include", "fa2_gfx950.h")) as f:
        header = f.read()
    for name in ("fa2_fwd_prefill_fp8", "fa2_fwd_prefill_fp8_plan"):
        assert "int %s(" % name in header, name
        assert name in _fa2_lib.SYMBOLS and getattr(lib, name) is not None
    assert "flash_attention_prefill_fp8" in FlashAttn.__all__ and callable(FlashAttn.flash_attention_prefill_fp8)
    assert "flash_attention_prefill" in FlashAttn.__all__


def test_plan_answers_as_the_16_bit_plan_up_to_head_dim_256():
    f16, bf16 = _fa2_lib.FA2_DTYPE_F16, _fa2_lib.FA2_DTYPE_BF16
    before = _fa2_lib.load().fa2_get_option(b"rows")
    try:
        for rows in (0, 128, 256):
            _fa2_lib.set_option("rows", rows)
            for shape in ((2, 4, 2, 300, 64, 8, 64), (2, 4, 2, 300, 80, 8, 64), (1, 2, 1, 256, 128, 64, 64), (8, 32, 8, 1024, 128, 64, 64), (2, 4, 2, 300, 256, 717, 0),
                          (3, 4, 1, 1, 144, 700, 0)):
                for dt in (f16, bf16):
                    assert _fa2_lib.prefill_fp8_plan(dt, *shape) == _fa2_lib.prefill_plan(dt, *shape), (rows, shape)
        plan = _fa2_lib.prefill_fp8_plan(f16, 2, 4, 2, 300, 128, 8, 64)
        assert (plan["kernel"], plan["contract"], plan["heads_main"]) == (_fa2_lib.FA2_KERNEL_HIP_PREFILL, 0, 8)
    finally:
        _fa2_lib.set_option("rows", before)
    lib = _fa2_lib.load()
    plan = _fa2_lib.FwdPlan()
    assert lib.fa2_fwd_prefill_fp8_plan(f16, 2, 4, 2, 300, 128, 8, 64, None) == -1
    # D = 72 (a multiple of 8, not of 16) and the head dims of the kernel that is not compiled (257 .. 512) are FA2_ERR_HEAD_DIM here and fine in the 16-bit call
    for D in (72, 264, 512):
        assert lib.fa2_fwd_prefill_fp8_plan(f16, 2, 4, 2, 300, D, 8, 64, ctypes.byref(plan)) == -3, D
        assert lib.fa2_fwd_prefill_plan(f16, 2, 4, 2, 300, D, 8, 64, ctypes.byref(plan)) == 0, D
    for bad, rc in ((dict(B=0), -2), (dict(Hkv=3), -2), (dict(page=96), -2), (dict(D=12), -3), (dict(D=520), -3), (dict(dtype=7), -5)):
        a = dict(dtype=f16, B=2, H=4, Hkv=2, max_q=300, D=128, capacity=8, page=64)
        a.update(bad)
        assert lib.fa2_fwd_prefill_fp8_plan(a["dtype"], a["B"], a["H"], a["Hkv"], a["max_q"], a["D"], a["capacity"], a["page"], ctypes.byref(plan)) == rc, bad


# ---------------------------------------------------------------------------------------------------------------- error codes on host memory
_HOST = ctypes.create_string_buffer(4096 + 16)
HOST = (ctypes.addressof(_HOST) + 15) & ~15          # 16-byte aligned host memory that no call here ever touches
NULL, BAD_SHAPE, HEAD_DIM, ALIGN, DTYPE, SCALE, GRID, SOFTCAP = -1, -2, -3, -4, -5, -6, -7, -10
S2, S3 = _fa2_lib.strides2, _fa2_lib.strides3


DEFAULTS = dict(dtype=_fa2_lib.FA2_DTYPE_F16, q=HOST, k=HOST, v=HOST, o=HOST, lse=HOST, cu=HOST, lens=HOST, bt=HOST, B=2, H=4, Hkv=2,
                max_q=300, D=128, cap=8, page=64, pages=20, qs=S2(128, 512), ks=S3(64 * 256, 128, 256), vs=S3(64 * 256, 128, 256), os=S2(128, 512),
                lss=1024, bts=8, scale=0.125, kd=HOST, vd=HOST + 64, ds=S2(2, 1), wl=-1, cap_=0.0, sl=None, st=0, stream=None)


def _call(**kw):
    return dc.host_call("prefill_fp8", DEFAULTS, **kw)


BAD = {      # one defect per class, in the order the classes are checked
    NULL: [dict(q=None), dict(k=None), dict(v=None), dict(o=None), dict(lse=None), dict(cu=None), dict(lens=None), dict(bt=None), dict(qs=None), dict(ks=None),
           dict(os=None), dict(ds=None), dict(ds=None, vd=None), dict(ds=None, kd=None)],
    BAD_SHAPE: [dict(B=0), dict(H=0), dict(Hkv=3), dict(max_q=0), dict(page=96), dict(page=-64), dict(cap=0), dict(pages=0), dict(wl=-2),
                dict(lss=-1), dict(st=-1), dict(cap=2 ** 25), dict(ds=S2(-2, 1)), dict(ds=S2(2, -1)),
                dict(ks=S3(16, 16, 2 ** 25)), dict(vs=S3(16, 16, 2 ** 25))],                  # one tile: 64 rows of 2^25 BYTES = 2^31
    HEAD_DIM: [dict(D=12), dict(D=72), dict(D=264), dict(D=512), dict(D=520)],
    ALIGN: [dict(q=HOST + 8), dict(k=HOST + 8), dict(v=HOST + 2), dict(o=HOST + 4), dict(lse=HOST + 2), dict(cu=HOST + 2), dict(lens=HOST + 1),
            dict(bt=HOST + 2), dict(sl=HOST + 2), dict(kd=HOST + 2), dict(vd=HOST + 1), dict(qs=S2(4, 512)), dict(ks=S3(64 * 256, 128, 8)),
            dict(vs=S3(64 * 256, 8, 256)), dict(ks=S3(64 * 256 + 8, 128, 256)), dict(os=S2(128, 0)), dict(bts=-8)],
    DTYPE: [dict(dtype=5), dict(dtype=_fa2_lib.FA2_DTYPE_F32)],
    SCALE: [dict(scale=float("nan")), dict(scale=float("inf"))],
    SOFTCAP: [dict(cap_=-1.0), dict(cap_=float("nan"))],
    GRID: [dict(B=2 ** 15, H=2 ** 15, Hkv=2 ** 15, max_q=2 ** 20)],
}
CLASSES = (NULL, BAD_SHAPE, HEAD_DIM, ALIGN, DTYPE, SCALE, SOFTCAP, GRID)


def test_every_error_code_is_returned():
    for rc, cases in BAD.items():
        for kw in cases:
            assert _call(**kw) == rc, kw
    # the contiguous layout takes no block table and no pool size; null descales need no stride pair
    assert _call(bt=None, page=0, cap=717, pages=0, q=None) == NULL
    assert _call(bt=None, page=0, cap=717, pages=0, D=72) == HEAD_DIM
    assert _call(kd=None, vd=None, ds=None, scale=float("nan")) == SCALE
    # the tile rule counts bytes: a row stride of 2^24 elements is 2^30 bytes per tile here (the 16-bit call refuses it), 2^25 is 2^31
    assert _call(ks=S3(16, 16, 2 ** 24), scale=float("nan")) == SCALE
    # the largest compiled head dim passes the head-dim class
    assert _call(D=256, qs=S2(256, 1024), os=S2(256, 1024), ks=S3(64 * 512, 256, 512), vs=S3(64 * 512, 256, 512), scale=float("nan")) == SCALE


def test_error_classes_are_checked_in_the_16_bit_calls_order():
    for i, first in enumerate(CLASSES):
        for later in CLASSES[i + 1:]:
            kw = dict(BAD[later][0])
            kw.update(BAD[first][0])
            if set(BAD[later][0]) & set(BAD[first][0]):
                continue
            assert _call(**kw) == first, (first, later, kw)
    # the descale cases sit where their kind is: a null stride pair before every size, a negative stride before the head dim, a misaligned descale after it
    assert _call(ds=None, B=0) == NULL and _call(ds=S2(-2, 1), D=72) == BAD_SHAPE and _call(kd=HOST + 2, D=72) == HEAD_DIM
    assert _call(kd=HOST + 2, dtype=5) == ALIGN


def test_the_16_bit_entry_still_refuses_an_e4m3_cache():
    assert dc.host_call("prefill", DEFAULTS, fmt=_fa2_lib.FA2_CACHE_E4M3, kd=None, vd=None, ds=None) == DTYPE


# ---------------------------------------------------------------------------------------------------------------- the operator
def _op_args(dtype=torch.float16, page=64, D=64, cache=E4M3):
    q = torch.zeros(10, 4, D, dtype=dtype)
    kc = torch.zeros(6, page, 2, D, dtype=dtype).to(cache)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    lens = torch.tensor([70, 100], dtype=torch.int32)
    bt = torch.zeros(2, 3, dtype=torch.int32)
    return q, kc, kc.clone(), cu, lens, bt


def test_operator_refuses_before_any_device_work():
    prefill = FlashAttn.flash_attention_prefill_fp8
    q, kc, vc, cu, lens, bt = _op_args()
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="flash_attention_prefill_fp8 serves float8_e4m3fn caches only"):
            prefill(*_op_args(dtype=dt, cache=dt))
    for name in ("float8_e5m2", "float8_e4m3fnuz", "float8_e5m2fnuz"):
        other = getattr(torch, name, None)
        if other is not None:
            with pytest.raises(ValueError, match="e5m2 and the fnuz formats are not served"):
                prefill(*_op_args(cache=other))
    with pytest.raises(ValueError, match="one dtype"):
        prefill(q, kc, vc.to(torch.float16), cu, lens, bt)
    with pytest.raises(ValueError, match="multiples of 16 up to 256.*got 72"):
        prefill(*_op_args(D=72))
    with pytest.raises(ValueError, match="multiples of 16 up to 256.*got 512"):
        prefill(*_op_args(D=512))
    for bad in (torch.ones(2, 3), torch.ones(3, 2), torch.ones(2, 2, dtype=torch.float64), torch.ones(2, 2, dtype=torch.float16), 1.0):
        for key in ("k_descale", "v_descale"):
            with pytest.raises(ValueError, match=r"k_descale / v_descale must be float32 tensors of shape \[B, Hkv\] = \[2, 2\]"):
                prefill(q, kc, vc, cu, lens, bt, **{key: bad})
    table = torch.zeros(128, 16)
    with pytest.raises(ValueError, match="rotary without an append"):
        prefill(q, kc, vc, cu, lens, bt, rotary_cos=table, rotary_sin=table)
    with pytest.raises(ValueError, match="inference only"):
        prefill(q.clone().requires_grad_(), kc, vc, cu, lens, bt)
    with pytest.raises(ValueError, match="block_table must be int32"):
        prefill(q, kc, vc, cu, lens, bt.long())
    with pytest.raises(ValueError, match="takes k and v together"):
        prefill(q, kc, vc, cu, lens, bt, k=torch.zeros(10, 2, 64, dtype=torch.float16))
    # everything in order: the first thing that stops a call on host tensors is the device check
    with pytest.raises(RuntimeError, match="must be on a ROCm device"):
        prefill(q, kc, vc, cu, lens, bt, k_descale=torch.ones(2, 2), v_descale=torch.ones(2, 2), max_seqlen_q=6)


# ---------------------------------------------------------------------------------------------------------------- the float64 checker's power
LENS = (700, 300, 129, 65, 64, 2, 1, 0, 40)           # tests/test_prefill_fp8_gpu.py's base case, H4 Hkv2 D64 fp16, general descales
NQS = (300, 257, 129, 65, 1, 2, 1, 0, 64)


def _as_outputs(ref, dtype):
    """A float64 reference as a kernel's answer: O rounded to the dtype, the LSE to float32."""
    return ref[0].to(dtype), ref[1].float()


def _per_head(codes, table, H):
    """Keys of query head h = the codes of K / V head h // g times table[s][h] -> [len, H, D] float32 lists (a reference with one K / V head per query head)."""
    g = H // codes[0].shape[1]
    return [c.float().repeat_interleave(g, 1) * table[s][None, :, None] for s, c in enumerate(codes)]


def test_float64_checker_has_power_for_descale_mistakes():
    H, Hkv, D, dtype = 4, 2, 64, torch.float16
    c = p8.make_case(LENS, NQS, H, Hkv, D, dtype, 11, torch.device("cpu"), descales="general")
    q, cu, scale, B = c["q"], c["cu"], D ** -0.5, len(LENS)
    true = pc.reference(q, cu, c["kt"], c["vt"], scale)
    assert not pc.check_float64("true", *_as_outputs(true, dtype), true)
    ones = torch.ones_like(c["kd"])
    flat = lambda d: [[float(d.reshape(-1)[min(s * Hkv + h, B * Hkv - 1)]) for h in range(H)] for s in range(B)]      # noqa: E731  ([s, h] on [B, Hkv] memory)
    nxt = lambda d: d.roll(-1, 0)                                                                                      # noqa: E731  (sequence s + 1's)
    wrong = {
        "k_descale ignored": (p8.dequant(c["kc"], ones), c["vt"]),
        "v_descale ignored": (c["kt"], p8.dequant(c["vc"], ones)),
        "[s, h] for [s, hkv]": (_per_head(c["kc"], torch.tensor(flat(c["kd"])), H), _per_head(c["vc"], torch.tensor(flat(c["vd"])), H)),
        "k: [s, h] for [s, hkv]": (_per_head(c["kc"], torch.tensor(flat(c["kd"])), H), c["vt"]),
        "v: [s, h] for [s, hkv]": (c["kt"], _per_head(c["vc"], torch.tensor(flat(c["vd"])), H)),
        "sequence s + 1's": (p8.dequant(c["kc"], nxt(c["kd"])), p8.dequant(c["vc"], nxt(c["vd"]))),
        "k: sequence s + 1's": (p8.dequant(c["kc"], nxt(c["kd"])), c["vt"]),
        "v: sequence s + 1's": (c["kt"], p8.dequant(c["vc"], nxt(c["vd"]))),
    }
    for name, (ks, vs) in wrong.items():
        if ks[0].shape[1] != vs[0].shape[1]:                # (one side per query head: the other side expanded to match, unchanged)
            g = H // Hkv
            ks, vs = ([t.repeat_interleave(g, 1) if t.shape[1] == Hkv else t for t in side] for side in (ks, vs))
        out = _as_outputs(pc.reference(q, cu, ks, vs, scale), dtype)
        assert pc.check_float64(name, *out, true), "%s passes the float64 check" % name
