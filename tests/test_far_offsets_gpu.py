"""64-bit addressing on the GPU: every tensor of a call — inputs, outputs, LSE, the delta workspace, a split's workspace — is a strided view into one
poisoned 4.25 GiB buffer, placed so that batch, head or row strides carry slices past byte offsets 2^31 and 2^32, or so that one head's span sits on
or beyond the documented limits (tests/far_layouts.py has the layouts, tests/test_far_offsets.py proves on the CPU that they cross what they claim).

Per case: the call runs on the far views and on a compact twin (same shapes, row pitches and data; span cases: the same pitch, the base moved);
where a plan query exists both must get the same plan, and the intended kernel; O, LSE, dQ, dK, dV (and delta) must be bitwise equal — the library is
deterministic, a tolerance would hide an off-by-one-slice read; the far outputs are held to dense float64 attention under tests/conftest.py's bars
(tools/fuzz_features.py's references and bar rule; tools/fuzz_mask.py's for the biased calls), so that twin and far cannot be wrong together; no
output row with a visible key holds a NaN; the inputs are unchanged; and after the views are poisoned again the whole arena is poison: nothing was
written outside the outputs.

Covered: the dense, windowed, dropout, biased and packed entry points and the operators (DENSE_CASES, SPAN_CASES, BIAS_SPAN_CASES, PACKED_CASES,
F32_CASES); the score-modifier calls, dense and packed, with ALiBi slopes whose batch stride is far (SCOREMOD_CASES, PACKED_CASES); every backward
with a gradient for the LSE — fa2_bwd_lse, fa2_bwd_window_lse on its three routes, fa2_bwd_varlen_lse —, the dlse far or compact beside far tensors,
a NaN in it on rows that see no key (LSE_CASES, tests/lse_refs.py's truth64 with u = dlse, and its non-vacuity rule); fa2_merge_fwd / fa2_merge_bwd
on three parts of one far stride set (MERGE_CASES, lse_refs.merge_check); fa2_fwd_decode, fa2_fwd_decode_fp8 and flash_attention_decode on caches
whose batches, K / V heads, key rows or pages are far, the block table, the descales and a split's workspace too (DECODE_CASES,
tests/decode_refs.py).  The inputs of a decode or merge case are written from byte images that hold poison wherever the call must not read — cache
rows at or beyond a length, unused pages, part rows of weight 0 — and are compared with those images afterwards.

The module skips — its only skip — when the device has less free memory than the arena plus 2 GiB."""
import ctypes
import importlib.util
import math
import os
import time

import pytest
import torch

import decode_calls as dc
import decode_refs as dr
import far_layouts as fl
import lse_refs as R
from conftest import FLOOR, GRAD_TOL, LSE_TRUTH_TOL, ROOT
from rocwmma_fattn import _fa2_lib

pytestmark = pytest.mark.gpu

CAUSAL, EXACT, BOTTOM_RIGHT = _fa2_lib.FA2_FLAG_CAUSAL, _fa2_lib.FA2_FLAG_EXACT_SCALE, _fa2_lib.FA2_FLAG_BOTTOM_RIGHT
HIP = (_fa2_lib.FA2_KERNEL_HIP_128, _fa2_lib.FA2_KERNEL_HIP_256)
BIAS_KINDS = {"io": _fa2_lib.FA2_BIAS_IO_DTYPE, "f32": _fa2_lib.FA2_BIAS_F32, "bool": _fa2_lib.FA2_BIAS_BOOL}
LN2 = math.log(2.0)


def _tool(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ff():
    return _tool("fuzz_features")


@pytest.fixture(scope="module")
def fm():
    return _tool("fuzz_mask")


def _arena(nbytes):
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    free, _ = torch.cuda.mem_get_info()
    print("free device memory at the arena's allocation: %.2f GiB (arena %.2f GiB)" % (free / fl.GIB, nbytes / fl.GIB))
    if free < nbytes + 2 * fl.GIB:
        pytest.skip("the far-offset arena needs %.2f GiB + 2 GiB of free device memory, the device reports %.2f GiB" % (nbytes / fl.GIB, free / fl.GIB))
    return fl.new_arena(nbytes, torch.device("cuda", 0))


@pytest.fixture(scope="module")
def arena():
    a = _arena(fl.ARENA_BYTES)
    yield a
    del a
    torch.cuda.empty_cache()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _s3(t):
    return _fa2_lib.strides3(t.stride(0), t.stride(1), t.stride(2))


def _s2(t):
    return _fa2_lib.strides2(t.stride(0), t.stride(1))


def _code(case):
    return _fa2_lib.FA2_DTYPE_F16 if case["dt"] == "f16" else _fa2_lib.FA2_DTYPE_BF16


def _bias_args(case, T):
    b = T["bias"]
    return b.data_ptr(), BIAS_KINDS[case["bias"][0]], _fa2_lib.strides3(*(b.stride(i) if b.size(i) > 1 else 0 for i in range(3)))


def _window(case):
    return case["window"] if case["window"] else (-1, -1, 0)


def _ws(T):
    return (T["ws"].data_ptr(), T["ws"].numel()) if "ws" in T else (None, 0)


def _fwd_flags(case):
    return (CAUSAL if case["causal"] else 0) | (EXACT if case["bwd"] else 0)


def _scale(case):
    return case["D"] ** -0.5


def _plan(case, T):
    """The plan query of the case's forward (None: the dropout calls have none)."""
    lib, plan = _fa2_lib.load(), _fa2_lib.FwdPlan()
    dims = (case["B"], case["H"], case["Hkv"], case["Nq"], case["Nkv"], case["D"])
    qs, ks, po = _s3(T["q"]), _s3(T["k"]), ctypes.byref(plan)
    if case["fam"] == "dense":
        _fa2_lib.check(lib.fa2_fwd_gqa_plan(_code(case), *dims, qs, ks, _scale(case), _fwd_flags(case), _ws(T)[1], po))
    elif case["fam"] == "window":
        _fa2_lib.check(lib.fa2_fwd_window_plan(_code(case), *dims, qs, ks, _scale(case), _fwd_flags(case), *_window(case), 0, po))
    elif case["fam"] == "bias":
        _fa2_lib.check(lib.fa2_fwd_plan(_code(case), *dims[:2], *dims[3:], qs, ks, _scale(case), _fwd_flags(case), BIAS_KINDS[case["bias"][0]], 0, po))
    else:
        return None
    return plan.as_dict()


BIAS_FORMS = {"tile": _fa2_lib.FA2_BIAS_FORM_TILE, "tile_dma": _fa2_lib.FA2_BIAS_FORM_TILE_DMA, "row": _fa2_lib.FA2_BIAS_FORM_ROW}


def _bias_form(case, T):
    """fa2_fwd_bias_form of the case's bias (its views are 16-byte aligned, as the query assumes)."""
    assert T["bias"].data_ptr() % 16 == 0
    ptr, kind, strides = _bias_args(case, T)
    return _fa2_lib.load().fa2_fwd_bias_form(kind, case["B"], case["H"], case["Nq"], case["Nkv"], case["D"], strides)


BWD_KERNELS = {"hip": _fa2_lib.FA2_BWD_KERNEL_HIP, "asm": _fa2_lib.FA2_BWD_KERNEL_ASM, "short": _fa2_lib.FA2_BWD_KERNEL_SHORT}


def _bwd_plan(case, T):
    """fa2_bwd_plan of the case's backward on the tensors T (dense and biased calls; the windowed and dropout backwards have no query): (dq, dkv)."""
    if case["fam"] not in ("dense", "bias"):
        return None
    plan = _fa2_lib.BwdPlan()
    kind, bstr = (_bias_args(case, T)[1:] if case["fam"] == "bias" else (_fa2_lib.FA2_BIAS_NONE, None))
    args = (_code(case), case["B"], case["H"], case["Hkv"], case["Nq"], case["Nkv"], case["D"], *[_s3(T[n]) for n in ("q", "k", "v", "o", "do")], _scale(case),
            CAUSAL if case["causal"] else 0, kind, bstr)
    if case.get("dlse"):                                                # fa2_bwd_lse's plan: with a dlse, head dim 128 leaves the hand-scheduled passes
        _fa2_lib.check(_fa2_lib.load().fa2_bwd_lse_plan(*args, 1, ctypes.byref(plan)))
    else:
        _fa2_lib.check(_fa2_lib.load().fa2_bwd_plan(*args, ctypes.byref(plan)))
    return plan.dq_kernel, plan.dkv_kernel


def _smod_args(case, T):
    """(softcap, alibi_slopes, alibi_batch_stride): [B, H] slopes with their batch stride, one shared [H] vector with stride 0."""
    if "slopes" not in T:                                               # soft-capping alone
        return case["softcap"], None, 0
    sl = T["slopes"]
    return case["softcap"], sl.data_ptr(), sl.stride(0) if sl.shape[0] > 1 else 0


def _fwd_args(case, T, pitch_bump=None):
    """(function, arguments) of the case's forward on the tensors T.  pitch_bump = (name, elements): that tensor's row pitch, raised."""
    lib, dt = _fa2_lib.load(), _code(case)
    B, H, Hkv, Nq, Nkv, D = (case[n] for n in ("B", "H", "Hkv", "Nq", "Nkv", "D"))
    st = {n: list(T[n].stride()[:3]) for n in ("q", "k", "v", "o")}
    if pitch_bump:
        st[pitch_bump[0]][2] += pitch_bump[1]
    ptrs = [T[n].data_ptr() for n in ("q", "k", "v", "o", "lse")]
    strides = [_fa2_lib.strides3(*st[n]) for n in ("q", "k", "v", "o")] + [_s2(T["lse"])]
    tail = (*strides, _scale(case), _fwd_flags(case))
    if case["fam"] == "dense":
        if Hkv == H and "ws" not in T:
            return lib.fa2_fwd, (dt, *ptrs, B, H, Nq, Nkv, D, *tail, _stream())
        return lib.fa2_fwd_gqa, (dt, *ptrs, B, H, Hkv, Nq, Nkv, D, *tail, *_ws(T), _stream())
    if case["fam"] == "window":
        return lib.fa2_fwd_window, (dt, *ptrs, B, H, Hkv, Nq, Nkv, D, *tail, *_window(case), _stream())
    if case["fam"] == "dropout":
        return lib.fa2_fwd_dropout, (dt, *ptrs, B, H, Hkv, Nq, Nkv, D, *tail, *_window(case), _stream(), case["p"], case["seed"])
    if case["fam"] == "scoremod":
        return lib.fa2_fwd_scoremod, (dt, *ptrs, B, H, Hkv, Nq, Nkv, D, *tail, *_window(case), _stream(), *_smod_args(case, T))
    return lib.fa2_fwd_bias, (dt, *ptrs, B, H, Nq, Nkv, D, *tail, *_bias_args(case, T), _stream())


def _bwd_args(case, T, pitch_bump=None):
    lib, dt = _fa2_lib.load(), _code(case)
    B, H, Hkv, Nq, Nkv, D = (case[n] for n in ("B", "H", "Hkv", "Nq", "Nkv", "D"))
    names = ("q", "k", "v", "o", "do", "dq", "dk", "dv")
    st = {n: list(T[n].stride()[:3]) for n in names}
    if pitch_bump:
        st[pitch_bump[0]][2] += pitch_bump[1]
    assert T["delta"].stride() == T["lse"].stride()                     # the delta workspace takes the LSE's strides
    ptrs = [T[n].data_ptr() for n in ("q", "k", "v", "o", "do", "lse", "dq", "dk", "dv", "delta")]
    tail = (*[_fa2_lib.strides3(*st[n]) for n in names], _s2(T["lse"]), _scale(case), CAUSAL if case["causal"] else 0)
    if case.get("dlse"):                                                # a gradient for the LSE: the family's backward, then dlse and its own strides
        assert Hkv == H and "ws" not in T
        dlse = (T["dlse"].data_ptr(), _s2(T["dlse"]))
        if case["fam"] in ("dense", "bias"):
            bias = _bias_args(case, T) if case["fam"] == "bias" else (None, _fa2_lib.FA2_BIAS_NONE, None)
            return lib.fa2_bwd_lse, (dt, *ptrs, B, H, Nq, Nkv, D, *tail, *bias, None, 0, _stream(), *dlse)
        drop = (case["p"], case["seed"]) if case["fam"] == "dropout" else (0.0, 0)
        smod = _smod_args(case, T) if case["fam"] == "scoremod" else (0.0, None, 0)
        return lib.fa2_bwd_window_lse, (dt, *ptrs, B, H, Nq, Nkv, D, *tail, *_window(case), _stream(), *drop, *smod, *dlse)
    if case["fam"] == "dense":
        if Hkv == H and "ws" not in T:
            return lib.fa2_bwd, (dt, *ptrs, B, H, Nq, Nkv, D, *tail, _stream())
        return lib.fa2_bwd_gqa, (dt, *ptrs, B, H, Hkv, Nq, Nkv, D, *tail, *_ws(T), _stream())
    assert Hkv == H                                                     # (the windowed, dropout and biased backwards are multi-head calls)
    if case["fam"] == "window":
        return lib.fa2_bwd_window, (dt, *ptrs, B, H, Nq, Nkv, D, *tail, *_window(case), _stream())
    if case["fam"] == "dropout":
        return lib.fa2_bwd_dropout, (dt, *ptrs, B, H, Nq, Nkv, D, *tail, *_window(case), _stream(), case["p"], case["seed"])
    if case["fam"] == "scoremod":
        return lib.fa2_bwd_scoremod, (dt, *ptrs, B, H, Nq, Nkv, D, *tail, *_window(case), _stream(), *_smod_args(case, T))
    return lib.fa2_bwd_bias, (dt, *ptrs, B, H, Nq, Nkv, D, *tail, *_bias_args(case, T), _stream())


def _inputs(case, specs, dev):
    """Random inputs of the case (one generator, the case's seed): {name: tensor on the device}, shapes as the slots'."""
    g = torch.Generator(device="cpu").manual_seed(case["seed"] & 0xFFFFFF)
    dt, data = fl.DTYPES[case["dt"]], {}
    for name in ("q", "k", "v") + (("do",) if case["bwd"] else ()):
        data[name] = torch.randn(specs[name].shape, generator=g).to(dt).to(dev)
    if case.get("bias"):
        kind, shape = case["bias"]
        if kind == "bool":
            m = torch.rand(shape, generator=g) < 0.8
            m[..., 0] = True                                            # every row keeps a key
            data["bias"] = m.to(dev)
        else:
            data["bias"] = (torch.randn(shape, generator=g) * 0.5).to(dt if kind == "io" else torch.float32).to(dev)
    if case.get("slopes"):                                              # ALiBi-sized, another vector per batch
        n, H = specs["slopes"].shape
        data["slopes"] = (0.5 ** (1 + torch.arange(H, dtype=torch.float32))[None, :] * (1.0 + 0.25 * torch.arange(n, dtype=torch.float32))[:, None]).to(dev)
    if case.get("dlse"):                                                # log2 units; rows that see no key carry a NaN
        dlse = torch.randn(specs["dlse"].shape, generator=g) * LN2
        dlse[:, :, ~R.ff.band(case["Nq"], case["Nkv"], *_window(case), case["causal"], "cpu").any(-1)] = float("nan")
        data["dlse"] = dlse.to(dev)
    return data


def _expect(case, plan, plan_twin):
    if plan is None:
        return
    assert plan == plan_twin, ("the twin is planned differently", plan, plan_twin)
    want, k = case["expect"], plan["kernel"]
    if want == "hip":
        assert k in HIP and plan["nsplit"] == 0, plan
    elif want == "asm":
        assert k == _fa2_lib.FA2_KERNEL_ASM and plan["rows"] == 256 and plan["kernel_tail"] == 0, plan
    elif want == "asm128":
        assert k == _fa2_lib.FA2_KERNEL_ASM and plan["rows"] == 128, plan
    elif want == "split":
        assert plan["nsplit"] > 1 and plan["split_items"] == case["B"] * case["H"], plan
    elif want == "bias":
        assert k == _fa2_lib.FA2_KERNEL_HIP_BIAS, plan
    elif want == "window":
        assert k == _fa2_lib.FA2_KERNEL_HIP_WINDOW, plan


def _truth_dense(ff, case, out, data):
    """Far outputs against dense float64 attention, batch by batch (tools/fuzz_features.py: ref64, the same-contract emulation in the reference's
    role, the bar rule max(2 * its error, tol * max(1, max|truth|)) with conftest's FLOOR / GRAD_TOL; LSE within LSE_TRUTH_TOL on live rows).
    -> (failures, live rows [B, H, Nq])."""
    code, dt, dev = _code(case), fl.DTYPES[case["dt"]], out["o"].device
    B, H, Hkv, Nq, Nkv = (case[n] for n in ("B", "H", "Hkv", "Nq", "Nkv"))
    left, right, off = _window(case)
    band = ff.band(Nq, Nkv, left, right, off, case["causal"], dev)
    fails, live = [], (band.any(-1)[None, None].expand(B, H, Nq))
    for b in range(B):
        keep = ff.keep_unit(case["seed"], case["p"], H, b, Nq, Nkv).to(dev)
        ke, ve = (data[n][b].repeat_interleave(H // Hkv, 0) for n in ("k", "v"))
        do = data["do"][b] if case["bwd"] else torch.zeros_like(data["q"][b])
        O, lse, dQ, dK, dV = ff.ref64(data["q"][b], ke, ve, do, keep, band, _scale(case), case["p"])
        eO, edQ, edK, edV = ff.emu(data["q"][b], ke, ve, do, keep, band, _scale(case), case["p"], dt)
        pairs = [("o", out["o"][b], O, eO, FLOOR[code])]
        if case["bwd"]:
            pairs += [("dq", out["dq"][b], dQ, edQ, GRAD_TOL[code]), ("dk", out["dk"][b], ff.fold_groups(dK, Hkv), ff.fold_groups(edK, Hkv), GRAD_TOL[code]),
                      ("dv", out["dv"][b], ff.fold_groups(dV, Hkv), ff.fold_groups(edV, Hkv), GRAD_TOL[code])]
        for n, got, true, em, tol in pairs:
            err, err_emu, bar = ff.error_and_bar(got, true, em, tol)
            if not err <= bar:
                fails.append("batch %d: %s err %.3e > %.3e against float64 (emulation %.3e)" % (b, n, err, bar, err_emu))
        lv = band.any(-1)
        lerr = (out["lse"][b][:, lv].double() - lse[:, lv]).abs().max().item()
        if not lerr <= LSE_TRUTH_TOL[code]:
            fails.append("batch %d: LSE err %.3e > %.3e against float64" % (b, lerr, LSE_TRUTH_TOL[code]))
    return fails, live


def _truth_bias(fm, case, out, data):
    """The biased calls against tools/fuzz_mask.py's dense float64 attention and its autograd; bars: conftest's FLOOR / GRAD_TOL at the largest true
    magnitude (one / two ulps of the I/O dtype there), LSE_TRUTH_TOL."""
    code = _code(case)
    q64, k64, v64 = (data[n].double().requires_grad_(True) for n in ("q", "k", "v"))
    o64 = fm.dense64(q64, k64, v64, data["bias"], case["causal"], _scale(case))
    pairs = [("o", o64.detach(), FLOOR[code])]
    if case["bwd"]:
        o64.backward(data["do"].double())
        pairs += [("dq", q64.grad, GRAD_TOL[code]), ("dk", k64.grad, GRAD_TOL[code]), ("dv", v64.grad, GRAD_TOL[code])]
    fails = []
    for n, true, tol in pairs:
        err, bar = (out[n].double() - true).abs().max().item(), tol * max(1.0, true.abs().max().item())
        if not err <= bar:
            fails.append("%s err %.3e > %.3e against float64" % (n, err, bar))
    s = (data["q"].double() @ data["k"].double().transpose(-1, -2)) * _scale(case)
    s = s.masked_fill(~data["bias"], float("-inf")) if data["bias"].dtype == torch.bool else s + data["bias"].double()
    lerr = (out["lse"].double() - torch.logsumexp(s, -1) / LN2).abs().max().item()
    if not lerr <= LSE_TRUTH_TOL[code]:
        fails.append("LSE err %.3e > %.3e against float64" % (lerr, LSE_TRUTH_TOL[code]))
    return fails, None


def _truth_lse(case, out, data):
    """The score-modifier calls and every backward with a dlse against tests/lse_refs.py, batch by batch: truth64 (float64 autograd of the contract
    with the LSE as a second output, u = dlse in natural-log units), emulate and bars_of, as tests/test_lse_gpu.py uses them; over the whole call the
    LSE term must move the float64 dQ and dK by five bars (check_not_vacuous).  Rows that see no key: O, dQ zero, whatever their dlse holds."""
    dt, dev = fl.DTYPES[case["dt"]], out["o"].device
    B, H, Hkv, Nq, Nkv = (case[n] for n in ("B", "H", "Hkv", "Nq", "Nkv"))
    left, right, off = _window(case)
    allow0 = R.ff.band(Nq, Nkv, left, right, off, case["causal"], dev)
    fails, whole, live = [], ([], [], []), allow0.any(-1)[None, None].expand(B, H, Nq)
    for b in range(B):
        allow, bias, keep, rs, u = allow0, None, None, 1.0, None
        if case["fam"] == "bias":
            m = data["bias"][b if data["bias"].shape[0] > 1 else 0]
            allow, bias = (allow0 & m, None) if m.dtype == torch.bool else (allow0, m)
        if case["fam"] == "dropout":
            keep, rs = R.ff.keep_unit(case["seed"], case["p"], H, b, Nq, Nkv).to(dev), 1.0 / (1.0 - R.ff.p_eff(case["p"]))
        slopes = data["slopes"][b if data["slopes"].shape[0] > 1 else 0] if case.get("slopes") else None
        if case.get("dlse"):
            u = torch.nan_to_num(data["dlse"][b], nan=0.0) / LN2         # (a dead row ignores its dlse: the references are given 0 there)
        kw = dict(softcap=case["softcap"], slopes=slopes, off=off, bias=bias, keep=keep, rs=rs)
        ke, ve = (data[n][b].repeat_interleave(H // Hkv, 0) for n in ("k", "v"))
        do = data["do"][b] if case["bwd"] else torch.zeros_like(data["q"][b])
        true, emu, plain = R.truth64(data["q"][b], ke, ve, do, u, allow, _scale(case), **kw), R.emulate(data["q"][b], ke, ve, do, u, allow, _scale(case), dt, **kw), None
        if u is not None:
            plain = R.truth64(data["q"][b], ke, ve, do, None, allow, _scale(case), **kw)
        for d in (true, emu) + ((plain,) if plain else ()):
            d["dK"], d["dV"] = R.fold(d["dK"], Hkv), R.fold(d["dV"], Hkv)
        bars = R.bars_of(true, emu, dt)
        got = dict(O=out["o"][b], lse=out["lse"][b])
        if case["bwd"]:
            got.update(dQ=out["dq"][b], dK=out["dk"][b], dV=out["dv"][b])
        try:
            R.check("%s b%d" % (case["id"], b), got, true, bars, names=tuple(got))
        except AssertionError as e:
            fails.append("batch %d: %s" % (b, e))
        dead = torch.isinf(true["lse"])
        if dead.any() and not ((got["O"][dead] == 0).all() and (not case["bwd"] or (got["dQ"][dead] == 0).all())):
            fails.append("batch %d: a row that sees no key has a non-zero O or dQ" % b)
        for acc, d in zip(whole, (true, emu, plain)):
            acc.append(d)
    if case.get("dlse"):
        assert not case["window"] or (~live).any(), "the windowed dlse cases are there for their dead rows"
        true, emu, plain = ({n: torch.stack([d[n] for d in acc]) for n in R.NAMES} for acc in whole)
        R.check_not_vacuous(case["id"], true, plain, R.bars_of(true, emu, dt))
    return fails, live


def _run_dense(case, arena, slots, twin, twin_arena, ff, fm):
    """One dense case: far call and twin, then every check of the module's docstring.  twin_arena None: the twin lives in the arena too."""
    t0 = time.perf_counter()
    same = twin_arena is None
    fl.validate(list(slots.values()) + (list(twin.values()) if same else []), arena.numel())      # bounds before anything runs
    if not same:
        fl.validate(list(twin.values()), twin_arena.numel())
    data = _inputs(case, slots, arena.device)
    fl.write_inputs(arena, slots, data)
    fl.write_inputs(arena if same else twin_arena, twin, data)
    T = {n: s.view(arena) for n, s in slots.items()}
    Tt = {n: s.view(arena if same else twin_arena) for n, s in twin.items()}
    outs = ["o", "lse"] + (["dq", "dk", "dv", "delta"] if case["bwd"] else [])
    with _fa2_lib.options(**case["opts"]):
        plan, plan_t = _plan(case, T), _plan(case, Tt)
        _expect(case, plan, plan_t)
        form = None
        if case["fam"] == "bias":
            form, form_t = _bias_form(case, T), _bias_form(case, Tt)
            assert form == form_t and (not case.get("form") or form == BIAS_FORMS[case["form"]]), (form, form_t, case.get("form"))
        bplan = None
        if case["bwd"]:
            bplan, bplan_t = _bwd_plan(case, T), _bwd_plan(case, Tt)
            assert bplan == bplan_t, ("the twin's backward is planned differently", bplan, bplan_t)
            if bplan is not None and case.get("expect_bwd"):
                assert bplan == tuple(BWD_KERNELS[k] for k in case["expect_bwd"]), (bplan, case["expect_bwd"])
        for tensors in (T, Tt):
            fn, args = _fwd_args(case, tensors)
            _fa2_lib.check(fn(*args))
            if case["bwd"]:
                fn, args = _bwd_args(case, tensors)
                _fa2_lib.check(fn(*args))
    torch.cuda.synchronize()
    if same:
        both = fl.harvest(arena, dict(slots, **{n + "_t": s for n, s in twin.items()}))
        far, tw = {n: t for n, t in both.items() if not n.endswith("_t")}, {n[:-2]: t for n, t in both.items() if n.endswith("_t")}
    else:
        far, tw = fl.harvest(arena, slots), fl.harvest(twin_arena, twin)
    fails = ["input %s was written" % n for n in data if not torch.equal(fl._bits(far[n]), fl._bits(data[n]))]      # (bits: a dlse may hold NaNs)
    fails += fl.compare_exact(far, tw, outs)
    if case["fam"] == "scoremod" or case.get("dlse"):
        truth, live = _truth_lse(case, far, data)
    else:
        truth, live = (_truth_bias(fm, case, far, data) if case["fam"] == "bias" else _truth_dense(ff, case, far, data))
    fails += truth
    fails += fl.nan_in_live_rows(far, [n for n in outs if n not in ("dk", "dv")], live) + fl.nan_in_live_rows(far, [n for n in outs if n in ("dk", "dv")])
    print("%s: plan %s, bias form %s, backward (dq, dkv) %s, %.2f s" % (case["id"], plan, form, bplan, time.perf_counter() - t0))
    assert not fails, fails
    return T


def _twin_arena(nbytes, dev):
    return fl.new_arena(fl._up(nbytes, 8) + 8, dev)


@pytest.mark.parametrize("case", fl.DENSE_CASES, ids=lambda c: c["id"])
def test_far_batch_and_head_strides(case, arena, ff, fm):
    """Every dense entry point and kernel family with its batches or heads 2 GiB apart (tests/far_layouts.py: DENSE_CASES says which call reaches
    which kernel; the plan is asserted where a query exists)."""
    lib, ws = _fa2_lib.load(), 0
    if case["ws"]:
        dims = (_code(case), case["B"], case["H"], case["Hkv"], case["Nq"], case["Nkv"], case["D"], 0)
        ws = max(lib.fa2_fwd_gqa_workspace_bytes(*dims), lib.fa2_bwd_gqa_workspace_bytes(*dims) if case["bwd"] else 0)
        assert ws > 0, "this shape was chosen to split"
        if case["expect"] == "bwd_split":
            assert lib.fa2_bwd_gqa_workspace_bytes(*dims) > 0
    slots, twin, tbytes = fl.dense_slots(case, ws)
    _run_dense(case, arena, slots, twin, _twin_arena(tbytes, arena.device), ff, fm)


@pytest.mark.parametrize("case", fl.SPAN_CASES, ids=lambda c: c["id"])
def test_spans_on_and_past_the_limits(case, arena, ff, fm):
    """One head whose span sits on the last accepted pitch of the 2 GiB rule (K, V; backward: Q and dO too), and Q / O (forward), O / dQ / dK / dV
    (backward) spans in [2 GiB, 4 GiB) and past 4 GiB, which the library accepts: the plan keeps the hand-scheduled forward below 4 GiB and leaves
    it above; the backward keeps the hand-scheduled passes with O on the last pitch of the 2 GiB rule and leaves them from there on (the dQ pass
    would form O's row offsets in 32 bits: fa2_bwd_plan is asserted).  Then the next pitch of every bounded
    tensor is refused by the launching entry point itself (real tensors: a refusal launches nothing)."""
    slots, twin = fl.span_slots(case)
    T = _run_dense(case, arena, slots, twin, None, ff, fm)
    if case["pitch"] == "limit":
        shape = -2                                                      # FA2_ERR_BAD_SHAPE
        assert _fa2_lib.error_string(shape).startswith("fa2: B, H, Nq")
        for name in case["wide"]:
            if name == "o":
                continue                                                # (not refused: the plan leaves the hand-scheduled passes, tests/test_far_offsets.py)
            # (the dense call, and the windowed and dropout calls of the same tensors: one validation serves them all)
            families = [case, dict(case, fam="window", window=fl.W100), dict(case, fam="dropout", window=fl.W100, p=0.25)]
            # ... and the score-modifier calls, which inherit the windowed call's span rules
            families.append(dict(case, fam="scoremod", window=fl.W100, softcap=30.0))
            for c in families:
                if case["bwd"]:
                    fn, args = _bwd_args(c, T, (name, 8))
                    assert fn(*args) == shape, (name, c["fam"])
                    # the same backward with a gradient for the LSE (fa2_bwd_lse, fa2_bwd_window_lse: the dlse arguments are checked last)
                    fn, args = _bwd_args(dict(c, dlse="far"), dict(T, dlse=T["lse"]), (name, 8))
                    assert fn in (_fa2_lib.load().fa2_bwd_lse, _fa2_lib.load().fa2_bwd_window_lse) and fn(*args) == shape, (name, c["fam"], "dlse")
                if name in ("k", "v"):
                    fn, args = _fwd_args(c, T, (name, 8))
                    assert fn(*args) == shape, (name, c["fam"])
        torch.cuda.synchronize()
        assert fl.arena_is_poison(arena)


@pytest.mark.parametrize("case", fl.BIAS_SPAN_CASES, ids=lambda c: c["id"])
def test_bias_slice_on_the_last_accepted_span(case, arena, ff, fm):
    """fa2_fwd_bias / fa2_bwd_bias with one bias slice on the last pitch of the 2 GiB slice rule (whole granules: the tile forms), its base past 2^31
    and its end past 2^32: an f32 slice of one head; an fp16 slice shared by a grid past 3/8 of the CUs, which the forward stages by LDS-DMA with
    32-bit offsets (fa2_fwd_bias_form is asserted); and that grid on the next pitch, where the forward leaves the LDS-DMA form and is still right.
    fa2_bwd_bias refuses the next pitch."""
    slots, twin = fl.bias_span_slots(case)
    T = _run_dense(case, arena, slots, twin, None, ff, fm)
    if case["bwd"]:
        fn, args = _bwd_args(case, T)
        args = list(args)
        b = T["bias"]
        args[-2] = _fa2_lib.strides3(0, 0, b.stride(2) + 16 // b.element_size())
        assert fn(*args) == -2                                           # FA2_ERR_BAD_SHAPE
        torch.cuda.synchronize()
        assert fl.arena_is_poison(arena)


@pytest.mark.parametrize("case", list(fl.SCOREMOD_CASES) + list(fl.LSE_CASES), ids=lambda c: c["id"])
def test_score_modifiers_and_lse_gradients_far(case, arena, ff, fm):
    """fa2_fwd_scoremod / fa2_bwd_scoremod (soft-capping and ALiBi slopes on a causal window; slopes [B, H] with a far alibi_batch_stride, or one shared
    [H] vector) and the backwards that take a gradient for the LSE — fa2_bwd_lse plain and biased, fa2_bwd_window_lse on its windowed, dropout and
    score-modifier routes — with dlse far like lse or compact beside far tensors (tests/far_layouts.py: SCOREMOD_CASES, LSE_CASES).  delta holds
    the modified row term and is compared with the twin's like every output."""
    slots, twin, tbytes = fl.dense_slots(case)
    _run_dense(case, arena, slots, twin, _twin_arena(tbytes, arena.device), ff, fm)


# ---------------------------------------------------------------------------------------------------------------- packed, row-far
def _cu(lens, dev):
    return torch.tensor([0] + [sum(lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32, device=dev)


def _packed_call(case, T, cu, cu_k, fwd):
    lib, dt = _fa2_lib.load(), _code(case)
    H, Hkv, D, B, mq, mk = case["H"], case["Hkv"], case["D"], len(fl.PACKED_LENS), max(fl.PACKED_LENS), max(fl.PACKED_LENS_K)
    s2 = lambda t: _fa2_lib.strides2(t.stride(1), t.stride(0))          # noqa: E731  {head, row}
    flags = (CAUSAL if case["causal"] else 0) | (BOTTOM_RIGHT if case["bottom_right"] else 0) | (EXACT if case["bwd"] and fwd else 0)
    drop = (case["p"], case["seed"]) if case["p"] > 0 else ()
    smod = (case.get("softcap", 0.0), T["slopes"].data_ptr(), T["slopes"].stride(0)) if case.get("slopes") else ()
    if smod or case.get("dlse"):
        assert not drop
        if fwd:
            fn, drop = (lib.fa2_fwd_varlen_scoremod if smod else lib.fa2_fwd_varlen), smod
        elif case.get("dlse"):                                          # fa2_bwd_varlen's arguments, dropout, score modifiers, then dlse and its head stride
            fn, drop = lib.fa2_bwd_varlen_lse, (0.0, 0, *(smod or (0.0, None, 0)), T["dlse"].data_ptr(), T["dlse"].stride(0))
        else:
            fn, drop = lib.fa2_bwd_varlen_scoremod, smod
    elif fwd:
        fn = lib.fa2_fwd_varlen_dropout if drop else lib.fa2_fwd_varlen
    else:
        fn = lib.fa2_bwd_varlen_dropout if drop else lib.fa2_bwd_varlen
    if fwd:
        return fn(dt, *[T[n].data_ptr() for n in ("q", "k", "v", "o", "lse")], B, H, Hkv, mq, mk, D, cu.data_ptr(), cu_k.data_ptr(),
                  *[s2(T[n]) for n in ("q", "k", "v", "o")], T["lse"].stride(0), D ** -0.5, flags, -1, -1, _stream(), *drop)
    assert T["delta"].stride() == T["lse"].stride() and H == Hkv
    return fn(dt, *[T[n].data_ptr() for n in ("q", "k", "v", "o", "do", "lse", "dq", "dk", "dv", "delta")], B, H, mq, mk, D, cu.data_ptr(), cu_k.data_ptr(),
              *[s2(T[n]) for n in ("q", "k", "v", "o", "do", "dq", "dk", "dv")], T["lse"].stride(0), D ** -0.5, flags, -1, -1, _stream(), *drop)


@pytest.mark.parametrize("case", fl.PACKED_CASES, ids=lambda c: c["id"])
def test_packed_rows_a_mebibyte_apart(case, arena, ff):
    """fa2_fwd_varlen / fa2_bwd_varlen and the dropout pair on [total, H, D] views whose rows are 1 MiB apart: cu_seqlens[s] * row pitch passes 2^31 and
    2^32.  The K / V lengths differ from the Q lengths: a sequence's Q and K bases are different far rows, and bottom-right causal is told from
    top-left by the float64 reference (its rows without a visible key: O and dQ zero, LSE -inf).  The twin is the same call on contiguous rows (the
    pitch cannot be kept compactly).  Rows behind cu[B] stay poison."""
    t0 = time.perf_counter()
    dev, lens, code, dt = arena.device, fl.PACKED_LENS, _code(case), fl.DTYPES[case["dt"]]
    slots, twin, tbytes = fl.packed_slots(case)
    fl.validate(list(slots.values()), arena.numel())
    tarena = _twin_arena(tbytes, dev)
    fl.validate(list(twin.values()), tarena.numel())
    lens_k = fl.PACKED_LENS_K
    assert len(lens_k) == len(lens) and lens_k != lens and sum(lens_k) <= fl.PACKED_TOTAL
    cu, cu_k = _cu(lens, dev), _cu(lens_k, dev)
    used = {n: sum(lens_k) if n in ("k", "v", "dk", "dv") else sum(lens) for n in slots}      # rows of each tensor the sequences take
    g = torch.Generator(device="cpu").manual_seed(case["seed"] & 0xFFFFFF)
    data = {n: torch.randn(slots[n].shape, generator=g).to(dt).to(dev) for n in ("q", "k", "v") + (("do",) if case["bwd"] else ())}
    lse_mode = bool(case.get("slopes") or case.get("dlse"))             # these are held to tests/lse_refs.py, like their dense calls
    if case.get("slopes"):                                              # another vector per sequence
        data["slopes"] = (0.5 ** (1 + torch.arange(case["H"], dtype=torch.float32))[None, :] * (1.0 + 0.125 * torch.arange(len(lens), dtype=torch.float32))[:, None]).to(dev)
        used["slopes"] = len(lens)
    if case.get("dlse"):                                                # log2 units; a NaN on the bottom-right rows that see no key
        dlse = torch.randn(slots["dlse"].shape, generator=g) * LN2
        for s, (n, nk) in enumerate(zip(lens, lens_k)):
            a = int(cu[s])
            dlse[:, a:a + max(n - nk, 0)] = float("nan")
        data["dlse"] = dlse.to(dev)
        assert torch.isnan(dlse).any() and case["bottom_right"]
    T, Tt = {n: s.view(arena) for n, s in slots.items()}, {n: s.view(tarena) for n, s in twin.items()}
    for tensors in (T, Tt):                                             # only the rows of the sequences are written: the rest stays poison
        for n, t in data.items():
            if n == "dlse":
                tensors[n][:, :used[n]].copy_(t[:, :used[n]])
            else:
                tensors[n][:used[n]].copy_(t[:used[n]])
    plan = _fa2_lib.FwdPlan()
    for tensors in (T, Tt):
        _fa2_lib.check(_fa2_lib.load().fa2_fwd_varlen_plan(code, len(lens), case["H"], case["Hkv"], max(lens), max(lens_k), case["D"],
                                                          _fa2_lib.strides2(tensors["q"].stride(1), tensors["q"].stride(0)),
                                                          _fa2_lib.strides2(tensors["k"].stride(1), tensors["k"].stride(0)), case["D"] ** -0.5,
                                                          CAUSAL if case["causal"] else 0, -1, -1, ctypes.byref(plan)))
        assert plan.kernel == _fa2_lib.FA2_KERNEL_HIP_VARLEN
        _fa2_lib.check(_packed_call(case, tensors, cu, cu_k, True))
        if case["bwd"]:
            _fa2_lib.check(_packed_call(case, tensors, cu, cu_k, False))
    torch.cuda.synchronize()
    far, tw = fl.harvest(arena, slots), fl.harvest(tarena, twin)
    outs = ["o", "lse"] + (["dq", "dk", "dv", "delta"] if case["bwd"] else [])
    cut = lambda t, n: t[:, :used[n]] if n == "dlse" else t[:used[n]]      # noqa: E731
    fails = ["input %s was written" % n for n in data if not torch.equal(fl._bits(cut(far[n], n)), fl._bits(cut(data[n], n)))]
    poison16 = torch.full((), -1, dtype=torch.int16, device=dev)
    for n in far:                                                       # rows behind cu[B]: untouched, in inputs and outputs alike
        tail = far[n][:, used[n]:] if n in ("lse", "delta", "dlse") else far[n][used[n]:]
        if not (tail.contiguous().view(torch.int16) == poison16).all():
            fails.append("%s: rows behind cu[B] were written" % n)
    rows = lambda t, n: t[:, :used[n]] if n in ("lse", "delta") else t[:used[n]]      # noqa: E731
    fails += fl.compare_exact({n: rows(far[n], n) for n in outs}, {n: rows(tw[n], n) for n in outs}, outs)
    H, Hkv = case["H"], case["Hkv"]
    for s, (n, nk) in enumerate(zip(lens, lens_k)):
        if n == 0:
            continue
        a, ak = int(cu[s]), int(cu_k[s])
        hm = lambda t: t[a:a + n].transpose(0, 1)                       # noqa: E731  [H, n, D]
        hk = lambda t: t[ak:ak + nk].transpose(0, 1)                    # noqa: E731  [Hkv, nk, D]
        band = ff.band(n, nk, -1, -1, nk - n if case["bottom_right"] else 0, case["causal"], dev)
        live = band.any(-1)
        keep = ff.keep_unit(case["seed"], case["p"], H, s, n, nk).to(dev)
        ke, ve = (hk(data[x]).repeat_interleave(H // Hkv, 0) for x in ("k", "v"))
        do = hm(data["do"]) if case["bwd"] else torch.zeros_like(hm(data["q"]))
        if lse_mode:
            u = torch.nan_to_num(data["dlse"][:, a:a + n], nan=0.0) / LN2 if case.get("dlse") else None
            kw = dict(softcap=case.get("softcap", 0.0), slopes=data["slopes"][s] if case.get("slopes") else None, off=nk - n if case["bottom_right"] else 0)
            true, emu = R.truth64(hm(data["q"]), ke, ve, do, u, band, case["D"] ** -0.5, **kw), R.emulate(hm(data["q"]), ke, ve, do, u, band, case["D"] ** -0.5, dt, **kw)
            bars = R.bars_of(true, emu, dt)
            got = dict(O=hm(far["o"]), lse=far["lse"][:, a:a + n])
            if case["bwd"]:
                got.update(dQ=hm(far["dq"]), dK=hk(far["dk"]), dV=hk(far["dv"]))
            try:
                R.check("%s sequence %d" % (case["id"], s), got, true, bars, names=tuple(got))
            except AssertionError as e:
                fails.append("sequence %d: %s" % (s, e))
            if not ((got["O"][:, ~live] == 0).all() and (not case["bwd"] or (got["dQ"][:, ~live] == 0).all())):
                fails.append("sequence %d: a row that sees no key has a non-zero O or dQ" % s)
            if case.get("dlse") and s == 0:                              # the longest sequence: a kernel that ignores dlse cannot pass
                assert (~live).any()
                R.check_not_vacuous(case["id"], true, R.truth64(hm(data["q"]), ke, ve, do, None, band, case["D"] ** -0.5, **kw), bars)
            continue
        O, lse, dQ, dK, dV = ff.ref64(hm(data["q"]), ke, ve, do, keep, band, case["D"] ** -0.5, case["p"])
        eO, edQ, edK, edV = ff.emu(hm(data["q"]), ke, ve, do, keep, band, case["D"] ** -0.5, case["p"], dt)
        pairs = [("o", hm(far["o"]), O, eO, FLOOR[code])]
        if case["bwd"]:
            pairs += [("dq", hm(far["dq"]), dQ, edQ, GRAD_TOL[code]), ("dk", hk(far["dk"]), dK, edK, GRAD_TOL[code]), ("dv", hk(far["dv"]), dV, edV, GRAD_TOL[code])]
        for name, got, true, em, tol in pairs:
            err, err_emu, bar = ff.error_and_bar(got, true, em, tol)
            if not err <= bar:
                fails.append("sequence %d: %s err %.3e > %.3e against float64 (emulation %.3e)" % (s, name, err, bar, err_emu))
            if torch.isnan(got.float()).any():
                fails.append("sequence %d: NaN in %s" % (s, name))
        got_lse = far["lse"][:, a:a + n]
        lerr = (got_lse[:, live].double() - lse[:, live]).abs().max().item()
        if not lerr <= LSE_TRUTH_TOL[code]:
            fails.append("sequence %d: LSE err %.3e > %.3e against float64" % (s, lerr, LSE_TRUTH_TOL[code]))
        if not torch.isneginf(got_lse[:, ~live]).all():
            fails.append("sequence %d: the LSE of a row without a visible key is not -inf" % s)
    print("%s: plan %s, %.2f s" % (case["id"], plan.as_dict(), time.perf_counter() - t0))
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------- the operator
def _operator_case(bnhd):
    return dict(id="operator", fam="dense", dt="f16", B=3, H=2, Hkv=2, Nq=320, Nkv=320, D=64, causal=True, far="batch", bwd=True, opts={}, expect=None, ws=None,
                window=None, p=0.0, seed=0x5EED4000 + bnhd, bias=None, layout="far")


@pytest.mark.parametrize("bnhd", [False, True], ids=["bhnd", "bnhd"])
def test_operator_takes_far_views_uncopied_in_both_front_ends(bnhd, arena, ff, fm):
    """flash_attention forward and autograd backward on batch-far views of both memory layouts — BHND (head stride N * D, row pitch D) and BNHD (the
    heads of a row side by side: head stride D, row pitch H * D; the operator's argument is [B, N, H, D]) — through the compiled front end and the
    Python one: q, k, v reach the kernels un-copied (data_ptr), both front ends give identical bits, equal to the operator's on compact tensors of
    the same layout, and right against float64.  The operator allocates its outputs itself: the arena holds the
    inputs only and must be all poison once they are poisoned again."""
    from rocwmma_fattn import FlashAttn as fa
    case = _operator_case(bnhd)
    specs = [s for s in fl.dense_specs(case) if s[0] in ("q", "k", "v", "do")]
    slots = fl.place_bnhd([s[:3] for s in specs], gap=32768) if bnhd else fl.place(specs, "batch", gap=32768)
    for s in slots.values():
        assert s.strides[1:3] == ((case["D"], case["H"] * case["D"]) if bnhd else (case["Nq"] * case["D"], case["D"]))
    fl.validate(list(slots.values()), arena.numel())
    data = _inputs(case, slots, arena.device)
    fl.write_inputs(arena, slots, data)
    as_op = lambda t: t.transpose(1, 2) if bnhd else t                  # noqa: E731  the operator's BNHD argument is [B, N, H, D]
    V = {n: as_op(s.view(arena)) for n, s in slots.items()}
    C = {n: as_op(t).contiguous() if bnhd else t.clone() for n, t in data.items()}       # compact, the same layout: [B, N, H, D] / [B, H, N, D]
    assert all(C[n].stride()[1:] == V[n].stride()[1:] and C[n].is_contiguous() for n in C)
    D, flags = case["D"], CAUSAL | EXACT
    fe = fa._frontend()
    assert fe is not None or not os.path.exists(os.path.join(os.path.dirname(fa.__file__), "_fa2_frontend.so"))
    results = []
    for name, fwd, bwd in (("compiled", getattr(fe, "forward", None), getattr(fe, "backward", None)), ("python", fa.flash_attn_wmma.forward_py, fa.flash_attn_wmma.backward_py)):
        if fwd is None:
            continue
        for tensors in (V, C):
            ret = fwd(tensors["q"], tensors["k"], tensors["v"], 64, 128, flags, D ** -0.5, bnhd)
            if tensors is V:
                for i, n in enumerate(("q", "k", "v")):
                    assert ret[1 + i].data_ptr() == tensors[n].data_ptr() and ret[1 + i].stride() == tensors[n].stride(), (name, n, "was copied")
            n_ax = 1 if bnhd else 2
            grads = bwd(ret[1], ret[2], ret[3], ret[4], tensors["do"], ret[5], case["Nq"], case["Nkv"], D, 128, 128, True, D ** -0.5, bnhd)
            results.append([as_op(ret[0].narrow(n_ax, 0, case["Nq"])), ret[5][:, :, :case["Nq"]]] + [as_op(g) for g in grads])
    # autograd through flash_attention on the far views
    qg, kg, vg = (V[n].detach().requires_grad_(True) for n in ("q", "k", "v"))
    assert qg.data_ptr() == V["q"].data_ptr()
    o = fa.flash_attention(qg, kg, vg, causal=True, BNHD_fmt=bnhd)
    o.backward(V["do"])
    results.append([as_op(o.detach()), results[0][1], as_op(qg.grad), as_op(kg.grad), as_op(vg.grad)])
    torch.cuda.synchronize()
    for r in results[1:]:
        for a, b in zip(results[0], r):
            assert a.shape == b.shape and torch.equal(a, b)
    far = dict(zip(("o", "lse", "dq", "dk", "dv"), results[0]))
    got = fl.harvest(arena, slots)
    assert all(torch.equal(got[n], data[n]) for n in data)
    fails, live = _truth_dense(ff, case, far, data)
    assert not fails + fl.nan_in_live_rows(far, ("o", "lse", "dq", "dk", "dv")), fails


def test_operator_varlen_takes_row_far_views_uncopied(arena, ff):
    """flash_attention_varlen, forward and autograd backward, on the row-far views (grouped K / V): equal bits to the same call on contiguous copies,
    q / k / v un-copied (forward_varlen returns the tensors it ran on)."""
    from rocwmma_fattn import FlashAttn as fa
    case = dict(fl.PACKED_CASES[0], bwd=True)
    slots, _, _ = fl.packed_slots(case)
    slots = {n: slots[n] for n in ("q", "k", "v", "do")}
    fl.validate(list(slots.values()), arena.numel())
    dev, lens, dt = arena.device, fl.PACKED_LENS, fl.DTYPES[case["dt"]]
    lens_k = fl.PACKED_LENS_K
    total, total_k, cu, cu_k = sum(lens), sum(lens_k), _cu(lens, dev), _cu(lens_k, dev)
    g = torch.Generator(device="cpu").manual_seed(77)
    data = {n: torch.randn(slots[n].shape, generator=g).to(dt).to(dev) for n in slots}
    fl.write_inputs(arena, slots, data)
    V = {n: s.view(arena) for n, s in slots.items()}
    ret = fa.flash_attn_wmma.forward_varlen(V["q"], V["k"], V["v"], cu, cu_k, max(lens), max(lens_k), CAUSAL, case["D"] ** -0.5, (-1, -1))
    for i, n in enumerate(("q", "k", "v")):
        assert ret[1 + i].data_ptr() == V[n].data_ptr() and ret[1 + i].stride() == V[n].stride(), (n, "was copied")
    res = []
    for tensors in (V, {n: t.clone() for n, t in data.items()}):
        qg, kg, vg = (tensors[n].detach().requires_grad_(True) for n in ("q", "k", "v"))
        o = fa.flash_attention_varlen(qg, kg, vg, cu, cu_k, max_seqlen_q=max(lens), max_seqlen_k=max(lens_k), causal=True)
        o.backward(tensors["do"])
        res.append([o.detach()[:total], qg.grad[:total], kg.grad[:total_k], vg.grad[:total_k]])
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a, b) and not torch.isnan(a.float()).any()
    got = fl.harvest(arena, slots)
    assert all(torch.equal(got[n], data[n]) for n in data)
    for s in (5, 7):                                                     # a sequence that crosses 4 GiB and one that starts past it, against float64
        a, n, ak, nk = int(cu[s]), lens[s], int(cu_k[s]), lens_k[s]
        hm = lambda t: t[a:a + n].transpose(0, 1)                        # noqa: E731
        hk = lambda t: t[ak:ak + nk].transpose(0, 1)                     # noqa: E731
        band = ff.band(n, nk, -1, -1, 0, True, dev)
        keep = torch.ones((case["H"], n, nk), dtype=torch.bool, device=dev)
        ke, ve = (hk(data[x]).repeat_interleave(case["H"] // case["Hkv"], 0) for x in ("k", "v"))
        O, _, dQ, dK, dV = ff.ref64(hm(data["q"]), ke, ve, hm(data["do"]), keep, band, case["D"] ** -0.5, 0.0)
        eO, edQ, edK, edV = ff.emu(hm(data["q"]), ke, ve, hm(data["do"]), keep, band, case["D"] ** -0.5, 0.0, dt)
        for name, got_t, true, em, tol in (("o", res[0][0], O, eO, FLOOR[0]), ("dq", res[0][1], dQ, edQ, GRAD_TOL[0]),
                                           ("dk", res[0][2], ff.fold_groups(dK, case["Hkv"]), ff.fold_groups(edK, case["Hkv"]), GRAD_TOL[0]),
                                           ("dv", res[0][3], ff.fold_groups(dV, case["Hkv"]), ff.fold_groups(edV, case["Hkv"]), GRAD_TOL[0])):
            err, err_emu, bar = ff.error_and_bar((hk if name in ("dk", "dv") else hm)(got_t), true, em, tol)
            assert err <= bar, (s, name, err, bar)


# ---------------------------------------------------------------------------------------------------------------- f32 element indices past 2^31
def test_f32_tensors_at_element_indices_past_two_to_the_31(ff, fm):
    """Its own arena of 8 GiB + 256 MiB (same memory rule): LSE and delta with a batch stride of 2^30 + 3072 floats — batch 2 starts at float index
    2^31 + 6144 —, and an f32 bias with the same batch stride; forward and backward, the same checks.  Then the paged decode case with that batch
    stride: its lse, its descales (f32) and its block table (int32) pass element index 2^31 where b * stride is formed."""
    big = _arena(fl.ARENA_F32_BYTES)
    try:
        for case in fl.F32_CASES:
            slots, twin, tbytes = fl.dense_slots(case, step=fl.F32_STEP)
            _run_dense(case, big, slots, twin, _twin_arena(tbytes, big.device), ff, fm)
        case = fl.DECODE_F32_CASE
        for fmt in fl.DECODE_FORMATS:
            prep = _decode_prepare(case, fmt)
            for ns, where in ((1, "near"), (3, "near"), (3, "far")):
                _decode_run(case, fmt, big, prep, ns, where, step=fl.F32_STEP)
    finally:
        del big
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- KV-cache decode
DECODE_SPLITS = (1, 3, 0)          # 0: the plan's own choice


def _decode_dims(case):
    paged = case["layout"] == "paged"
    return (_code(case), case["B"], case["H"], case["Hkv"], case["Nq"], case["D"], fl.DECODE_NMAX // case["page"] if paged else case["nmax"], case["page"])


def _decode_plan(case, fmt, ns):
    """(plan, workspace bytes) of the case's call; the FP8 queries must answer like the 16-bit ones, and the case's kernel must be the planned one."""
    lib = _fa2_lib.load()
    plan, need = _fa2_lib.decode_plan(*_decode_dims(case), ns).as_dict(), lib.fa2_fwd_decode_workspace_bytes(*_decode_dims(case), ns)
    if fmt == "fp8":
        assert _fa2_lib.decode_fp8_plan(*_decode_dims(case), ns).as_dict() == plan and lib.fa2_fwd_decode_fp8_workspace_bytes(*_decode_dims(case), ns) == need
    assert plan["kernel"] == _fa2_lib.FA2_KERNEL_HIP_DECODE and plan["row_tiles"] == case["rt"], (plan, case["rt"])
    assert (need > 0) == (plan["nsplit"] > 1) and (ns == 0 or plan["nsplit"] == ns)
    return plan, need


def _decode_call(case, fmt, T, ns, need):
    """the C entry of the format on the slot views T (decode_calls.py has the argument order) -> its return code"""
    kw = dc.tensor_kw(T["q"], T["k"], T["v"], T["o"], T["lse"], T["lens"], T.get("bt"), T.get("kd"), T.get("vd"), scale=_scale(case))
    assert tuple(kw[n] for n in ("dtype", "B", "H", "Hkv", "Nq", "D", "cap", "page")) == _decode_dims(case)
    return dc.call("fp8" if fmt == "fp8" else "plain", **kw, ns=ns, ws=T["ws"].data_ptr() if need else None, wsb=need, stream=_stream())


def _decode_prepare(case, fmt):
    """CPU work of a (case, format), done once: the data, the block tables and the references (tests/decode_refs.py)."""
    data = fl.decode_inputs(case, fmt)
    tables = fl.decode_block_tables(case, fmt) if case["layout"] == "paged" else (None, None, None, None)
    if fmt == "fp8":
        refs = dr.refs_fp8(data["q"], data["k"], data["v"], data["kd"], data["vd"], case["lens"], _code(case))
    else:
        refs = dr.refs16(data["q"], data["k"], data["v"], case["lens"], _code(case))
    return data, tables, refs


def _decode_run(case, fmt, arena, prep, ns, ws_where, step=fl.FAR_STEP):
    """One call on the far views and on the twin, then every check of the module's docstring.  -> the far O and LSE (log2)."""
    t0 = time.perf_counter()
    data, (bt, bt_t, _, _), refs = prep
    plan, need = _decode_plan(case, fmt, ns)
    slots, twin, tbytes = fl.decode_slots(case, fmt, need, ws_where, step)
    fl.validate(list(slots.values()), arena.numel())                     # bounds before anything runs
    tarena = _twin_arena(tbytes, arena.device)
    fl.validate(list(twin.values()), tarena.numel())
    images = [fl.decode_images(case, fmt, sl, data, table) for sl, table in ((slots, bt), (twin, bt_t))]
    for ar, sl, img in ((arena, slots, images[0]), (tarena, twin, images[1])):
        for n, im in img.items():                                        # (o, lse and the workspace stay poison: NaN)
            sl[n].bytes_view(ar).copy_(im)
        _fa2_lib.check(_decode_call(case, fmt, {n: s.view(ar) for n, s in sl.items()}, ns, need))
    torch.cuda.synchronize()
    far, tw = fl.harvest(arena, slots), fl.harvest(tarena, twin)
    fails = []
    for got, img, who in ((far, images[0], "far"), (tw, images[1], "twin")):
        fails += fl.image_failures(got, img, who)
    fails += fl.compare_exact(far, tw, ["o", "lse"])
    print("%s %s: splits %d -> %s, workspace %d bytes %s, %.2f s" % (case["id"], fmt, ns, plan, need, ws_where if need else "-", time.perf_counter() - t0))
    assert not fails, fails
    dr.check(far["o"], far["lse"], refs, case["lens"], _code(case), (case["id"], fmt, ns, ws_where))
    return far["o"], far["lse"]


@pytest.mark.parametrize("fmt", fl.DECODE_FORMATS)
@pytest.mark.parametrize("case", fl.DECODE_CASES, ids=lambda c: c["id"])
def test_decode_far_caches(case, fmt, arena):
    """fa2_fwd_decode and fa2_fwd_decode_fp8 (tests/far_layouts.py: DECODE_CASES) on caches whose batches, K / V heads, key rows or pages lie past byte
    offsets 2^31 and 2^32 — e4m3 caches: past ELEMENT index 2^31 and 2^32 too —, the block table's rows and the descales far as well: one part, three
    parts and the plan's own split, a split's workspace (pre-filled with NaN) once near the arena's start and once past 4 GiB.  The twin of a paged
    case is a small pool with its own page numbering: O and LSE must still match bit for bit.  Truth: tests/decode_refs.py (the oracle per sequence
    and float64, the bars of tests/test_decode_gpu.py).  Rows at or beyond a length, unused pages and the page that the block table's unused entries
    name are poison before and after."""
    prep = _decode_prepare(case, fmt)
    seen = set()
    for ns in DECODE_SPLITS:
        for where in (("near", "far") if _decode_plan(case, fmt, ns)[1] else ("near",)):
            _decode_run(case, fmt, arena, prep, ns, where)
            seen.add((ns, where))
    assert {(3, "near"), (3, "far"), (1, "near")} <= seen


@pytest.mark.parametrize("fmt", fl.DECODE_FORMATS)
@pytest.mark.parametrize("case", [fl.DECODE_CASES[1], fl.DECODE_CASES[6]], ids=lambda c: c["id"])
def test_operator_decode_takes_far_caches_uncopied(case, fmt, arena):
    """flash_attention_decode on the batch-far and on the paged views, 16-bit and e4m3 caches: the C call's O bits (the plan's own split) and its LSE,
    and — the operator allocates o, lse and the workspace itself — an arena that is all poison once the inputs are poisoned again: no cache was
    copied into it, nothing was written beside them."""
    from rocwmma_fattn import FlashAttn as fa
    prep = _decode_prepare(case, fmt)
    o, lse = _decode_run(case, fmt, arena, prep, 0, "near")
    slots = {n: s for n, s in fl.decode_slots(case, fmt)[0].items() if n not in ("o", "lse")}
    fl.validate(list(slots.values()), arena.numel())
    images = fl.decode_images(case, fmt, slots, prep[0], prep[1][0])
    for n, im in images.items():
        slots[n].bytes_view(arena).copy_(im)
    V = {n: s.view(arena) for n, s in slots.items()}
    assert fa._decode_strides_ok(V["q"]) and V["lens"].is_contiguous()   # (the operator copies a q it cannot pass on; a cache it cannot pass on raises)
    po, pl = fa.flash_attention_decode(V["q"], V["k"], V["v"], V["lens"], block_table=V.get("bt"), return_lse=True, k_descale=V.get("kd"), v_descale=V.get("vd"))
    torch.cuda.synchronize()
    assert torch.equal(po.view(torch.int16), o.view(torch.int16)) and dr.same_lse(pl * 1.4426950408889634, lse)
    got = fl.harvest(arena, slots)
    assert not fl.image_failures(got, images)


# ---------------------------------------------------------------------------------------------------------------- merge of partial results
def _merge_calls(case, T):
    """fa2_merge_fwd, then fa2_merge_bwd on the tensors T."""
    lib, n = _fa2_lib.load(), fl.MERGE_PARTS
    if case["layout"] == "packed":
        geo = (1, case["H"], case["Nq"], case["D"])
        s3, s2 = (lambda t: _fa2_lib.strides3(0, t.stride(1), t.stride(0))), (lambda t: _fa2_lib.strides2(0, t.stride(0)))
    else:
        geo = (case["B"], case["H"], case["Nq"], case["D"])
        s3, s2 = _s3, _s2
    arr = lambda fmt: (ctypes.c_void_p * n)(*(T[fmt % k].data_ptr() for k in range(n)))      # noqa: E731
    for k in range(1, n):                                               # one stride set for all parts
        assert T["o%d" % k].stride() == T["o0"].stride() and T["l%d" % k].stride() == T["l0"].stride() and T["do%d" % k].stride() == T["do0"].stride()
    flags = _fa2_lib.FA2_MERGE_NATURAL_LSE if case["natural"] else 0
    _fa2_lib.check(lib.fa2_merge_fwd(_code(case), n, arr("o%d"), arr("l%d"), T["o"].data_ptr(), T["lse"].data_ptr(), *geo, s3(T["o0"]), s2(T["l0"]), s3(T["o"]),
                                     s2(T["lse"]), flags, _stream()))
    _fa2_lib.check(lib.fa2_merge_bwd(_code(case), n, arr("o%d"), arr("l%d"), T["lse"].data_ptr(), T["dout"].data_ptr(), T["dlse"].data_ptr(), arr("do%d"), arr("dl%d"),
                                     *geo, s3(T["o0"]), s2(T["l0"]), s2(T["lse"]), s3(T["dout"]), s2(T["dlse"]), s3(T["do0"]), s2(T["dl0"]), flags, _stream()))


@pytest.mark.parametrize("case", fl.MERGE_CASES, ids=lambda c: c["id"])
def test_merge_far_parts(case, arena):
    """fa2_merge_fwd and fa2_merge_bwd (tests/far_layouts.py: MERGE_CASES) on three parts that share one far stride set — batches or heads FAR_STEP apart,
    the packed calling form with rows 1 MiB apart, and compact parts whose bases lie at the arena's start, past 2^31 and past 2^32 —, with o, lse,
    dout, dlse and the parts' gradients far too.  Rows of weight 0 in part 1 keep poison in that part's O: they are never read, so the merged O and
    every gradient are finite.  Truth: the float64 merge and its autograd under tests/test_merge_gpu.py's bars (lse_refs.merge_check)."""
    t0 = time.perf_counter()
    slots, twin, tbytes = fl.merge_slots(case)
    fl.validate(list(slots.values()), arena.numel())
    tarena = _twin_arena(tbytes, arena.device)
    fl.validate(list(twin.values()), tarena.numel())
    data = fl.merge_inputs(case)
    images = fl.merge_images(case, slots, data)
    for ar, sl in ((arena, slots), (tarena, twin)):
        for n, im in images.items():
            sl[n].bytes_view(ar).copy_(im)
        _merge_calls(case, {n: s.view(ar) for n, s in sl.items()})
    torch.cuda.synchronize()
    far, tw = fl.harvest(arena, slots), fl.harvest(tarena, twin)
    outs = [n for n in slots if n not in fl.MERGE_INPUTS]
    fails = fl.image_failures(far, images, "far") + fl.image_failures(tw, images, "twin") + fl.compare_exact(far, tw, outs) + fl.nan_in_live_rows(far, outs)
    print("%s: %.2f s" % (case["id"], time.perf_counter() - t0))
    assert not fails, fails
    cpu = {n: fl.merge_as_slot(case, far[n].cpu()) for n in outs}        # [B, H, Nq, D] / [B, H, Nq]
    assert torch.isfinite(cpu["o"].float()).all()
    parts = range(fl.MERGE_PARTS)
    R.merge_check(case["id"], fl.DTYPES[case["dt"]], case["natural"], [data["o%d" % k] for k in parts], [data["l%d" % k] for k in parts], data["dout"], data["dlse"],
                  cpu["o"], cpu["lse"], [cpu["do%d" % k] for k in parts], [cpu["dl%d" % k] for k in parts])
