"""64-bit addressing on the GPU: every tensor of a call — inputs, outputs, LSE, the delta workspace, a split's workspace — is a strided view into one
poisoned 4.25 GiB buffer, placed so that batch, head or row strides carry slices past byte offsets 2^31 and 2^32, or so that one head's span sits on
or beyond the documented limits (tests/far_layouts.py has the layouts, tests/test_far_offsets.py proves on the CPU that they cross what they claim).

Per case: the call runs on the far views and on a compact twin (same shapes, row pitches and data; span cases: the same pitch, the base moved);
where a plan query exists both must get the same plan, and the intended kernel; O, LSE, dQ, dK, dV (and delta) must be bitwise equal — the library is
deterministic, a tolerance would hide an off-by-one-slice read; the far outputs are held to dense float64 attention under tests/conftest.py's bars
(tools/fuzz_features.py's references and bar rule; tools/fuzz_mask.py's for the biased calls), so that twin and far cannot be wrong together; no
output row with a visible key holds a NaN; the inputs are unchanged; and after the views are poisoned again the whole arena is poison: nothing was
written outside the outputs.

The module skips — its only skip — when the device has less free memory than the arena plus 2 GiB."""
import ctypes
import importlib.util
import math
import os
import time

import pytest
import torch

import far_layouts as fl
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
    _fa2_lib.check(_fa2_lib.load().fa2_bwd_plan(_code(case), case["B"], case["H"], case["Hkv"], case["Nq"], case["Nkv"], case["D"],
                                                *[_s3(T[n]) for n in ("q", "k", "v", "o", "do")], _scale(case), CAUSAL if case["causal"] else 0, kind, bstr,
                                                ctypes.byref(plan)))
    return plan.dq_kernel, plan.dkv_kernel


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
    if case["fam"] == "dense":
        if Hkv == H and "ws" not in T:
            return lib.fa2_bwd, (dt, *ptrs, B, H, Nq, Nkv, D, *tail, _stream())
        return lib.fa2_bwd_gqa, (dt, *ptrs, B, H, Hkv, Nq, Nkv, D, *tail, *_ws(T), _stream())
    assert Hkv == H                                                     # (the windowed, dropout and biased backwards are multi-head calls)
    if case["fam"] == "window":
        return lib.fa2_bwd_window, (dt, *ptrs, B, H, Nq, Nkv, D, *tail, *_window(case), _stream())
    if case["fam"] == "dropout":
        return lib.fa2_bwd_dropout, (dt, *ptrs, B, H, Nq, Nkv, D, *tail, *_window(case), _stream(), case["p"], case["seed"])
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
    fails = ["input %s was written" % n for n in data if not torch.equal(far[n], data[n])]
    fails += fl.compare_exact(far, tw, outs)
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
            for c in families:
                if case["bwd"]:
                    fn, args = _bwd_args(c, T, (name, 8))
                    assert fn(*args) == shape, (name, c["fam"])
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


# ---------------------------------------------------------------------------------------------------------------- packed, row-far
def _cu(lens, dev):
    return torch.tensor([0] + [sum(lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32, device=dev)


def _packed_call(case, T, cu, cu_k, fwd):
    lib, dt = _fa2_lib.load(), _code(case)
    H, Hkv, D, B, mq, mk = case["H"], case["Hkv"], case["D"], len(fl.PACKED_LENS), max(fl.PACKED_LENS), max(fl.PACKED_LENS_K)
    s2 = lambda t: _fa2_lib.strides2(t.stride(1), t.stride(0))          # noqa: E731  {head, row}
    flags = (CAUSAL if case["causal"] else 0) | (BOTTOM_RIGHT if case["bottom_right"] else 0) | (EXACT if case["bwd"] and fwd else 0)
    drop = (case["p"], case["seed"]) if case["p"] > 0 else ()
    if fwd:
        fn = lib.fa2_fwd_varlen_dropout if drop else lib.fa2_fwd_varlen
        return fn(dt, *[T[n].data_ptr() for n in ("q", "k", "v", "o", "lse")], B, H, Hkv, mq, mk, D, cu.data_ptr(), cu_k.data_ptr(),
                  *[s2(T[n]) for n in ("q", "k", "v", "o")], T["lse"].stride(0), D ** -0.5, flags, -1, -1, _stream(), *drop)
    assert T["delta"].stride() == T["lse"].stride() and H == Hkv
    fn = lib.fa2_bwd_varlen_dropout if drop else lib.fa2_bwd_varlen
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
    T, Tt = {n: s.view(arena) for n, s in slots.items()}, {n: s.view(tarena) for n, s in twin.items()}
    for tensors in (T, Tt):                                             # only the rows of the sequences are written: the rest stays poison
        for n, t in data.items():
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
    fails = ["input %s was written" % n for n in data if not torch.equal(far[n][:used[n]], data[n][:used[n]])]
    poison16 = torch.full((), -1, dtype=torch.int16, device=dev)
    for n in far:                                                       # rows behind cu[B]: untouched, in inputs and outputs alike
        tail = far[n][:, used[n]:] if n in ("lse", "delta") else far[n][used[n]:]
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
    2^31 + 6144 —, and an f32 bias with the same batch stride; forward and backward, the same checks."""
    big = _arena(fl.ARENA_F32_BYTES)
    try:
        for case in fl.F32_CASES:
            slots, twin, tbytes = fl.dense_slots(case, step=fl.F32_STEP)
            _run_dense(case, big, slots, twin, _twin_arena(tbytes, big.device), ff, fm)
    finally:
        del big
        torch.cuda.empty_cache()
