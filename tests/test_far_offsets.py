"""64-bit addressing, the parts that need no GPU (tests/test_far_offsets_gpu.py runs the calls): the layouts of tests/far_layouts.py really cross byte
offsets 2^31 and 2^32 (built on device "meta"), the checker flags every mutant it is there for, and the library's validation and plan sit exactly on
the documented span limits ("addressing limits"; include/fa2_gfx950.h) — null tensors and queries only, nothing touches a device.

The dense launching entry points report a null tensor before they look at a span (the order of the checks is part of the C-ABI, tests/test_abi_golden.py),
so their edges are pinned through the plan queries, which run the same validation on the same call description (fa2_fwd_plan and its grouped and
windowed twins; fa2_bwd_plan); the packed entry points check their tensors last and show the edge themselves.  tests/test_far_offsets_gpu.py
repeats the refusals through the launching entry points, on real tensors.

The decode, merge, score-modifier and LSE-gradient layouts are proved here too (what crosses byte 2^31 and 2^32, which e4m3 caches pass element
index 2^31, that a wide-row cache's invalid keys stay inside the arena, that every paged sequence takes a page of each region), their checkers are
fed mutants — an output built from the neighbouring page id, the key at index len included, a write into a poison page, a row merged from the wrong
part's base, a gradient that ignored dlse —, and the packed score-modifier and LSE entry points and fa2_bwd_lse_plan sit on the span edges of the
calls they extend.  The decode call documents no span limit; its plan and workspace queries take sizes only and are asserted per case."""
import ctypes
import re

import numpy as np
import pytest
import torch

import far_layouts as fl
from conftest import ROOT
from rocwmma_fattn import _fa2_lib

P31, P32 = 1 << 31, 1 << 32


def _codes():
    text = open(ROOT + "/include/fa2_gfx950.h").read()
    return {m[0]: int(m[1]) for m in re.findall(r"#define\s+(FA2_\w+)\s+(-?\d+)", text)}


# ---------------------------------------------------------------------------------------------------------------- the layouts
def _meta_views(slots, nbytes):
    arena = torch.empty(nbytes, dtype=torch.uint8, device="meta")
    for s in slots.values():
        v = s.view(arena)
        assert tuple(v.shape) == s.shape and tuple(v.stride()) == s.strides and v.storage_offset() * s.esize == s.offset
        assert tuple(s.bytes_view(arena).shape)[-1] == s.row_bytes()


def _crosses(slot, dim, lo):
    """Some slice along `dim` starts a little past lo — by 12 or 24 KiB plus what the tensors placed before it take, never by a round number — and another one below lo."""
    starts = [slot.slice_range(dim, i)[0] for i in range(slot.shape[dim])]
    hit = [a for a in starts if lo < a < lo + 64 * fl.MIB and a % (1 << 16) != 0]
    return bool(hit) and min(starts) < lo


@pytest.mark.parametrize("case", fl.DENSE_CASES, ids=lambda c: c["id"])
def test_dense_layouts_cross_both_thresholds_inside_the_arena(case):
    need = 3 << 20 if case["ws"] else 0
    slots, twin, tbytes = fl.dense_slots(case, need)
    fl.validate(list(slots.values()), fl.ARENA_BYTES)
    fl.validate(list(twin.values()), tbytes)
    _meta_views(slots, fl.ARENA_BYTES)
    _meta_views(twin, tbytes)
    dim = 0 if case["far"] == "batch" else 1
    for name, s in slots.items():
        if name == "ws":
            assert (s.offset > P32) == (case["ws"] == "far")
            continue
        d = 0 if name == "bias" else dim
        starts = [s.slice_range(d, i)[0] for i in range(s.shape[d])]
        assert _crosses(s, d, P32), (name, starts)
        # (the six Q heads of a grouped head-far call share the arena at equal steps: one of them lies between the thresholds, not right behind 2^31)
        assert _crosses(s, d, P31) if s.shape[d] == 3 else any(P31 < a < P32 for a in starts), (name, starts)
        t = twin[name]
        assert t.shape == s.shape and t.strides[2:] == s.strides[2:]            # same row pitch
        assert t.strides[1] == (s.shape[2] * s.strides[2] if len(s.shape) == 4 else s.shape[2])      # heads and batches contiguous
        assert t.strides[0] == s.shape[1] * t.strides[1]
    if case["Hkv"] != case["H"] and case["far"] == "head":
        assert case["Hkv"] == 3 and case["H"] == 6               # the K / V heads of a grouped call are far too


@pytest.mark.parametrize("case", fl.F32_CASES, ids=lambda c: c["id"])
def test_f32_layouts_pass_element_index_two_to_the_31(case):
    slots, twin, tbytes = fl.dense_slots(case, step=fl.F32_STEP)
    fl.validate(list(slots.values()), fl.ARENA_F32_BYTES)
    _meta_views(slots, fl.ARENA_F32_BYTES)
    f32 = [s for s in slots.values() if s.dtype == torch.float32]
    assert {s.name for s in f32} >= ({"lse", "delta"} | ({"bias"} if case["bias"] else set()))
    for s in f32:
        first = [s.slice_range(0, b)[0] // 4 for b in range(3)]                  # float index of each batch's first element
        assert first[0] < P31 // 4 and P31 // 2 < first[1] < P31 and P31 < first[2] < P31 + 16 * fl.MIB, (s.name, first)
        assert 2 * s.strides[0] > P31                                            # ... and b * stride[0] itself leaves 31 bits


@pytest.mark.parametrize("case", fl.PACKED_CASES, ids=lambda c: c["id"])
def test_packed_layout_starts_sequences_past_both_thresholds(case):
    slots, twin, tbytes = fl.packed_slots(case)
    fl.validate(list(slots.values()), fl.ARENA_BYTES)
    fl.validate(list(twin.values()), tbytes)
    _meta_views(slots, fl.ARENA_BYTES)
    lens = fl.PACKED_LENS
    bases = np.concatenate([[0], np.cumsum(lens)])
    assert bases[-1] < fl.PACKED_TOTAL and max(lens) == 1500 and 0 in lens and 1 in lens
    pitch = fl.PACKED_PITCH_BYTES
    assert pitch == 2 * (1 << 19)
    for name in ("q", "k", "v", "o"):
        s = slots[name]
        assert s.strides[0] * s.esize == pitch
        starts = [s.offset + int(b) * pitch for b in bases[:-1]]
        assert sum(a > P32 for a in starts) >= 2 and any(P31 < a < P32 for a in starts) and starts[0] < P31
        # a sequence that straddles each threshold: base * pitch below it, its last row beyond
        for lim in (P31, P32):
            assert any(a < lim < a + n * pitch for a, n in zip(starts, lens)), (name, lim)
    # every sequence's own span obeys the documented rule (the stated maximum is what the library is told)
    assert fl.span_bytes(max(lens), pitch // 2, case["D"]) + fl.SPAN_SLACK_ROWS * pitch <= fl.SPAN_LIMIT
    assert slots["lse"].offset > P32
    # K / V: lengths of their own — other bases, fewer and more keys than queries — with the same crossings
    lens_k = fl.PACKED_LENS_K
    bases_k = np.concatenate([[0], np.cumsum(lens_k)])
    assert len(lens_k) == len(lens) and bases_k[-1] < fl.PACKED_TOTAL and max(lens_k) <= max(lens)
    assert any(nk < n for n, nk in zip(lens, lens_k)) and any(nk > n for n, nk in zip(lens, lens_k)) and all((n == 0) == (nk == 0) for n, nk in zip(lens, lens_k))
    assert sum(int(a) != int(b) for a, b in zip(bases[:-1], bases_k[:-1])) >= 3
    for name in ("k", "v"):
        starts = [slots[name].offset + int(b) * pitch for b in bases_k[:-1]]
        assert sum(a > P32 for a in starts) >= 2 and any(P31 < a < P32 for a in starts) and starts[0] < P31
        for lim in (P31, P32):
            assert any(a < lim < a + n * pitch for a, n in zip(starts, lens_k)), (name, lim)


@pytest.mark.parametrize("case", fl.SPAN_CASES, ids=lambda c: c["id"])
def test_span_layouts_sit_where_they_claim(case):
    slots, twin = fl.span_slots(case)
    fl.validate(list(slots.values()) + list(twin.values()), fl.ARENA_BYTES)
    _meta_views(slots, fl.ARENA_BYTES)
    pitch = fl.span_pitch_bytes(case) // 2
    for name in case["wide"]:
        s, t = slots[name], twin[name]
        n = s.shape[2]
        assert s.strides[2] == pitch == t.strides[2] and t.offset != s.offset and abs(t.offset - s.offset) < 65536          # the twin: the base moved
        span = fl.span_bytes(n, pitch, case["D"])
        assert s.extent()[1] - s.extent()[0] == span
        if case["pitch"] == "limit":
            assert span + fl.SPAN_SLACK_ROWS * pitch * 2 <= fl.SPAN_LIMIT < fl.span_bytes(n, pitch + 8, case["D"]) + fl.SPAN_SLACK_ROWS * (pitch + 8) * 2
            assert s.extent()[0] > P31 and s.extent()[1] > P32                   # ... and the base is far
        elif case["pitch"] == "limit128":                                          # the 128-row kernel's rule, a ragged Nq: waves wholly past Nq
            Nq = case["Nq"]
            assert n == Nq and ((Nq + 128) * pitch + 256) * 2 < P32 <= ((Nq + 128) * (pitch + 8) + 256) * 2 and span > P31
            rows_past = (Nq - 1) // 128 * 128 + 96 + 31 - (Nq - 1)                 # the last workgroup's last wave's last row, past row Nq - 1
            assert 1 <= Nq % 128 <= 64 and rows_past >= 96 and ((Nq - 1 + rows_past) * pitch + 256) * 2 < P32
            assert ((Nq - 1 + rows_past) * pitch) * 2 >= ((Nq + 32) * pitch + 256) * 2       # ... far more than one wave's 32 rows past Nq
        elif case["pitch"] == "limit_trim":                                        # the 256-row bodies' rule at a head dim below the body's
            Nq, D = case["Nq"], case["D"]
            assert ((Nq + 64) * pitch + D) * 2 < P31 <= ((Nq + 64) * (pitch + 8) + D) * 2 and D < 128
            assert s.extent()[0] > P31 and s.extent()[1] > P32
        elif case["pitch"] == fl.SPAN_PITCH_3G:
            assert P31 <= span < P32 and fl.span_bytes(n + 64, pitch, case["D"]) < P32
        else:
            assert span > P32
    for name, s in slots.items():
        if name not in case["wide"] and len(s.shape) == 4:
            assert s.strides[2] == case["D"]


@pytest.mark.parametrize("case", fl.BIAS_SPAN_CASES, ids=lambda c: c["id"])
def test_bias_span_layout_is_the_last_accepted_slice(case):
    slots, twin = fl.bias_span_slots(case)
    fl.validate(list(slots.values()) + list(twin.values()), fl.ARENA_BYTES)
    _meta_views(slots, fl.ARENA_BYTES)
    pitch, (Nq, Nkv), es = slots["bias"].strides[2], (case["Nq"], case["Nkv"]), slots["bias"].esize
    gran = 16 // es
    rule = lambda p: ((Nq - 1) * p + Nkv + 64 * p) * es                           # noqa: E731
    last = pitch - case["pitch_step"] * gran
    assert rule(last) < fl.SPAN_LIMIT <= rule(last + gran) and last % gran == 0 and last == fl.last_bias_pitch(Nq, Nkv, es) and twin["bias"].strides == slots["bias"].strides
    assert case["pitch_step"] in (0, 1) and (rule(pitch) < fl.SPAN_LIMIT) == (case["pitch_step"] == 0)
    assert slots["bias"].extent()[0] > P31 and slots["bias"].extent()[1] > P32
    if case["form"] == "tile_dma" or case["pitch_step"]:                          # a grid past 3/8 of the MI355X's 256 CUs, 256-row workgroups
        assert case["B"] * case["H"] * -(-Nq // 256) > 256 * 3 // 8


def test_bnhd_placement_puts_the_heads_of_a_row_side_by_side():
    specs = [(n, torch.float16, (3, 2, 320, 64)) for n in ("q", "k", "v", "do")]
    slots = fl.place_bnhd(specs, gap=32768)
    fl.validate(list(slots.values()), fl.ARENA_BYTES)
    _meta_views(slots, fl.ARENA_BYTES)
    arena = torch.empty(fl.ARENA_BYTES, dtype=torch.uint8, device="meta")
    for s in slots.values():
        assert s.strides == (fl.FAR_STEP // 2, 64, 128, 1) and _crosses(s, 0, P31) and _crosses(s, 0, P32)
        v = s.view(arena).transpose(1, 2)                                         # the operator's [B, N, H, D] argument
        assert tuple(v.shape) == (3, 320, 2, 64) and v[0].is_contiguous() and v.stride(0) == fl.FAR_STEP // 2


# ---------------------------------------------------------------------------------------------------------------- the checker and its mutants
def _small_case():
    """A far layout in miniature: 3 batches 256 KiB apart in a 1 MiB arena, o / lse outputs, on the CPU."""
    step = 256 * 1024 + 3 * 64
    specs = [("q", torch.float16, (3, 2, 16, 8), 8), ("o", torch.float16, (3, 2, 16, 8), 8), ("lse", torch.float32, (3, 2, 16), None)]
    slots = fl.place(specs, "batch", step=step, gap=64)
    fl.validate(list(slots.values()), 1 << 20)
    arena = fl.new_arena(1 << 20, "cpu")
    g = torch.Generator().manual_seed(1)
    data = {"q": torch.randn((3, 2, 16, 8), generator=g).half()}
    fl.write_inputs(arena, slots, data)
    result = {"o": torch.randn((3, 2, 16, 8), generator=g).half(), "lse": torch.randn((3, 2, 16), generator=g)}
    return arena, slots, data, result


def _kernel(arena, slots, result):
    for n, t in result.items():
        slots[n].view(arena).copy_(t)


def _check(arena, slots, twin_out, live=None):
    out = fl.harvest(arena, slots)
    return out, fl.compare_exact(out, twin_out, ("o", "lse")) + fl.nan_in_live_rows(out, ("o", "lse"), live)


def test_checker_passes_the_clean_case_and_leaves_the_arena_poisoned():
    arena, slots, data, result = _small_case()
    assert not fl.arena_is_poison(arena)                        # the inputs are in it
    _kernel(arena, slots, result)
    out, fails = _check(arena, slots, result)
    assert not fails and torch.equal(out["q"], data["q"]) and fl.arena_is_poison(arena)
    assert torch.isnan(slots["o"].view(arena).float()).all() and torch.isnan(slots["lse"].view(arena)).all()       # poison reads as NaN in fp16 and f32
    assert torch.isnan(slots["q"].view(arena).view(torch.bfloat16).float()).all()                                  # ... and in bf16


def test_checker_flags_one_changed_element():
    arena, slots, data, result = _small_case()
    bad = {n: t.clone() for n, t in result.items()}
    bad["o"][2, 1, 7, 3] += 2.0 ** -10
    _kernel(arena, slots, bad)
    _, fails = _check(arena, slots, result)
    assert len(fails) == 1 and "o: 1 elements differ" in fails[0] and "(2, 1, 7, 3)" in fails[0]
    bad = {n: t.clone() for n, t in result.items()}
    bad["lse"][1, 0, 15] = torch.nextafter(bad["lse"][1, 0, 15], torch.tensor(9.0))
    _kernel(arena, slots, bad)
    _, fails = _check(arena, slots, result)
    assert len(fails) == 1 and fails[0].startswith("lse:")


def test_checker_flags_a_row_taken_from_the_neighbouring_slice():
    arena, slots, data, result = _small_case()
    bad = {n: t.clone() for n, t in result.items()}
    bad["o"][1, 0, 5] = result["o"][2, 0, 5]                     # what a base computed with the wrong batch would store
    _kernel(arena, slots, bad)
    _, fails = _check(arena, slots, result)
    assert len(fails) == 1 and "first at (1, 0, 5, 0)" in fails[0]


def test_checker_flags_one_poison_byte_overwritten_outside_the_views():
    for where in ("between", "end"):
        arena, slots, data, result = _small_case()
        _kernel(arena, slots, result)
        at = slots["o"].slice_range(0, 1)[1] + 3 if where == "between" else arena.numel() - 1      # the gap behind a slice / the arena's last byte
        arena[at] = 0xFE
        with pytest.raises(AssertionError, match="arena offset %d " % at):
            fl.harvest(arena, slots)
        assert fl.arena_is_poison(arena)                         # (left clean for the next case)
    # a write into ANOTHER view of the case is caught by the comparison of that view (inputs are compared with what was written)
    arena, slots, data, result = _small_case()
    _kernel(arena, slots, result)
    slots["q"].view(arena)[2, 1, 3, 0] = 1.0
    assert not torch.equal(fl.harvest(arena, slots)["q"], data["q"])


def test_checker_flags_a_nan_in_a_live_row_and_ignores_dead_rows():
    arena, slots, data, result = _small_case()
    bad = {n: t.clone() for n, t in result.items()}
    bad["o"][0, 1, 4, 2] = float("nan")
    live = torch.ones((3, 2, 16), dtype=torch.bool)
    _kernel(arena, slots, bad)
    _, fails = _check(arena, slots, bad, live)
    assert fails == ["o: NaN in a live row, first at (0, 1, 4, 2)"]
    live[0, 1, 4] = False                                        # the same row declared dead: not this check's business
    _kernel(arena, slots, bad)
    assert not _check(arena, slots, bad, live)[1]
    # a stray read shows as exactly this: poison that reached an output
    bad["o"][0, 1, 4] = torch.full((8,), -1, dtype=torch.int16).view(torch.float16)
    _kernel(arena, slots, bad)
    assert _check(arena, slots, bad)[1]


def test_first_stray_byte_scans_in_chunks():
    arena = fl.new_arena(1 << 16, "cpu")
    assert fl.first_stray_byte(arena, chunk=4096) is None
    arena[4096 * 7 + 5] = 0
    assert fl.first_stray_byte(arena, chunk=4096) == 4096 * 7 + 5 and not fl.arena_is_poison(arena)


# ---------------------------------------------------------------------------------------------------------------- the library's edges
def test_last_pitch_is_the_documented_rule():
    for n, D in ((192, 64), (77, 128), (1500, 64), (2 ** 21 - 128, 64)):
        p = fl.last_pitch(n, D)
        assert p % 8 == 0 and fl.span_bytes(n, p, D) + 64 * p * 2 <= fl.SPAN_LIMIT < fl.span_bytes(n, p + 8, D) + 64 * (p + 8) * 2


def _s3(pitch, n):
    return _fa2_lib.strides3(n * pitch, n * pitch, pitch)


def test_forward_plan_queries_sit_on_the_kv_span_edge():
    """fa2_fwd_plan, fa2_fwd_gqa_plan and fa2_fwd_window_plan (windowed, and as the dropout calls' validation: same call description): the last K
    pitch of the documented rule is planned, the next one refused (the queries describe V with K's strides)."""
    lib, c, plan = _fa2_lib.load(), _codes(), _fa2_lib.FwdPlan()
    po = ctypes.byref(plan)
    for dt, Nq, Nkv, D in ((0, 320, 192, 64), (1, 64, 8192, 128), (0, 256, 77, 64), (1, 192, 300, 512), (0, 384, 384, 160)):
        good = fl.last_pitch(Nkv, D)
        qs = _s3(D, Nq)
        for pitch, want in ((good, 0), (good + 8, c["FA2_ERR_BAD_SHAPE"])):
            ks = _s3(pitch, Nkv)
            assert lib.fa2_fwd_plan(dt, 1, 2, Nq, Nkv, D, qs, ks, 0.125, 0, 0, 0, po) == want, (Nkv, D, pitch)
            assert lib.fa2_fwd_gqa_plan(dt, 1, 2, 1, Nq, Nkv, D, qs, ks, 0.125, 1, 0, po) == want
            assert lib.fa2_fwd_window_plan(dt, 1, 2, 1, Nq, Nkv, D, qs, ks, 0.125, 0, 100, 0, 64, 0, po) == want
            if D <= 256:
                assert lib.fa2_fwd_plan(dt, 1, 2, Nq, Nkv, D, qs, ks, 0.125, 0, _fa2_lib.FA2_BIAS_F32, 0, po) == want
        # Q is not bounded in the forward: a Q span past 4 GiB is planned (on the compiler-scheduled kernels)
        assert lib.fa2_fwd_plan(dt, 1, 2, Nq, Nkv, D, _s3(1 << 24, Nq), _s3(D, Nkv), 0.125, 0, 0, 0, po) == 0
        assert plan.kernel in (_fa2_lib.FA2_KERNEL_HIP_128, _fa2_lib.FA2_KERNEL_HIP_256)


def _bwd_plan(lib, dt, B, H, Hkv, Nq, Nkv, D, st=None, flags=0, bias_kind=0, bias_strides=None):
    """fa2_bwd_plan -> (return code, dq kernel, dkv kernel); st: {tensor: strides3} of the tensors that are not contiguous."""
    st, plan = st or {}, _fa2_lib.BwdPlan()
    rc = lib.fa2_bwd_plan(dt, B, H, Hkv, Nq, Nkv, D, *[st.get(n) for n in ("q", "k", "v", "o", "do")], D ** -0.5, flags, bias_kind, bias_strides, ctypes.byref(plan))
    return rc, plan.dq_kernel, plan.dkv_kernel


def test_backward_plan_query_sits_on_the_span_edge_of_every_bounded_tensor():
    """fa2_bwd_plan validates like fa2_bwd / fa2_bwd_ws / fa2_bwd_gqa / fa2_bwd_bias (one call description, one validation): Q, dO, K and V each on the
    last pitch of the documented rule are planned, the next pitch is FA2_ERR_BAD_SHAPE; so is the bias slice of the masked backward.  O is never
    refused."""
    lib, c = _fa2_lib.load(), _codes()
    shape = c["FA2_ERR_BAD_SHAPE"]
    for dt, H, Hkv, Nq, Nkv, D in ((0, 2, 2, 192, 192, 64), (1, 4, 2, 320, 77, 128), (0, 2, 1, 192, 300, 512)):
        for which in ("q", "do", "k", "v"):
            n = Nq if which in ("q", "do") else Nkv
            good = fl.last_pitch(n, D)
            assert _bwd_plan(lib, dt, 1, H, Hkv, Nq, Nkv, D, {which: _s3(good, n)})[0] == 0, (which, D)
            assert _bwd_plan(lib, dt, 1, H, Hkv, Nq, Nkv, D, {which: _s3(good + 8, n)})[0] == shape, (which, D)
            for has_dlse in (0, 1):                                     # fa2_bwd_lse's own query: the same validation, with and without a dlse
                plan = _fa2_lib.BwdPlan()
                st = lambda p: [{which: _s3(p, n)}.get(t) for t in ("q", "k", "v", "o", "do")]      # noqa: E731
                assert lib.fa2_bwd_lse_plan(dt, 1, H, Hkv, Nq, Nkv, D, *st(good), D ** -0.5, 0, 0, None, has_dlse, ctypes.byref(plan)) == 0
                assert lib.fa2_bwd_lse_plan(dt, 1, H, Hkv, Nq, Nkv, D, *st(good + 8), D ** -0.5, 0, 0, None, has_dlse, ctypes.byref(plan)) == shape
            if Hkv == H and D <= 256:        # the masked backward: the same tensors, and its own slice rule
                assert _bwd_plan(lib, dt, 1, H, Hkv, Nq, Nkv, D, {which: _s3(good + 8, n)}, bias_kind=_fa2_lib.FA2_BIAS_BOOL)[0] == shape
        assert _bwd_plan(lib, dt, 1, H, Hkv, Nq, Nkv, D, {"o": _s3(1 << 24, Nq)})[0] == 0
    Nq, Nkv = 256, 256
    for kind, es in ((_fa2_lib.FA2_BIAS_F32, 4), (_fa2_lib.FA2_BIAS_IO_DTYPE, 2), (_fa2_lib.FA2_BIAS_BOOL, 1)):
        good = fl.last_bias_pitch(Nq, Nkv, es, gran=1)
        assert ((Nq - 1) * good + Nkv + 64 * good) * es < fl.SPAN_LIMIT <= ((Nq - 1) * (good + 1) + Nkv + 64 * (good + 1)) * es
        assert _bwd_plan(lib, 0, 1, 2, 2, Nq, Nkv, 64, bias_kind=kind, bias_strides=_fa2_lib.strides3(0, 0, good)) == (0, 1, 1)
        assert _bwd_plan(lib, 0, 1, 2, 2, Nq, Nkv, 64, bias_kind=kind, bias_strides=_fa2_lib.strides3(0, 0, good + 1))[0] == shape
        # the forward has no such rule: it accepts the slice (and takes a load form with 64-bit row pointers)
        plan = _fa2_lib.FwdPlan()
        assert lib.fa2_fwd_plan(0, 1, 2, Nq, Nkv, 64, None, None, 0.125, 0, kind, 0, ctypes.byref(plan)) == 0 and plan.kernel == _fa2_lib.FA2_KERNEL_HIP_BIAS


def test_backward_plan_leaves_the_hand_scheduled_passes_exactly_on_the_o_span_rule():
    """The guard this audit added (host.cpp: plan_bwd).  The hand-scheduled dQ pass of head dim 128 forms O's row offsets in 32 bits: with O on the last
    pitch of the 2 GiB rule both passes stay hand-scheduled, with the next pitch — and with O spans in [2 GiB, 4 GiB) and past 4 GiB — both run the
    compiler-scheduled kernels (the dK / dV pass follows the dQ pass: the sign of delta), and nothing is refused.  Beside it, what else the
    plan decides."""
    lib = _fa2_lib.load()
    HIP, ASM, SHORT = _fa2_lib.FA2_BWD_KERNEL_HIP, _fa2_lib.FA2_BWD_KERNEL_ASM, _fa2_lib.FA2_BWD_KERNEL_SHORT
    for dt, B, H, Nq, Nkv in ((0, 1, 1, 320, 320), (1, 2, 8, 288, 1024), (0, 1, 3, 4096, 512)):
        good = fl.last_pitch(Nq, 128)
        assert fl.span_bytes(Nq, good, 128) + 64 * good * 2 <= fl.SPAN_LIMIT < fl.span_bytes(Nq, good + 8, 128) + 64 * (good + 8) * 2
        assert _bwd_plan(lib, dt, B, H, H, Nq, Nkv, 128) == (0, ASM, ASM)
        assert _bwd_plan(lib, dt, B, H, H, Nq, Nkv, 128, {"o": _s3(good, Nq)}) == (0, ASM, ASM), (Nq, good)
        assert _bwd_plan(lib, dt, B, H, H, Nq, Nkv, 128, {"o": _s3(good + 8, Nq)}) == (0, HIP, HIP), (Nq, good + 8)
        for span in (3 << 30, 5 << 30):                         # inside [2 GiB, 4 GiB): no wrap yet, but outside the bound; past 4 GiB: the product would wrap
            assert _bwd_plan(lib, dt, B, H, H, Nq, Nkv, 128, {"o": _s3(span // 2 // (Nq - 1) // 128 * 128, Nq)}) == (0, HIP, HIP)
        # the other tensors' pitches do not move that edge, a causal call sits on it too
        assert _bwd_plan(lib, dt, B, H, H, Nq, Nkv, 128, {"o": _s3(good, Nq), "q": _s3(256, Nq), "do": _s3(384, Nq)}, flags=1) == (0, ASM, ASM)
        assert _bwd_plan(lib, dt, B, H, H, Nq, Nkv, 128, {"o": _s3(good + 8, Nq), "q": _s3(256, Nq)}, flags=1) == (0, HIP, HIP)
    # what the test-suite's GPU cases rely on: grouped heads keep the hand-scheduled dQ pass only; short sweeps; other head dims
    assert _bwd_plan(lib, 0, 3, 4, 2, 320, 320, 128) == (0, ASM, HIP)
    assert _bwd_plan(lib, 0, 3, 2, 2, 320, 77, 64) == (0, SHORT, HIP) and _bwd_plan(lib, 0, 3, 2, 2, 320, 77, 128) == (0, ASM, ASM)
    assert _bwd_plan(lib, 0, 1, 1, 1, 320, 77, 128, {"o": _s3(fl.last_pitch(320, 128) + 8, 320)}) == (0, SHORT, HIP)
    assert _bwd_plan(lib, 1, 3, 2, 2, 300, 300, 64, flags=1) == (0, HIP, HIP) and _bwd_plan(lib, 0, 1, 3, 3, 192, 192, 512) == (0, HIP, HIP)
    assert lib.fa2_bwd_plan(0, 1, 1, 1, 64, 64, 64, *[None] * 5, 0.125, 0, 0, None, None) == _codes()["FA2_ERR_NULL_POINTER"]


def test_packed_entry_points_sit_on_the_span_edge_of_every_bounded_tensor():
    """The packed entry points check their tensors last: with null tensors the last pitch reaches FA2_ERR_NULL_POINTER and the next one is
    FA2_ERR_BAD_SHAPE — K and V in the forward, the dropout forward and the plan; Q, dO, K and V in both backwards."""
    lib, c, plan = _fa2_lib.load(), _codes(), _fa2_lib.FwdPlan()
    null, shape = c["FA2_ERR_NULL_POINTER"], c["FA2_ERR_BAD_SHAPE"]
    H, D, mq, mk = 2, 64, 1500, 1100
    s2 = lambda pitch: _fa2_lib.strides2(D, pitch)             # noqa: E731  {head, row}
    small = s2(H * D)
    for which in ("k", "v"):
        for step, want in ((0, null), (8, shape)):
            st = {n: small for n in "qkvo"}
            st[which] = s2(fl.last_pitch(mk, D) + step)
            args = (3, H, H, mq, mk, D, None, None, st["q"], st["k"], st["v"], st["o"], 0, 0.125, 1, -1, -1, None)
            assert lib.fa2_fwd_varlen(0, *[None] * 5, *args) == want, (which, step)
            assert lib.fa2_fwd_varlen_dropout(0, *[None] * 5, *args, 0.25, 7) == want
            assert lib.fa2_fwd_varlen_scoremod(0, *[None] * 5, *args, 30.0, None, 0) == want          # the score-modifier call inherits the packed rule
            if which == "k":
                assert lib.fa2_fwd_varlen_plan(0, 3, H, H, mq, mk, D, small, st["k"], 0.125, 1, -1, -1, ctypes.byref(plan)) == (0 if want == null else shape)
    for which in ("q", "do", "k", "v"):
        n = mq if which in ("q", "do") else mk
        for step, want in ((0, null), (8, shape)):
            st = {t: small for t in ("q", "k", "v", "o", "do", "dq", "dk", "dv")}
            st[which] = s2(fl.last_pitch(n, D) + step)
            args = (3, H, mq, mk, D, None, None) + tuple(st[t] for t in ("q", "k", "v", "o", "do", "dq", "dk", "dv")) + (0, 0.125, 1, -1, -1, None)
            assert lib.fa2_bwd_varlen(1, *[None] * 10, *args) == want, (which, step)
            assert lib.fa2_bwd_varlen_dropout(1, *[None] * 10, *args, 0.25, 7) == want
            assert lib.fa2_bwd_varlen_scoremod(1, *[None] * 10, *args, 30.0, None, 0) == want
            for drop, cap in ((0.0, 0.0), (0.25, 0.0), (0.0, 30.0)):      # fa2_bwd_varlen_lse on each of its routes: the edge sits at the same pitch
                assert lib.fa2_bwd_varlen_lse(1, *[None] * 10, *args, drop, 7, cap, None, 0, None, 0) == want, (which, step, drop, cap)
    # O, dQ, dK, dV are not bounded: 1 MiB rows for 1500-row sequences reach the null tensors
    st = {t: small for t in ("q", "k", "v", "o", "do", "dq", "dk", "dv")}
    for t in ("o", "dq", "dk", "dv"):
        st[t] = s2(1 << 24)
    args = (3, H, mq, mk, D, None, None) + tuple(st[t] for t in ("q", "k", "v", "o", "do", "dq", "dk", "dv")) + (0, 0.125, 1, -1, -1, None)
    assert lib.fa2_bwd_varlen(0, *[None] * 10, *args) == null


def _asm_plan(lib, dt, B, H, Nq, Nkv, D, q_pitch, flags=0, scale=None):
    plan = _fa2_lib.FwdPlan()
    _fa2_lib.check(lib.fa2_fwd_plan(dt, B, H, Nq, Nkv, D, _s3(q_pitch, Nq), _s3(D, Nkv), D ** -0.5 if scale is None else scale, flags, 0, 0, ctypes.byref(plan)))
    return plan.kernel, plan.rows


def test_plan_leaves_the_hand_scheduled_forward_bodies_exactly_on_their_q_span_rules():
    """DESIGN.md "addressing limits": the 256-row bodies address a head's Q rows — 64 rows of slack — with 32-bit byte offsets: below 4 GiB at the
    body's own head dim (row pitch a multiple of it), below 2 GiB at a head dim below it (the out-of-range marker is byte offset 2^31); the 128-row
    kernel of head dims up to 256 addresses Q and O — 128 rows of slack (every wave of the last workgroup forms its rows' offsets), 256 columns — below 4 GiB.  The last pitch inside stays hand-scheduled, the
    first outside runs the compiler-scheduled kernels; nothing is refused."""
    lib = _fa2_lib.load()
    ASM, HIP = _fa2_lib.FA2_KERNEL_ASM, (_fa2_lib.FA2_KERNEL_HIP_128, _fa2_lib.FA2_KERNEL_HIP_256)
    B, H, Nq, Nkv = 2, 64, 320, 2048                          # a grid of 256-row workgroups well past 3/8 of any device's CUs, a sweep long enough
    for dt, D, HD, limit in ((0, 128, 128, P32), (1, 128, 128, P32), (0, 64, 64, P32), (0, 96, 128, P31), (0, 48, 64, P31)):
        step = HD if D == HD else 8
        inside = ((limit // 2 - 1 - D) // (Nq + 64)) // step * step
        assert ((Nq + 64) * inside + D) * 2 < limit <= ((Nq + 64) * (inside + step) + D) * 2
        assert _asm_plan(lib, dt, B, H, Nq, Nkv, D, inside) == (ASM, 256), (dt, D, inside)
        assert _asm_plan(lib, dt, B, H, Nq, Nkv, D, inside + step)[0] in HIP, (dt, D, inside + step)
    for dt, D, Nq in ((0, 256, 320), (1, 192, 320), (1, 256, 257), (0, 160, 264)):
        inside = ((P32 // 2 - 1 - 256) // (Nq + 128)) // 8 * 8
        assert ((Nq + 128) * inside + 256) * 2 < P32 <= ((Nq + 128) * (inside + 8) + 256) * 2
        assert _asm_plan(lib, dt, B, H, Nq, Nkv, D, inside) == (ASM, 128), (dt, D)
        assert _asm_plan(lib, dt, B, H, Nq, Nkv, D, inside + 8)[0] in HIP, (dt, D)


def test_forward_bias_takes_the_lds_dma_form_exactly_inside_the_slice_rule():
    """The forward refuses no bias: it stages the tile by LDS-DMA, 32-bit byte offsets into one (b, h) slice, while the slice obeys the backward's
    2 GiB rule — on a grid past 3/8 of the CUs, head dims up to 128 — and loads it from 64-bit row pointers from the next pitch on
    (fa2_fwd_bias_form; host.cpp: bias_load_form, which the launch executes)."""
    lib, c = _fa2_lib.load(), _codes()
    TILE, DMA, ROW = _fa2_lib.FA2_BIAS_FORM_TILE, _fa2_lib.FA2_BIAS_FORM_TILE_DMA, _fa2_lib.FA2_BIAS_FORM_ROW
    form = lambda kind, B, H, Nq, Nkv, D, pitch: lib.fa2_fwd_bias_form(kind, B, H, Nq, Nkv, D, _fa2_lib.strides3(0, 0, pitch))      # noqa: E731
    for kind, es in ((_fa2_lib.FA2_BIAS_F32, 4), (_fa2_lib.FA2_BIAS_IO_DTYPE, 2), (_fa2_lib.FA2_BIAS_BOOL, 1)):
        gran = 16 // es
        for Nq, Nkv, D in ((256, 256, 64), (1000, 512, 128), (300, 4096, 96)):
            good = fl.last_bias_pitch(Nq, Nkv, es)
            assert ((Nq - 1) * good + Nkv + 64 * good) * es < fl.SPAN_LIMIT <= ((Nq - 1) * (good + gran) + Nkv + 64 * (good + gran)) * es
            assert form(kind, 3, 33, Nq, Nkv, D, good) == DMA, (kind, Nq, good)
            assert form(kind, 3, 33, Nq, Nkv, D, good + gran) == TILE, (kind, Nq, good + gran)
            assert form(kind, 3, 33, Nq, Nkv, D, 1 << 26) == TILE                 # a slice past 4 GiB
            assert form(kind, 1, 1, Nq, Nkv, D, good) == TILE                     # a small grid keeps the 64-bit row pointers at any pitch
        assert form(kind, 3, 33, 256, 256, 256, 256) == TILE                      # head dims above 128 too
        assert form(kind, 3, 33, 256, 256, 64, 0) == ROW
    assert form(7, 1, 1, 64, 64, 64, 64) == c["FA2_ERR_BIAS"] and lib.fa2_fwd_bias_form(1, 1, 1, 64, 64, 64, None) == c["FA2_ERR_NULL_POINTER"]
    assert form(1, 1, 1, 64, 64, 60, 64) == c["FA2_ERR_HEAD_DIM"] and form(1, 0, 1, 64, 64, 64, 64) == c["FA2_ERR_BAD_SHAPE"]


@pytest.mark.parametrize("case", list(fl.DENSE_CASES) + fl.SPAN_CASES + fl.BIAS_SPAN_CASES + fl.F32_CASES + list(fl.SCOREMOD_CASES) + list(fl.LSE_CASES),
                         ids=lambda c: c["id"])
def test_every_case_is_planned_on_the_kernel_it_names(case):
    """The case table says which kernel a shape is there for (`expect`, `expect_bwd`, under the case's options): the plan queries, asked with the
    layout's own strides, agree — for the far layout and for its twin.  (The GPU module asserts the same before it launches; here the table cannot
    drift unnoticed on a machine without a GPU.  Plans depend on the CU count: 256, the MI355X's, is also what the library assumes without a device.)"""
    import test_far_offsets_gpu as tg
    lib, ws = _fa2_lib.load(), 0
    if case["layout"] == "span":
        slots, twin = fl.span_slots(case)
    elif case["layout"] == "bias_span":
        slots, twin = fl.bias_span_slots(case)
    else:
        if case["ws"]:
            dims = (tg._code(case), case["B"], case["H"], case["Hkv"], case["Nq"], case["Nkv"], case["D"], 0)
            ws = max(lib.fa2_fwd_gqa_workspace_bytes(*dims), lib.fa2_bwd_gqa_workspace_bytes(*dims) if case["bwd"] else 0)
            assert ws > 0 and (case["expect"] != "bwd_split" or lib.fa2_bwd_gqa_workspace_bytes(*dims) > 0)
        slots, twin, _ = fl.dense_slots(case, ws, step=fl.F32_STEP if case in fl.F32_CASES else fl.FAR_STEP)
    arena = torch.empty(fl.ARENA_F32_BYTES, dtype=torch.uint8, device="meta")
    T, Tt = ({n: s.view(arena) for n, s in sl.items()} for sl in (slots, twin))
    with _fa2_lib.options(**case["opts"]):
        tg._expect(case, tg._plan(case, T), tg._plan(case, Tt))
        if case["fam"] == "bias":
            assert case["form"] and tg._bias_form(case, T) == tg._bias_form(case, Tt) == tg.BIAS_FORMS[case["form"]], (case["form"], tg._bias_form(case, T))
        if case["bwd"] and case["fam"] in ("dense", "bias"):
            got, got_t = tg._bwd_plan(case, T), tg._bwd_plan(case, Tt)
            assert got == got_t and (not case.get("expect_bwd") or got == tuple(tg.BWD_KERNELS[k] for k in case["expect_bwd"])), (got, got_t, case["expect_bwd"])


# ---------------------------------------------------------------------------------------------------------------- KV-cache decode
def _decode_ids(v):
    return v["id"] if isinstance(v, dict) else v


def test_decode_table_reaches_every_kernel_length_and_format():
    cases = fl.DECODE_CASES
    lens = {n for c in cases for n in c["lens"]}
    assert {0, 65, 129, 1000} <= lens and any(0 < n < c["Nq"] for c in cases for n in c["lens"])
    assert {c["rt"] for c in cases} == {1, 2, 4} and {c["D"] for c in cases} == {64, 128} and {c["dt"] for c in cases} == {"f16", "bf16"}
    assert {c["layout"] for c in cases} == {"batch", "head", "wide", "paged"} and {c["page"] for c in cases} == {0, 64, 128}
    assert {c["bt"] for c in cases if c["layout"] == "paged"} == {"far", "compact"} and {c["descale"] for c in cases} == {"kv", "k", "v"}
    assert all(n <= c["nmax"] for c in cases for n in c["lens"]) and all(c["Nq"] * (c["H"] // c["Hkv"]) <= 64 for c in cases)


@pytest.mark.parametrize("fmt", fl.DECODE_FORMATS)
@pytest.mark.parametrize("case", fl.DECODE_CASES, ids=_decode_ids)
def test_decode_layouts_cross_what_they_claim(case, fmt):
    """Every decode layout, with a split's workspace near and far: inside the arena, no two rows share a byte, and the slices named by the layout cross
    byte 2^31 and byte 2^32 — for the e4m3 caches that is element index 2^31 and 2^32 of the cache, for the 16-bit wide-row cache element index 2^31.
    The plan and workspace queries take sizes only, so the far call and its twin get one answer; it names the row tiles the case is there for."""
    import test_far_offsets_gpu as tg
    need = [tg._decode_plan(case, fmt, ns)[1] for ns in tg.DECODE_SPLITS]
    assert need[0] == 0 and need[1] > 0 and need[2] > 0
    for where in ("near", "far"):
        slots, twin, tbytes = fl.decode_slots(case, fmt, max(need), where)
        fl.validate(list(slots.values()), fl.ARENA_BYTES)
        fl.validate(list(twin.values()), tbytes)
        _meta_views(slots, fl.ARENA_BYTES)
        _meta_views(twin, tbytes)
        assert (slots["ws"].offset > P32) == (where == "far") and (slots["ws"].offset < P31) == (where == "near")
    assert ("kd" in slots, "vd" in slots) == ((fmt == "fp8" and "k" in case["descale"]), (fmt == "fp8" and "v" in case["descale"]))
    assert all(t.shape == slots[n].shape or (case["layout"] == "paged" and n in ("k", "v")) for n, t in twin.items())
    lay, k, v = case["layout"], slots["k"], slots["v"]
    ces = 1 if fmt == "fp8" else 2
    assert k.esize == ces and k.dtype == v.dtype and k.strides == v.strides
    if lay in ("batch", "paged"):
        far = ["q", "o", "lse"] + [n for n in ("kd", "vd") if n in slots] + (["k", "v"] if lay == "batch" else []) + (["bt"] if case["bt"] == "far" else [])
        for n in far:
            assert _crosses(slots[n], 0, P31) and _crosses(slots[n], 0, P32) and slots[n].strides[0] * slots[n].esize == fl.FAR_STEP, n
        assert slots["lens"].strides == (1,)                                          # cache_seqlens stays contiguous: the operator requires it
        if fmt == "fp8" and lay == "batch":                                           # the cache's ELEMENT index: batch 1 past 2^31, batch 2 past 2^32
            assert P31 < k.strides[0] < P32 < 2 * k.strides[0]
    if lay == "head":
        for n, dim in (("k", 2), ("v", 2), ("q", 2), ("o", 2), ("lse", 1)):
            starts = [slots[n].slice_range(dim, i)[0] for i in range(slots[n].shape[dim])]
            assert min(starts) < P31 and any(P31 < a < P32 for a in starts) and max(starts) > P32, (n, starts)
        assert k.strides[2] * ces == fl.FAR_STEP and (fmt != "fp8" or P31 < k.strides[2] < P32 < 2 * k.strides[2])
    if lay == "wide":
        n, rows = case["lens"][0], k.row_starts()[0, :, 0]
        assert k.strides[1] * ces == fl.DECODE_WIDE_PITCH == v.strides[1] * ces and 0 < v.offset - k.offset < 65536      # K and V interleave inside the pitch
        for s in (k, v):
            at = s.row_starts()[0, :, 0]
            assert at[0] < P31 and ((at[:n] > P31) & (at[:n] < P32)).any() and at[n - 1] > P32 and at[n - 32] > P32      # the whole last key tile lies past 2^32
            assert at[n:].min() > P32 and at[-1] + s.row_bytes() <= fl.ARENA_BYTES and len(at) > n                      # the invalid keys stay inside the arena
        elem = (rows[n - 1] - k.offset) // ces                                                                          # the last key's element index in the cache
        assert elem > (P32 if fmt == "fp8" else P31) and elem == (n - 1) * k.strides[1]
    if lay == "paged":
        bt, bt_t, poison, pages_t = fl.decode_block_tables(case, fmt)
        low, mid, high = fl.decode_page_regions(case, fmt)
        assert low and mid and len(high) >= 3 and k.strides[0] * ces == fl.DECODE_PAGE_STRIDE == v.strides[0] * ces and fl.DECODE_PAGE_STRIDE // 4096 % 2 == 1
        assert 0 < v.offset - k.offset < fl.DECODE_PAGE_STRIDE and k.shape[0] == fl.DECODE_NUM_PAGES and twin["k"].shape[0] == pages_t
        for s in (k, v):                                                                                                # the regions are what the slots say
            assert all(s.slice_range(0, p)[1] <= P31 for p in low) and all(P31 < s.slice_range(0, p)[0] and s.slice_range(0, p)[1] <= P32 for p in mid)
            assert all(s.slice_range(0, p)[0] > P32 for p in high)
        taken = []
        for b, n in enumerate(case["lens"]):
            used = -(-n // case["page"])
            mine = [int(p) for p in bt[b, :used]]
            taken += mine
            if n:
                assert all(any(p in r for p in mine) for r in (low, mid, high)), (b, mine)
                assert mine != sorted(mine)                                                                             # shuffled
            assert all(int(p) == poison for p in bt[b, used:])
        assert len(set(taken)) == len(taken) and poison not in taken and poison in high and 0 <= bt.min() and bt.max() < fl.DECODE_NUM_PAGES
        tw = [int(p) for b, n in enumerate(case["lens"]) for p in bt_t[b, :-(-n // case["page"])]]
        assert len(set(tw)) == len(tw) == pages_t - 1 and 0 <= bt_t.min() and bt_t.max() < pages_t and tw != [int(p) for p in taken]
        spare_t = (set(range(pages_t)) - set(tw)).pop()                                                                 # the twin's page nobody writes
        assert all(int(p) == spare_t for b, n in enumerate(case["lens"]) for p in bt_t[b, -(-n // case["page"]):])
        if fmt == "fp8":                                                                                                # page id * page stride as an element index
            assert max(taken) * k.strides[0] > P32 and any(P31 < p * k.strides[0] < P32 for p in taken)
        if case["bt"] == "compact":
            assert slots["bt"].strides == (bt.shape[1], 1)
    # the images: valid rows hold data, every other cache byte is poison; a paged twin holds the same logical rows under its own numbering
    data = fl.decode_inputs(case, fmt)
    tables = fl.decode_block_tables(case, fmt) if lay == "paged" else (None, None)
    img, img_t = fl.decode_images(case, fmt, slots, data, tables[0]), fl.decode_images(case, fmt, twin, data, tables[1])
    valid = sum(case["lens"]) * case["Hkv"] * case["D"] * ces
    for im in (img, img_t):
        assert set(im) == set(slots) - {"o", "lse", "ws"}
        for n in ("k", "v"):
            raw = data[n].contiguous().view(torch.uint8)
            assert int((im[n] != fl.POISON).sum()) <= valid and int((im[n] != fl.POISON).sum()) >= valid * 0.98         # (a data byte may equal 0xFF by chance: fp16 only)
            for b, ln in enumerate(case["lens"]):
                if lay != "paged":
                    assert torch.equal(im[n][b, :ln], raw[b, :ln]) and (im[n][b, ln:] == fl.POISON).all()
    if lay == "paged":
        page = case["page"]
        for b, ln in enumerate(case["lens"]):
            for j in range(-(-ln // page)):
                rows = min(page, ln - j * page)
                assert torch.equal(img["k"][int(tables[0][b, j]), :rows], img_t["k"][int(tables[1][b, j]), :rows])
                assert (img["k"][int(tables[0][b, j]), rows:] == fl.POISON).all()


def _toy_paged_case():
    """A paged decode in miniature, on the CPU: six pages of 64 keys 40 KiB apart in a 1 MiB arena, two sequences (70 and 100 keys) whose pages are
    neighbours in memory, page 5 for the block table's unused entries, page 0 unused.  The 'kernel' is dense float64 attention through the block
    table, reading the arena's own views — what it reads past a length or in a page nobody wrote is poison, as on the GPU."""
    import decode_refs as dr
    case = dict(id="toy", layout="paged", dt="f16", D=64, H=2, Hkv=1, Nq=2, lens=(70, 100), B=2, page=64)
    f16, f32, i32 = torch.float16, torch.float32, torch.int32
    slots = {"q": fl._bslot("q", f16, (2, 2, 2, 64), [512, 256, 128], 0), "o": fl._bslot("o", f16, (2, 2, 2, 64), [512, 256, 128], 4096 + 16),
             "lse": fl._bslot("lse", f32, (2, 2, 2), [16, 8], 8192 + 32), "lens": fl._bslot("lens", i32, (2,), [], 12288), "bt": fl._bslot("bt", i32, (2, 2), [8], 12288 + 64),
             "k": fl._bslot("k", f16, (6, 64, 1, 64), [40960, 128, 128], 65536), "v": fl._bslot("v", f16, (6, 64, 1, 64), [40960, 128, 128], 65536 + 16384)}
    fl.validate(list(slots.values()), 1 << 20)
    g = torch.Generator().manual_seed(11)
    data = {"q": torch.randn((2, 2, 2, 64), generator=g).half(), "k": torch.randn((2, 128, 1, 64), generator=g).half(),
            "v": torch.randn((2, 128, 1, 64), generator=g).half(), "lens": torch.tensor(case["lens"], dtype=i32)}
    bt = np.array([[4, 1], [2, 3]], dtype=np.int32)
    images = fl.decode_images(case, "16", slots, data, bt)
    refs = dr.refs16(data["q"], data["k"], data["v"], case["lens"], 0)
    return case, slots, images, refs


def _toy_decode(arena, slots, case, mutant=None):
    T = {n: s.view(arena) for n, s in slots.items()}
    page, Nq, D = case["page"], case["Nq"], case["D"]
    for b in range(case["B"]):
        n = int(T["lens"][b]) + (1 if mutant == "key_at_len" and b == 0 else 0)
        pids = [int(T["bt"][b, j // page]) + (1 if mutant == "neighbour_page" and (b, j // page) == (0, 1) else 0) for j in range(n)]
        kk = torch.stack([T["k"][p, j % page, 0] for j, p in enumerate(pids)]).double()
        vv = torch.stack([T["v"][p, j % page, 0] for j, p in enumerate(pids)]).double()
        s = torch.einsum("ihd,jd->hij", T["q"][b].double(), kk) * D ** -0.5
        keep = torch.arange(n)[None, :] <= (n - Nq + torch.arange(Nq))[:, None]
        s = s.masked_fill(~keep, float("-inf"))
        dead = ~keep.any(1)
        lse = torch.logsumexp(s.masked_fill(dead[None, :, None], 0.0), -1)
        p = torch.exp(s - lse.unsqueeze(-1)).masked_fill(dead[None, :, None], 0.0)
        T["o"][b] = torch.einsum("hij,jd->ihd", p, vv).half()
        T["lse"][b] = (lse / np.log(2.0)).masked_fill(dead[None, :], float("-inf")).float()
    if mutant == "write_into_poison_page":
        T["k"][5, 3, 0, 7] = 1.0


def _toy_check(arena, slots, case, images, refs, twin_out):
    """What tests/test_far_offsets_gpu.py's _decode_run checks, in its order -> list of failures."""
    import decode_refs as dr
    got = fl.harvest(arena, slots)
    fails = fl.image_failures(got, images) + fl.compare_exact(got, twin_out, ["o", "lse"])
    try:
        dr.check(got["o"], got["lse"], refs, case["lens"], 0, "toy")
    except AssertionError as e:
        fails.append("truth: %s" % (e,))
    return fails


def test_decode_checker_flags_its_mutants():
    case, slots, images, refs = _toy_paged_case()
    runs = {}
    for mutant in (None, "neighbour_page", "key_at_len", "write_into_poison_page"):
        arena = fl.new_arena(1 << 20, "cpu")
        for n, im in images.items():
            slots[n].bytes_view(arena).copy_(im)
        _toy_decode(arena, slots, case, mutant)
        if mutant is None:
            clean = {n: slots[n].view(arena).clone() for n in ("o", "lse")}
        runs[mutant] = _toy_check(arena, slots, case, images, refs, clean)
        assert fl.arena_is_poison(arena)
    assert runs[None] == []
    # an output built from the neighbouring page id — real keys of the other sequence, nothing non-finite: the twin and the truth both object
    assert any(f.startswith("o:") for f in runs["neighbour_page"]) and any("oracle O" in f or "float64 O" in f for f in runs["neighbour_page"])
    assert not any("input" in f for f in runs["neighbour_page"])
    # the key at index len is poison: it reaches O as NaN
    assert any("O not finite" in f for f in runs["key_at_len"]) and any(f.startswith("o:") for f in runs["key_at_len"])
    # a write into a page nobody uses: the outputs are right, the page's image is not
    assert runs["write_into_poison_page"] == [" input k was written, or a row beyond a length is no longer poison"]


# ---------------------------------------------------------------------------------------------------------------- merge, score modifiers, a gradient for the LSE
@pytest.mark.parametrize("case", fl.MERGE_CASES, ids=_decode_ids)
def test_merge_layouts_cross_both_thresholds_with_one_stride_set(case):
    slots, twin, tbytes = fl.merge_slots(case)
    fl.validate(list(slots.values()), fl.ARENA_BYTES)
    fl.validate(list(twin.values()), tbytes)
    _meta_views(slots, fl.ARENA_BYTES)
    _meta_views(twin, tbytes)
    assert set(slots) == set(fl.MERGE_O_NAMES + fl.MERGE_L_NAMES) and set(fl.MERGE_INPUTS) < set(slots)
    for group in (["o%d" % k for k in range(fl.MERGE_PARTS)], ["l%d" % k for k in range(fl.MERGE_PARTS)], ["do%d" % k for k in range(fl.MERGE_PARTS)],
                  ["dl%d" % k for k in range(fl.MERGE_PARTS)]):
        assert len({slots[n].strides for n in group}) == 1 and len({slots[n].offset for n in group}) == fl.MERGE_PARTS      # one stride set, bases of their own
    lay = case["layout"]
    if lay in ("batch", "head"):
        dim = 0 if lay == "batch" else 1
        for n, s in slots.items():
            assert _crosses(s, dim, P31) and _crosses(s, dim, P32), n
        assert slots["o2"].offset - slots["o0"].offset == 2 * fl.MERGE_PART_GAP
    elif lay == "packed":
        assert case["B"] == 1 and case["Nq"] == fl.PACKED_TOTAL
        for n in fl.MERGE_O_NAMES:
            s = slots[n]
            at = s.row_starts()[:, 0]
            assert s.kind == "packed" and s.strides[0] * s.esize == fl.PACKED_PITCH_BYTES and at[0] < P31 and ((at > P31) & (at < P32)).any() and at[-1] > P32
        assert all(slots[n].offset > P32 and slots[n].shape == (case["H"], case["Nq"]) for n in fl.MERGE_L_NAMES)
    else:                                                                 # the parts' bases: the arena's start, past 2^31, past 2^32
        for names in (("o0", "o1", "o2"), ("l0", "l1", "l2"), ("do0", "do1", "do2"), ("dl0", "dl1", "dl2")):
            a, b, c = (slots[n].offset for n in names)
            assert a < 16 * fl.MIB and P31 < b < P32 < c
    assert {c["D"] for c in fl.MERGE_CASES} >= {128, 40} and {c["dt"] for c in fl.MERGE_CASES} == {"f16", "bf16"} and any(c["natural"] for c in fl.MERGE_CASES)
    # the data: part 1 has rows of weight 0 whose O stays poison; every other input byte is data
    data = fl.merge_inputs(case)
    img = fl.merge_images(case, slots, data)
    un = data["unwritten"]
    assert un.any() and not un.all() and un[:, :, 0].all() and all(torch.isneginf(data["l%d" % k][:, :, 0]).all() for k in range(fl.MERGE_PARTS))
    assert int((img["o1"] == fl.POISON).all(-1).sum()) == int(un.sum())
    assert not torch.isneginf(data["l0"][:, :, 1:]).any() and not torch.isneginf(data["l2"][:, :, 1:]).any()


def test_merge_checker_flags_a_row_merged_from_the_wrong_parts_base():
    import lse_refs as R
    case = dict(fl.MERGE_CASES[0], B=2, H=2, Nq=9, D=16)
    data = fl.merge_inputs(case)
    parts = range(fl.MERGE_PARTS)
    outs, lses = [data["o%d" % k] for k in parts], [data["l%d" % k] for k in parts]
    clean = [torch.where(torch.isneginf(l).unsqueeze(-1), torch.zeros_like(o), o) for o, l in zip(outs, lses)]

    def result(os_):
        oin, lin = [o.double().requires_grad_(True) for o in os_], [(l.double() * R.LN2).requires_grad_(True) for l in lses]
        O, L = R.merge64(oin, lin)
        dead = torch.isneginf(L.detach())
        ((O * data["dout"].double()).sum() + (L.masked_fill(dead, 0.0) * (data["dlse"].double() / R.LN2)).masked_fill(dead, 0.0).sum()).backward()
        return (O.detach().half(), (L.detach() / R.LN2).float(), [t.grad.half() for t in oin], [(t.grad * R.LN2).float() for t in lin])

    good = result(clean)
    R.merge_check("clean", torch.float16, False, outs, lses, data["dout"], data["dlse"], *good)
    # row (1, 0, 5) of the merged O taken with every part's pointer rotated by one: the weights of parts k meet the rows of parts k + 1
    wrong = result([clean[1], clean[2], clean[0]])
    bad_o = good[0].clone()
    bad_o[1, 0, 5] = wrong[0][1, 0, 5]
    assert (bad_o != good[0]).any()
    with pytest.raises(AssertionError):
        R.merge_check("mutant", torch.float16, False, outs, lses, data["dout"], data["dlse"], bad_o, *good[1:])
    # ... and a part's gradient that went to another part's base
    with pytest.raises(AssertionError):
        R.merge_check("mutant", torch.float16, False, outs, lses, data["dout"], data["dlse"], good[0], good[1], [good[2][1], good[2][0], good[2][2]], good[3])


@pytest.mark.parametrize("case", list(fl.SCOREMOD_CASES) + list(fl.LSE_CASES), ids=_decode_ids)
def test_scoremod_and_lse_layouts_place_slopes_and_dlse_where_they_claim(case):
    import lse_refs as R
    slots, twin, tbytes = fl.dense_slots(case)
    fl.validate(list(slots.values()), fl.ARENA_BYTES)
    fl.validate(list(twin.values()), tbytes)
    _meta_views(slots, fl.ARENA_BYTES)
    dim = 0 if case["far"] == "batch" else 1
    for n in ("q", "k", "v", "o", "lse"):
        starts = [slots[n].slice_range(dim, i)[0] for i in range(slots[n].shape[dim])]
        assert min(starts) < P31 and any(P31 < a < P32 for a in starts) and max(starts) > P32, n
    if case["slopes"]:
        s = slots["slopes"]
        assert case["softcap"] == 30.0 and s.dtype == torch.float32 and s.shape == (case["B"], case["H"])
        if case["far"] == "batch":                                        # b * alibi_batch_stride + h past byte 2^31 and 2^32
            assert _crosses(s, 0, P31) and _crosses(s, 0, P32) and s.strides[0] * 4 == fl.FAR_STEP
        else:
            assert case["B"] == 1                                         # one shared [H] vector: the call passes stride 0
    if case["dlse"]:
        s = slots["dlse"]
        assert case["bwd"] and s.shape == slots["lse"].shape
        if case["dlse"] == "far":
            assert s.strides == slots["lse"].strides and _crosses(s, dim, P31) and _crosses(s, dim, P32)
        else:                                                             # compact beside far tensors: strides of its own
            assert s.strides == (case["H"] * case["Nq"], case["Nq"], 1) != slots["lse"].strides and s.extent()[1] < P31
        dead = ~R.ff.band(case["Nq"], case["Nkv"], *(case["window"] or (-1, -1, 0)), case["causal"], "cpu").any(-1)
        assert bool(dead.any()) == (case["window"] is not None) and not dead.all()
    tabs = list(fl.SCOREMOD_CASES) + list(fl.LSE_CASES)
    assert {c["dlse"] for c in tabs} == {None, "far", "compact"} and any(c["dlse"] == "compact" and c["far"] for c in tabs)
    assert {(c["fam"], bool(c["dlse"])) for c in tabs} >= {("scoremod", False), ("dense", True), ("bias", True), ("window", True), ("dropout", True), ("scoremod", True)}


def test_f32_decode_case_puts_lse_descales_and_block_table_past_element_index_two_to_the_31():
    import test_far_offsets_gpu as tg
    case = fl.DECODE_F32_CASE
    assert case["layout"] == "paged" and case["bt"] == "far" and case["descale"] == "kv" and case["B"] == 3 and case["lens"][2] > 0
    for where in ("near", "far"):
        slots, twin, tbytes = fl.decode_slots(case, "fp8", tg._decode_plan(case, "fp8", 3)[1], where, step=fl.F32_STEP)
        fl.validate(list(slots.values()), fl.ARENA_F32_BYTES)
        fl.validate(list(twin.values()), tbytes)
        _meta_views(slots, fl.ARENA_F32_BYTES)
    for n in ("lse", "kd", "vd", "bt"):                                  # 4-byte elements: b * stride[0] leaves 31 bits for the last sequence, which has keys
        s = slots[n]
        first = [s.slice_range(0, b)[0] // 4 for b in range(3)]
        assert s.esize == 4 and first[0] < P31 // 4 and P31 // 2 < first[1] < P31 < first[2] and 2 * s.strides[0] > P31, (n, first)
    assert max(s.extent()[1] for s in (slots["k"], slots["v"])) < fl.ARENA_BYTES      # the pool itself stays where the other arena has it


def test_f32_case_puts_dlse_and_slopes_past_float_index_two_to_the_31():
    case = fl.F32_CASES[-1]
    slots, _, _ = fl.dense_slots(case, step=fl.F32_STEP)
    assert case["dlse"] == "far" and case["slopes"] and case["fam"] == "scoremod"
    for n in ("dlse", "slopes"):
        first = [slots[n].slice_range(0, b)[0] // 4 for b in range(3)]
        assert first[0] < P31 // 4 and P31 // 2 < first[1] < P31 < first[2] and 2 * slots[n].strides[0] > P31, (n, first)


def test_lse_checker_flags_a_gradient_that_ignored_dlse():
    """tests/test_far_offsets_gpu.py's _truth_lse on the CPU: given the emulation's own outputs it passes, given gradients computed without the dlse
    term it objects to dQ (dV does not depend on dlse), and its dead rows — a NaN in dlse — are there."""
    import lse_refs as R
    import test_far_offsets_gpu as tg
    case = dict(fl.LSE_CASES[5], B=2, H=2, Hkv=2, Nq=96, Nkv=48, far=None)
    assert case["fam"] == "window" and case["dlse"]
    slots, _, _ = fl.dense_slots(case)
    data = tg._inputs(case, slots, "cpu")
    dead = torch.isnan(data["dlse"])
    assert dead[:, :, 84:].all() and not dead[:, :, :84].any()

    def outputs(with_u):
        out = {n: [] for n in ("o", "lse", "dq", "dk", "dv")}
        allow = R.ff.band(96, 48, *case["window"], True, "cpu")
        for b in range(2):
            u = torch.nan_to_num(data["dlse"][b], nan=0.0) / R.LN2 if with_u else None
            e = R.emulate(data["q"][b], data["k"][b], data["v"][b], data["do"][b], u, allow, tg._scale(case), torch.float16)
            for n, m in (("o", "O"), ("lse", "lse"), ("dq", "dQ"), ("dk", "dK"), ("dv", "dV")):
                out[n].append(e[m].float() if n == "lse" else e[m].half())
        return {n: torch.stack(v) for n, v in out.items()}

    fails, live = tg._truth_lse(case, outputs(True), data)
    assert fails == [] and not live[:, :, 84:].any() and live[:, :, :84].all()
    fails, _ = tg._truth_lse(case, outputs(False), data)
    assert len(fails) == 2 and all("dQ" in f for f in fails), fails


def test_packed_scoremod_and_lse_cases_place_slopes_and_dlse_far():
    cases = {c["id"]: c for c in fl.PACKED_CASES}
    assert {"varlen_smod_gqa_topleft", "varlen_smod_bottomright", "varlen_lse"} <= set(cases)
    top, bottom, lse = cases["varlen_smod_gqa_topleft"], cases["varlen_smod_bottomright"], cases["varlen_lse"]
    assert top["Hkv"] < top["H"] and not top["bwd"] and not top["bottom_right"] and bottom["bwd"] and bottom["bottom_right"] and lse["bwd"] and lse["bottom_right"]
    for c in (top, bottom):
        s = fl.packed_slots(c)[0]["slopes"]                              # [num_sequences, H]: s * alibi_batch_stride + h
        starts = [s.slice_range(0, i)[0] for i in range(s.shape[0])]
        assert c["softcap"] == 30.0 and s.shape == (len(fl.PACKED_LENS), c["H"]) and s.strides[0] * 4 == fl.PACKED_SLOPES_STEP
        assert starts[0] < P31 and sum(a > P31 for a in starts) >= 2 and starts[-1] % (1 << 16) != 0
        assert [n for n, a in zip(fl.PACKED_LENS, starts) if a > P31 and n > 0], "a sequence with rows reads its slopes past 2^31"
    slots = fl.packed_slots(lse)[0]
    assert slots["dlse"].offset > P32 and slots["dlse"].strides == slots["lse"].strides and slots["dlse"].offset != slots["lse"].offset
    # bottom-right: sequences with fewer keys than rows have rows that see no key (they carry a NaN in dlse)
    assert any(nk < n for n, nk in zip(fl.PACKED_LENS, fl.PACKED_LENS_K))
