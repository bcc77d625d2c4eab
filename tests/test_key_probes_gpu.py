"""GPU tests (`-m gpu`) of the dense forward and backward on the inputs of tests/key_probes.py: counting inputs (A), pointer inputs (B) and random inputs
with per-element bars (C); and of every backward — dense, windowed, packed, grouped, masked, dropout, score modifiers, their packed twins and the *_lse
entries — on two-key pointer inputs (D, the second half of this file).  The bars do not grow with the sweep: one (row, key) pair missed at Nkv = 4096 fails A's LSE (one count) or B's O (the row
points at it), where the per-tensor bars of the other test modules pass a whole dropped tile (tests/test_key_probes.py proves both on float64 mutants).

Every case asks the library's plan query which kernel serves the call and asserts the route it is named for BEFORE it runs anything — on paper too:
tests/test_key_probes.py runs route_of() of every case without a GPU.  Classes A and B need no [Nq, Nkv] reference (the pointer builder checks its own
condition from the integer Gram matrix on the device); class C computes float64 dense attention on the device, a few heads at a time."""
import ctypes

import pytest
import torch

import key_probes as kp
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import dropout_keep_mask, flash_attn_wmma
from test_parity_gpu import PERSISTENT_SHAPES
from test_split_gpu import SPLIT_SHAPES          # (its decode-sized entry B1 H32 Nq1 x 8192 is among them)

F16, BF16 = torch.float16, torch.bfloat16
ASM, HIP256, HIP128 = _fa2_lib.FA2_KERNEL_ASM, _fa2_lib.FA2_KERNEL_HIP_256, _fa2_lib.FA2_KERNEL_HIP_128
PRE, P16 = _fa2_lib.FA2_CONTRACT_PRESCALE_Q, _fa2_lib.FA2_CONTRACT_LSUM_P16
EXACT = _fa2_lib.FA2_FLAG_EXACT_SCALE


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run the CPU suite with -m 'not gpu'"
    return torch.device("cuda", 0)


def _code(dtype):
    return 0 if dtype == F16 else 1


def _s3(t):
    return _fa2_lib.strides3(t.stride(0), t.stride(1), t.stride(2))


def _layout(t, bnhd):
    """A [B,H,N,D] tensor as the call sees it: stored [B,N,H,D] when bnhd (a BHND view with BNHD strides)."""
    return t.transpose(1, 2).contiguous().transpose(1, 2) if bnhd else t


# ---------------------------------------------------------------------------------------------------------------- the cases
def case(route, B, H, Nq, Nkv, D, dtype, causal=False, Hkv=None, bnhd=False, ws=False, opts=None, classes="AB", expect=None, maps=None):
    return dict(route=route, B=B, H=H, Hkv=Hkv or H, Nq=Nq, Nkv=Nkv, D=D, dtype=dtype, causal=causal, bnhd=bnhd, ws=ws, opts=opts or {}, classes=classes,
                expect=expect or {}, maps=maps)


def _id(c):
    return "%s-%dx%dx%dx%dx%d-%s%s%s%s" % (c["route"], c["B"], c["H"], c["Nq"], c["Nkv"], c["D"], "f16" if c["dtype"] == F16 else "bf16",
                                           "-causal" if c["causal"] else "", "-bnhd" if c["bnhd"] else "", "-hkv%d" % c["Hkv"] if c["Hkv"] != c["H"] else "")


FULL_ASM = 1987           # the library's default of option "asm" (route_of asserts it); bit 6 cleared: the 32x32x16 bodies
PERSISTENT = PERSISTENT_SHAPES[:4]      # (the fifth, config 2 itself, is the long-sweep case below)


def _forward_cases():
    out = []
    for dtype in (F16, BF16):
        for causal in (False, True):
            # the 16x16x32 head-dim-128 bodies, ten items on 256 CUs: one item per workgroup; and the 32x32x16 bodies (option "asm" bit 6 cleared)
            out.append(case("d128_m16", 1, 2, 1100, 1984, 128, dtype, causal, opts=dict(rows=256), classes="ABC", maps="all",
                            expect=dict(kernel=ASM, rows=256, contract=(PRE | P16) if dtype == F16 else P16, nsplit=0, items_le_cus=True)))
            out.append(case("d128_m32", 1, 2, 1100, 1984, 128, dtype, causal, opts=dict(rows=256, asm=FULL_ASM & ~64), classes="ABC", maps="edges",
                            expect=dict(kernel=ASM, rows=256, contract=PRE if dtype == F16 else 0, nsplit=0, items_le_cus=True)))
    for (B, H, Nq, Nkv, bnhd) in PERSISTENT:
        for causal in (False, True):
            nkv = max(Nkv, Nq) if causal else Nkv          # (top-left causal: keep the square case, as test_parity_gpu does)
            out.append(case("persistent", B, H, Nq, nkv, 128, F16, causal, bnhd=bnhd, opts=dict(rows=256), maps="edges",
                            expect=dict(kernel=ASM, rows=256, nsplit=0, items_gt_cus=True)))
    out.append(case("persistent_long", 2, 16, 4096, 4096, 128, F16, False, classes="C", expect=dict(kernel=ASM, rows=256, nsplit=0, items_gt_cus=True)))
    for (B, H, Nq, Nkv, D, dt, bnhd) in SPLIT_SHAPES:
        out.append(case("split", B, H, Nq, Nkv, D, (F16, BF16)[dt], False, bnhd=bnhd, ws=True, maps="edges", expect=dict(split=True)))
    # head dim 64: the folded fp16 body and the bf16 one (row sums of the rounded P), 264 items (option rows = 256: between 1 and 1.5 rounds the plain
    # fp16 call takes the 128-row compiled kernel)
    out.append(case("d64", 1, 33, 2048, 2048, 64, F16, False, opts=dict(rows=256), maps="edges", expect=dict(kernel=ASM, contract=PRE | P16, nsplit=0)))
    out.append(case("d64", 1, 33, 2048, 2048, 64, BF16, True, maps="edges", expect=dict(kernel=ASM, contract=P16, nsplit=0)))
    for D in (200, 256):                                    # the 128-row hand-scheduled kernel of head dims 136 .. 256
        for dtype, causal in ((F16, False), (BF16, True)):
            out.append(case("d256", 1, 2, 640, 1500, D, dtype, causal, maps="edges", expect=dict(kernel=ASM, rows=128, nsplit=0)))
    for Nkv in (77, 128):                                   # the single-pass short-KV kernel (512 workgroups: without it the 8-wave streaming kernel)
        for D, dtype in ((128, F16), (64, BF16)):
            out.append(case("short_kv", 2, 16, 4096, Nkv, D, dtype, False, maps="edges", expect=dict(kernel=HIP128, rows=128, contract=0, nsplit=0, short=True)))
    for D in (80, 320):                                     # compiler-scheduled kernels
        for dtype, causal in ((F16, False), (BF16, True)):
            out.append(case("compiled", 1, 2, 300, 700, D, dtype, causal, maps="edges", expect=dict(kernel=HIP128, contract=0, nsplit=0)))
    for H, Hkv, dtype, causal in ((32, 8, F16, False), (32, 8, BF16, True), (16, 1, F16, True), (16, 1, BF16, False)):
        out.append(case("grouped", 1, H, 1100, 1984, 128, dtype, causal, Hkv=Hkv, ws=True, maps="edges", expect=dict(gqa=True)))
    return out


FORWARD_CASES = _forward_cases()
WINDOW_CASES = [      # bands that start and end inside a tile, rows that see no key (B2 H4 Hkv2 D128)
    dict(Nq=700, Nkv=900, window=(100, 0), q_offset=200, causal=True), dict(Nq=700, Nkv=900, window=(70, 30), q_offset=5, causal=False),
    dict(Nq=700, Nkv=900, window=(10, 10), q_offset=600, causal=False), dict(Nq=300, Nkv=2000, window=(1000, -1), q_offset=1300, causal=True),
    dict(Nq=130, Nkv=520, window=(-1, 3), q_offset=0, causal=False)]
PACKED_Q = [0, 1, 63, 64, 65, 700]
PACKED_K = [65, 0, 64, 63, 700, 1]      # Nq_s != Nkv_s in all but none: the two causal alignments differ, sequences with no key or no row
# The backward's plan query names the KIND of kernel of each pass and nothing else: "hip" for the dK / dV pass at head dim 128 is the compiled wave-pair pass
# (the only compiled one there), and that a call is split shows only in its workspace size being > 0 — neither is asserted beyond that.
BACKWARD_CASES = [    # route, B, H, Nq, Nkv, D, dtype, causal, ws, classes, (dq kernel, dkv kernel)
    ("plain", 1, 2, 1100, 1984, 128, F16, False, False, "BC", ("asm", "hip")), ("plain", 1, 2, 1100, 1984, 128, F16, True, False, "BC", ("asm", "hip")),
    ("plain", 1, 2, 1100, 1984, 128, BF16, False, False, "BC", ("asm", "hip")), ("plain", 1, 2, 1100, 1984, 128, BF16, True, False, "BC", ("asm", "hip")),
    ("m16_both", 1, 8, 640, 640, 128, F16, True, False, "BC", ("asm", "asm")), ("m16_both", 1, 8, 640, 640, 128, BF16, False, False, "BC", ("asm", "asm")),
    ("wave_pair", 1, 2, 129, 127, 128, F16, True, False, "BC", ("asm", "hip")),
    ("split", 1, 24, 3072, 3072, 64, BF16, False, True, "BC", ("hip", "hip")),
    ("long", 1, 2, 4096, 4096, 128, BF16, True, False, "C", ("asm", "asm")),
]
SEED_C_BWD = 123        # the class-C backward inputs: tests/test_key_probes.py measure_kappa() draws the same
BWD_KERNEL = {"hip": _fa2_lib.FA2_BWD_KERNEL_HIP, "asm": _fa2_lib.FA2_BWD_KERNEL_ASM}


SEED_D = 131            # the class-D inputs of the dense backward cases: tests/test_key_probes.py measure_kappa_d() draws the same
D_KINDS = ("edge", "inner")


def dense_d_inputs(b, kind, device=None):
    """The class-D inputs (tests/key_probes.py) of a BACKWARD_CASES row: targets on ('edge') or one key inside ('inner') the ends of every row's sweep."""
    route, B, H, Nq, Nkv, D, dtype, causal = b[:8]
    lo, hi = kp.row_ranges(Nq, Nkv, causal=causal)
    pa, pb = kp.two_pointer_maps(lo, hi, Nkv, seed=SEED_D, kind=kind)
    return kp.two_pointer_inputs(B, H, H, Nq, Nkv, D, dtype, pa, pb, seed=SEED_D + 1, device=device, visible=_vis(dict(Nq=Nq, Nkv=Nkv, causal=causal), device))


def all_forward_shapes():
    return [(c["B"], c["H"], c["Nq"], c["Nkv"], c["D"]) for c in FORWARD_CASES] + [(2, 4, w["Nq"], w["Nkv"], 128) for w in WINDOW_CASES] + \
        [(1, 4, max(PACKED_Q), max(PACKED_K), 128), (2, 3, 300, 700, 128)]


def maps_of(Nq, Nkv, causal, which="all"):
    kind = "causal" if causal else "shift"
    edges = [("edges_causal" if causal else "edges", 65)]
    if which == "edges":
        return edges + [("perm_causal" if causal else "perm", 0)]
    return [(kind, s) for s in kp.shifts_of(Nkv)] + edges + [("perm_causal" if causal else "perm", 0)]


def pointer_pairs():
    """(D, Nq, Nkv, causal) of every pointer call the tests below make."""
    out = {(c["D"], c["Nq"], c["Nkv"], c["causal"]) for c in FORWARD_CASES if "B" in c["classes"]}
    return out | {(b[5], b[3], b[4], b[7]) for b in BACKWARD_CASES if "B" in b[9]}


# ---------------------------------------------------------------------------------------------------------------- routes
def _empty_qk(c, device):
    mk = lambda h, n: _layout(torch.empty((c["B"], h, n, c["D"]), dtype=c["dtype"], device=device), c["bnhd"])  # noqa: E731
    return mk(c["H"], c["Nq"]), mk(c["Hkv"], c["Nkv"])


def route_of(c, q=None, k=None):
    """The plan of the call forward_call(c, ...) makes, with the route the case is named for asserted.  Runs without a GPU (meta tensors)."""
    lib = _fa2_lib.load()
    if q is None:
        q, k = _empty_qk(c, "meta")
    assert lib.fa2_get_option(b"asm") == FULL_ASM
    dt, e = _code(c["dtype"]), c["expect"]
    with _fa2_lib.options(**c["opts"]):
        if e.get("gqa"):
            need = 0 if c["causal"] else lib.fa2_fwd_gqa_workspace_bytes(dt, c["B"], c["H"], c["Hkv"], c["Nq"], c["Nkv"], c["D"], 0)
            plan = _fa2_lib.gqa_plan(q, k, c["causal"], workspace_bytes=need)
            mha = _fa2_lib.fwd_plan(q, q.new_empty((c["B"], c["H"], c["Nkv"], c["D"])), c["causal"], workspace_bytes=need)
            assert plan.as_dict() == mha.as_dict() and plan.kernel in (ASM, HIP128, HIP256), plan.as_dict()       # the MHA call's kernels, k / v through the group
        else:
            need = lib.fa2_fwd_workspace_bytes(dt, c["B"], c["H"], c["Nq"], c["Nkv"], c["D"], 0) if c["ws"] else 0
            plan = _fa2_lib.fwd_plan(q, k, c["causal"], workspace_bytes=need)
        if e.get("short"):
            with _fa2_lib.options(short=0):
                assert _fa2_lib.fwd_plan(q, k, c["causal"]).rows == 256       # (what would run without the short-KV kernel)
    d = plan.as_dict()
    for name in ("kernel", "rows", "contract", "nsplit"):
        if name in e:
            assert d[name] == e[name], (name, d)
    assert plan.heads_main == c["B"] * c["H"] and plan.kernel_tail == 0, d
    if e.get("split"):
        assert need > 0 and plan.nsplit > 1 and plan.split_items > 0, d
    items = c["B"] * c["H"] * ((c["Nq"] + 255) // 256)
    if e.get("items_gt_cus"):
        assert items > 256        # more items than CUs: workgroups run several items and fetch across the item seam
    if e.get("items_le_cus"):
        assert items <= 256
    return plan, need


def forward_call(c, q, k, v, need):
    """The call of case c on [B,H,N,D] views -> (o like q, lse f32 [B,H,Nq] in log2 units)."""
    lib = _fa2_lib.load(build_if_missing=False)
    B, H, Nq, D = q.shape
    Hkv, Nkv = k.shape[1], k.shape[2]
    o = torch.full_like(q, float("nan"))
    lse = torch.full((B, H, Nq), float("nan"), dtype=torch.float32, device=q.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (_code(q.dtype), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H)
    tail = (Nq, Nkv, D, _s3(q), _s3(k), _s3(v), _s3(o), _fa2_lib.strides2(lse.stride(0), lse.stride(1)), float(D ** -0.5), int(c["causal"]))
    ws = torch.full(((need + 3) // 4 + 4,), float("nan"), dtype=torch.float32, device=q.device) if need else None      # (every byte the merge reads was written by a part)
    with _fa2_lib.options(**c["opts"]):
        if Hkv != H:
            rc = lib.fa2_fwd_gqa(*head, Hkv, *tail, ws.data_ptr() if need else None, need, stream)
        elif need:
            rc = lib.fa2_fwd_ws(*head, *tail, ws.data_ptr(), need, stream)
        else:
            rc = lib.fa2_fwd(*head, *tail, stream)
        _fa2_lib.check(rc)
        torch.cuda.synchronize()
    return o, lse


def _vis(c, device):
    return (~torch.ones(c["Nq"], c["Nkv"], dtype=torch.bool, device=device).triu(1)) if c["causal"] else None


def _contract_of(plan):
    return bool(plan.contract & PRE), bool(plan.contract & P16)


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.gpu
@pytest.mark.parametrize("c", FORWARD_CASES, ids=_id)
def test_forward_routes_on_key_probes(c):
    dev = _dev()
    B, H, Hkv, Nq, Nkv, D, dtype = (c[n] for n in ("B", "H", "Hkv", "Nq", "Nkv", "D", "dtype"))
    fails = []
    if "A" in c["classes"]:
        q, k, v = (_layout(t, c["bnhd"]) for t in kp.counting_inputs(B, H, Hkv, Nq, Nkv, D, dtype, seed=101, device=dev))
        plan, need = route_of(c, q, k)
        o, lse = forward_call(c, q, k, v, need)
        lo, hi = kp.row_ranges(Nq, Nkv, causal=c["causal"], device=dev)
        fails += ["A: " + f for f in kp.check_counting(o, lse, *kp.counting_expect(v, lo, hi, H, dtype, split=plan.nsplit > 1))]
    if "B" in c["classes"]:
        for kind, shift in maps_of(Nq, Nkv, c["causal"], c["maps"]):
            pi = kp.pointer_map(kind, Nq, Nkv, shift, seed=7)
            inp = kp.pointer_inputs(B, H, Hkv, Nq, Nkv, D, dtype, pi, seed=103 + shift, device=dev, visible=_vis(c, dev))
            q, k, v = (_layout(inp[n], c["bnhd"]) for n in "qkv")
            plan, need = route_of(c, q, k)
            folded, p16 = _contract_of(plan)
            o, lse = forward_call(c, q, k, v, need)
            tag = "B %s %d: " % (kind, shift)
            fails += [tag + f for f in kp.check_elements("O", o, *kp.pointer_expect_o(inp, dtype))]
            lerr = float((lse.double() - kp.pointer_expect_lse(inp, dtype, folded=folded)).abs().max())
            if not lerr <= kp.pointer_lse_bar(inp, dtype, p16):
                fails.append(tag + "LSE err %.3e > %.3e" % (lerr, kp.pointer_lse_bar(inp, dtype, p16)))
    if "C" in c["classes"]:
        q, k, v = (_layout(t, c["bnhd"]) for t in kp.random_inputs(B, H, Hkv, Nq, Nkv, D, dtype, seed=105, device=dev))
        plan, need = route_of(c, q, k)
        folded, _ = _contract_of(plan)
        o, _ = forward_call(c, q, k, v, need)
        scale = D ** -0.5
        qr, sr = ((q.float() * (scale * kp.LOG2E)).to(dtype), 1.0 / kp.LOG2E) if folded else (q, scale)       # the prescaled-Q twin, as tools/fuzz_parity.py
        ref = kp.dense64(qr, k, v, sr, causal=c["causal"])
        print("C: worst O err / bar %.3f" % kp.worst_ratio(o, ref["o"], kp.o_bar(ref, dtype)))
        fails += ["C: " + f for f in kp.check_random(ref, dtype, o=o)]
    assert fails == [], fails


def _family_forward(q, k, v, causal, window=None, dropout=None, bias=None):
    """The windowed / dropout / masked entry points through the operator's own front end (BHND) -> (o, lse log2 [B,H,Nq])."""
    ret = flash_attn_wmma.forward_py(q, k, v, 64, 128, bool(causal), q.shape[3] ** -0.5, False, bias=bias, window=window, dropout=dropout)
    torch.cuda.synchronize()
    return ret[0], ret[5][:, :, :q.shape[2]]


@pytest.mark.gpu
@pytest.mark.parametrize("w", WINDOW_CASES, ids=lambda w: "%dx%d-%s-off%d%s" % (w["Nq"], w["Nkv"], w["window"], w["q_offset"], "-causal" if w["causal"] else ""))
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_window_with_q_offset_counts_every_rows_keys(w, dtype):
    dev = _dev()
    B, H, Hkv, D = 2, 4, 2, 128
    q, k, v = kp.counting_inputs(B, H, Hkv, w["Nq"], w["Nkv"], D, dtype, seed=111, device=dev)
    plan = _fa2_lib.window_plan(q, k, w["causal"], w["window"][0], w["window"][1], w["q_offset"])
    assert plan.kernel == _fa2_lib.FA2_KERNEL_HIP_WINDOW and plan.heads_main == B * H, plan.as_dict()
    o, lse = _family_forward(q, k, v, w["causal"], window=(w["window"][0], w["window"][1], w["q_offset"]))
    lo, hi = kp.row_ranges(w["Nq"], w["Nkv"], causal=w["causal"], window=w["window"], q_offset=w["q_offset"], device=dev)
    if w["q_offset"] == 600:
        assert int((hi == lo).sum()) > 0          # rows that see no key
    assert kp.check_counting(o, lse, *kp.counting_expect(v, lo, hi, H, dtype)) == []


@pytest.mark.gpu
@pytest.mark.parametrize("align", ["full", "top_left", "bottom_right"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_packed_batches_count_their_own_keys_only(align, dtype):
    """Lengths 0, 1, 63, 64, 65, 700: a key of the neighbouring sequence, or a row placed under the other causal alignment, changes a count."""
    dev = _dev()
    H, Hkv, D = 4, 2, 128
    cu_q = torch.tensor([0] + PACKED_Q, dtype=torch.int32).cumsum(0).to(torch.int32).to(dev)
    cu_k = torch.tensor([0] + PACKED_K, dtype=torch.int32).cumsum(0).to(torch.int32).to(dev)
    tq, tk = sum(PACKED_Q), sum(PACKED_K)
    q4, k4, v4 = kp.counting_inputs(1, H, Hkv, tq, tk, D, dtype, seed=113, device=dev)
    q, k, v = (t[0].transpose(0, 1).contiguous() for t in (q4, k4, v4))             # [total, H, D]
    flags = {"full": 0, "top_left": _fa2_lib.FA2_FLAG_CAUSAL, "bottom_right": _fa2_lib.FA2_FLAG_CAUSAL | _fa2_lib.FA2_FLAG_BOTTOM_RIGHT}[align]
    plan = _fa2_lib.varlen_plan(q, k, max(PACKED_Q), max(PACKED_K), len(PACKED_Q), flags=flags)
    assert plan.kernel == _fa2_lib.FA2_KERNEL_HIP_VARLEN, plan.as_dict()
    ret = flash_attn_wmma.forward_varlen(q, k, v, cu_q, cu_k, max(PACKED_Q), max(PACKED_K), flags, D ** -0.5, (-1, -1))
    torch.cuda.synchronize()
    o, lse = ret[0], ret[5]                                                       # [total_q, H, D], [H, total_q]
    fails, q0, k0 = [], 0, 0
    for nq, nk in zip(PACKED_Q, PACKED_K):
        if nq:
            lo, hi = kp.row_ranges(nq, nk, causal=align != "full", bottom_right=align == "bottom_right", device=dev)
            exp = kp.counting_expect(v4[:, :, k0:k0 + nk], lo, hi, H, dtype)
            fails += ["%d x %d: %s" % (nq, nk, f) for f in kp.check_counting(o[q0:q0 + nq].transpose(0, 1)[None], lse[None, :, q0:q0 + nq], *exp)]
        q0, k0 = q0 + nq, k0 + nk
    assert fails == [], fails


@pytest.mark.gpu
@pytest.mark.parametrize("per_head", [False, True], ids=["broadcast", "per_head"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_bool_keep_mask_counts_its_popcount(per_head, dtype):
    dev = _dev()
    B, H, Nq, Nkv, D = 2, 3, 300, 700, 128
    q, k, v = kp.counting_inputs(B, H, H, Nq, Nkv, D, dtype, seed=115, device=dev)
    keep = (torch.rand((B, H if per_head else 1, Nq, Nkv), generator=torch.Generator().manual_seed(116)) < 0.5).to(dev)
    plan = _fa2_lib.fwd_plan(q, k, False, bias_kind=_fa2_lib.FA2_BIAS_BOOL)
    assert plan.kernel == _fa2_lib.FA2_KERNEL_HIP_BIAS, plan.as_dict()
    o, lse = _family_forward(q, k, v, False, bias=keep)
    assert kp.check_counting(o, lse, *kp.counting_expect_mask(v, keep, H, dtype)) == []


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_dropout_keeps_the_keys_of_the_librarys_mask(dtype):
    """p = 0.25: O is the sum over the keys the library's host-side keep mask names, divided by count * (1 - p_eff); the LSE is the undropped count's."""
    dev = _dev()
    B, H, Nq, Nkv, D, p, seed = 1, 2, 300, 700, 128, 0.25, 1234
    q, k, v = kp.counting_inputs(B, H, H, Nq, Nkv, D, dtype, seed=117, device=dev)
    # (the dropout calls have no plan query; that the dropout kernels served the call shows in the result: the kept keys are those of the library's mask)
    o, lse = _family_forward(q, k, v, False, window=(-1, -1, 0), dropout=(p, seed))
    kept = dropout_keep_mask(seed, p, B, H, Nq, Nkv).to(dev)
    assert 0.2 < 1.0 - float(kept.float().mean()) < 0.3
    keep = torch.ones((1, 1, Nq, Nkv), dtype=torch.bool, device=dev)
    assert kp.check_counting(o, lse, *kp.counting_expect_mask(v, keep, H, dtype, kept=kept, p_eff=round(p * 65536) / 65536.0)) == []


# ---------------------------------------------------------------------------------------------------------------- backward
def bwd_route_of(b):
    route, B, H, Nq, Nkv, D, dtype, causal, ws, classes, kernels = b
    lib = _fa2_lib.load()
    plan = _fa2_lib.BwdPlan()
    s = lambda n: _fa2_lib.strides3(H * n * D, n * D, D)  # noqa: E731
    _fa2_lib.check(lib.fa2_bwd_plan(_code(dtype), B, H, H, Nq, Nkv, D, s(Nq), s(Nkv), s(Nkv), s(Nq), s(Nq), float(D ** -0.5), int(causal), 0, None, ctypes.byref(plan)))
    assert (plan.dq_kernel, plan.dkv_kernel) == tuple(BWD_KERNEL[x] for x in kernels), (plan.dq_kernel, plan.dkv_kernel)
    need = lib.fa2_bwd_workspace_bytes(_code(dtype), B, H, Nq, Nkv, D, int(causal)) if ws else 0
    assert (need > 0) == ws
    return need


def _fwd_bwd(q, k, v, do, causal, need):
    """The forward of a differentiated call (scores scaled in f32: FA2_FLAG_EXACT_SCALE) and the backward, through the C-ABI on contiguous tensors."""
    lib = _fa2_lib.load(build_if_missing=False)
    B, H, Nq, D = q.shape
    Nkv = k.shape[2]
    dt, scale = _code(q.dtype), float(D ** -0.5)
    o = torch.empty_like(q)
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    delta = torch.empty_like(lse)
    dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
    s2 = _fa2_lib.strides2(lse.stride(0), lse.stride(1))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _fa2_lib.check(lib.fa2_fwd(dt, q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, Nq, Nkv, D, _s3(q), _s3(k), _s3(v), _s3(o), s2,
                               scale, int(causal) | EXACT, stream))
    args = (dt, q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr(),
            B, H, Nq, Nkv, D, _s3(q), _s3(k), _s3(v), _s3(o), _s3(do), _s3(dq), _s3(dk), _s3(dv), s2, scale, int(causal))
    if need:
        ws = torch.full(((need + 3) // 4 + 4,), float("nan"), dtype=torch.float32, device=q.device)
        _fa2_lib.check(lib.fa2_bwd_ws(*args, ws.data_ptr(), need, stream))
    else:
        _fa2_lib.check(lib.fa2_bwd(*args, stream))
    torch.cuda.synchronize()
    return o, dq, dk, dv


@pytest.mark.gpu
@pytest.mark.parametrize("b", BACKWARD_CASES, ids=lambda b: "%s-%dx%dx%dx%dx%d-%s%s" % (b[0], b[1], b[2], b[3], b[4], b[5], "f16" if b[6] == F16 else "bf16", "-causal" if b[7] else ""))
def test_backward_routes_on_key_probes(b):
    route, B, H, Nq, Nkv, D, dtype, causal, ws, classes, kernels = b
    dev = _dev()
    need = bwd_route_of(b)
    scale = D ** -0.5
    fails = []
    c = dict(Nq=Nq, Nkv=Nkv, causal=causal)
    if "B" in classes:
        for kind, shift in maps_of(Nq, Nkv, causal, "edges"):
            pi = kp.pointer_map(kind, Nq, Nkv, shift, seed=9)
            inp = kp.pointer_inputs(B, H, H, Nq, Nkv, D, dtype, pi, seed=121 + shift, device=dev, visible=_vis(c, dev))
            do = torch.randn((B, H, Nq, D), generator=torch.Generator().manual_seed(122)).to(dtype).to(dev)
            o, dq, dk, dv = _fwd_bwd(inp["q"], inp["k"], inp["v"], do, causal, need)
            tag = "B %s %d: " % (kind, shift)
            fails += [tag + f for f in kp.check_elements("O", o, *kp.pointer_expect_o(inp, dtype)) + kp.check_elements("dV", dv, *kp.pointer_expect_dv(inp, do, dtype))]
            ref = kp.dense64(inp["q"], inp["k"], inp["v"], scale, causal=causal, do=do)
            fails += [tag + f for f in kp.check_random(ref, dtype, dq=dq, dk=dk)]
            del ref
    if "C" in classes:
        q, k, v, do = kp.random_inputs(B, H, H, Nq, Nkv, D, dtype, seed=SEED_C_BWD, device=dev, with_do=True)
        o, dq, dk, dv = _fwd_bwd(q, k, v, do, causal, need)
        ref = kp.dense64(q, k, v, scale, causal=causal, do=do)
        print("C: worst err / bar: O %.3f dQ %.3f dK %.3f dV %.3f" % (kp.worst_ratio(o, ref["o"], kp.o_bar(ref, dtype)), kp.worst_ratio(dq, ref["dq"], kp.dq_bar(ref, dtype)),
                                                                      kp.worst_ratio(dk, ref["dk"], kp.dk_bar(ref, dtype)), kp.worst_ratio(dv, ref["dv"], kp.dv_bar(ref, dtype))))
        fails += ["C: " + f for f in kp.check_random(ref, dtype, o=o, dq=dq, dk=dk, dv=dv)]
    assert fails == [], fails


# ---------------------------------------------------------------------------------------------------------------- class D: two-key pointer probes of every backward
# tests/key_probes.py class D: every row puts half its weight on each of two keys that sit ON the ends of its visible interval ("edge") or one key inside
# them ("inner"); O, dQ, dK and dV are held element by element to float64 under the call's own modifiers.  The family backwards walk the transposed band,
# the packed sequences' offsets, the group sum, the regenerated dropout mask and the score modifiers' derivative: a pair dropped or added there moves dQ_i,
# dK_a and dV_a by tens of bars (tests/test_key_probes.py shows it on float64 mutants).  Outputs are NaN before every call.
LN2 = 0.6931471805599453
CAUSAL, BOTTOM_RIGHT = _fa2_lib.FA2_FLAG_CAUSAL, _fa2_lib.FA2_FLAG_BOTTOM_RIGHT
D_WORST = {}            # case id -> {tensor: worst err / bar}: what the run prints (profiles/ keeps one run's)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _s2(t):
    return _fa2_lib.strides2(t.stride(0), t.stride(1))


def _nan_like(*ts):
    return tuple(torch.full_like(t, float("nan")) for t in ts)


def _dt(dtype):
    return "f16" if dtype == F16 else "bf16"


def _report(tag, fails, worst):
    D_WORST[tag] = worst
    print("D %s: worst err / bar %s" % (tag, " ".join("%s %.3f" % (n, x) for n, x in worst.items())))
    return ["%s: %s" % (tag, f) for f in fails]


def _band_of(Nq, Nkv, causal=False, window=(-1, -1), q_offset=0, bottom_right=False, device=None):
    lo, hi = kp.row_ranges(Nq, Nkv, causal=causal, bottom_right=bottom_right, window=window, q_offset=q_offset)
    j = torch.arange(Nkv)[None]
    vis = (j >= lo[:, None]) & (j < hi[:, None])
    return lo, hi, (vis.to(device) if device is not None else vis)


def alibi_bias(slopes, Nq, Nkv, off):
    """-slope_h |i + off - j| as an additive [1 or B, H, Nq, Nkv] float64 tensor (slopes [H] or [B, H])."""
    dist = (torch.arange(Nq, device=slopes.device)[:, None] + off - torch.arange(Nkv, device=slopes.device)[None]).abs().double()
    s = slopes.double().view(-1, slopes.shape[-1]) if slopes.dim() == 2 else slopes.double().view(1, -1)
    return -s[:, :, None, None] * dist


def bhnd_call(inp, causal=False, window=None, bias=None, dropout=None, smod=None, dlse=None, gqa=False, ws_bytes=0, opts=None):
    """Forward (flagged FA2_FLAG_EXACT_SCALE, as every differentiated call) and backward of one [B,H,N,D] call through the C-ABI -> (o, dq, dk, dv).
    window = (left, right, q_offset): the windowed family (fa2_fwd_window / fa2_bwd_window; with dropout = (p, seed) fa2_*_dropout, with smod = (softcap,
    slopes or None) fa2_*_scoremod); bias: fa2_fwd_bias / fa2_bwd_bias (fa2_bwd_bias_ws with ws_bytes); gqa: fa2_fwd_gqa / fa2_bwd_gqa; else fa2_fwd /
    fa2_bwd (fa2_bwd_ws).  dlse (natural-log units, [B,H,Nq]): the family's *_lse entry.  The windowed and masked backwards have no grouped form: grouped
    k / v are expanded for them and dK / dV come back per query head."""
    from rocwmma_fattn.FlashAttn import _prepare_bias
    lib = _fa2_lib.load(build_if_missing=False)
    q, do = inp["q"], inp["do"]
    k, v = inp["k"], inp["v"]
    B, H, Nq, D = q.shape
    Hkv, Nkv = k.shape[1], k.shape[2]
    dt, scale, flags = _code(q.dtype), float(inp["scale"]), (CAUSAL if causal else 0) | EXACT
    o, = _nan_like(q)
    lse = torch.full((B, H, Nq), float("nan"), dtype=torch.float32, device=q.device)
    fwd = (dt, q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H)
    ftail = (Nq, Nkv, D, _s3(q), _s3(k), _s3(v), _s3(o), _s2(lse), scale, flags)
    bias_args = None
    if bias is not None:
        bias_t, kind, bstr = _prepare_bias(bias, B, H, Nq, Nkv, q.dtype, q.device)
        bias_args = (bias_t.data_ptr(), kind, _fa2_lib.strides3(*bstr))
    smod_args = None
    if smod is not None:
        smod_args = (float(smod[0]), None, 0) if smod[1] is None else (float(smod[0]), smod[1].data_ptr(), smod[1].stride(0) if smod[1].dim() == 2 else 0)
    with _fa2_lib.options(**(opts or {})):
        if window is not None:
            name = "fa2_fwd_scoremod" if smod is not None else "fa2_fwd_dropout" if dropout is not None else "fa2_fwd_window"
            extra = smod_args if smod is not None else (float(dropout[0]), int(dropout[1])) if dropout is not None else ()
            rc = getattr(lib, name)(*fwd, Hkv, *ftail, *window, _stream(), *extra)
        elif bias is not None:
            rc = lib.fa2_fwd_bias(*fwd, *ftail, *bias_args, _stream())
        elif gqa:
            rc = lib.fa2_fwd_gqa(*fwd, Hkv, *ftail, None, 0, _stream())
        else:
            rc = lib.fa2_fwd(*fwd, *ftail, _stream())
        _fa2_lib.check(rc)
        torch.cuda.synchronize()
    if not gqa and Hkv != H:
        k, v = (t.repeat_interleave(H // Hkv, dim=1) for t in (k, v))
    dq, dk, dv = _nan_like(q, k, v)
    delta = torch.full_like(lse, float("nan"))
    ws = torch.full(((ws_bytes + 3) // 4 + 4,), float("nan"), dtype=torch.float32, device=q.device) if ws_bytes else None
    ws_args = (ws.data_ptr() if ws_bytes else None, ws_bytes)
    head = (dt, q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), B, H)
    tail = (Nq, Nkv, D, *(_s3(t) for t in (q, k, v, o, do, dq, dk, dv)), _s2(lse), scale, int(causal))
    if dlse is not None:
        g = (dlse.float() * LN2).contiguous()
        g_args = (g.data_ptr(), _s2(g))
    if gqa:
        assert dlse is None
        rc = lib.fa2_bwd_gqa(*head, Hkv, *tail, *ws_args, _stream())
    elif window is not None:
        if dlse is not None:
            rc = lib.fa2_bwd_window_lse(*head, *tail, *window, _stream(), *((0.0, 0) if dropout is None else (float(dropout[0]), int(dropout[1]))),
                                        *(smod_args or (0.0, None, 0)), *g_args)
        elif smod is not None:
            rc = lib.fa2_bwd_scoremod(*head, *tail, *window, _stream(), *smod_args)
        elif dropout is not None:
            rc = lib.fa2_bwd_dropout(*head, *tail, *window, _stream(), float(dropout[0]), int(dropout[1]))
        else:
            rc = lib.fa2_bwd_window(*head, *tail, *window, _stream())
    elif dlse is not None:
        rc = lib.fa2_bwd_lse(*head, *tail, *(bias_args or (None, _fa2_lib.FA2_BIAS_NONE, None)), *ws_args, _stream(), *g_args)
    elif bias is not None:
        rc = lib.fa2_bwd_bias_ws(*head, *tail, *bias_args, *ws_args, _stream()) if ws_bytes else lib.fa2_bwd_bias(*head, *tail, *bias_args, _stream())
    else:
        rc = lib.fa2_bwd_ws(*head, *tail, *ws_args, _stream()) if ws_bytes else lib.fa2_bwd(*head, *tail, _stream())
    _fa2_lib.check(rc)
    torch.cuda.synchronize()
    return o, dq, dk, dv


def _dlse_of(B, H, Nq, seed, device):
    return torch.randn((B, H, Nq), generator=torch.Generator().manual_seed(seed)).to(device or "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("b", [b for b in BACKWARD_CASES if "B" in b[9]], ids=lambda b: "%s-%dx%dx%dx%dx%d-%s%s" % (b[0], b[1], b[2], b[3], b[4], b[5], "f16" if b[6] == F16 else "bf16", "-causal" if b[7] else ""))
def test_dense_backward_resolves_both_targets_of_every_row(b):
    """Class D on every dense backward route; the plain fp16 rows also through fa2_bwd_lse with a gradient for the LSE (the reference adds P dlse)."""
    route, B, H, Nq, Nkv, D, dtype, causal, ws, classes, kernels = b
    dev = _dev()
    need = bwd_route_of(b)
    fails = []
    for kind in D_KINDS if causal else D_KINDS[:1]:          # (full attention has no band edge: both kinds draw the same uniform targets)
        inp = dense_d_inputs(b, kind, dev)
        o, dq, dk, dv = bhnd_call(inp, causal=causal, ws_bytes=need)
        fails += _report("%s %dx%d %s%s %s" % (route, Nq, Nkv, _dt(dtype), " causal" if causal else "", kind), *kp.check_two_pointer(inp, dtype, o, dq, dk, dv))
    if route == "plain" and dtype == F16:
        plan = _fa2_lib.BwdPlan()
        s = _fa2_lib.strides3(H * Nq * D, Nq * D, D), _fa2_lib.strides3(H * Nkv * D, Nkv * D, D)
        _fa2_lib.check(_fa2_lib.load().fa2_bwd_lse_plan(_code(dtype), B, H, H, Nq, Nkv, D, s[0], s[1], s[1], s[0], s[0], float(D ** -0.5), int(causal), 0, None, 1,
                                                        ctypes.byref(plan)))
        assert (plan.dq_kernel, plan.dkv_kernel) == (BWD_KERNEL["hip"], BWD_KERNEL["hip"]), (plan.dq_kernel, plan.dkv_kernel)      # a dlse: no hand-scheduled pass
        dlse = _dlse_of(B, H, Nq, 141, dev)
        lo, hi = kp.row_ranges(Nq, Nkv, causal=causal)
        pa, pb = kp.two_pointer_maps(lo, hi, Nkv, seed=SEED_D, kind="edge")
        inp = kp.two_pointer_inputs(B, H, H, Nq, Nkv, D, dtype, pa, pb, seed=SEED_D + 1, device=dev, visible=_vis(dict(Nq=Nq, Nkv=Nkv, causal=causal), dev), dlse=dlse)
        o, dq, dk, dv = bhnd_call(inp, causal=causal, dlse=dlse)
        fails += _report("%s %dx%d %s%s lse" % (route, Nq, Nkv, _dt(dtype), " causal" if causal else ""), *kp.check_two_pointer(inp, dtype, o, dq, dk, dv))
    assert fails == [], fails


def window_d_cases():
    out = []
    for wi, w in enumerate(WINDOW_CASES):
        for dtype in (F16, BF16):
            out.append(dict(w, D=128, dtype=dtype, rows=None, dlse=(wi == 1 and dtype == BF16)))
    out.append(dict(WINDOW_CASES[0], D=64, dtype=F16, rows=None, dlse=False))
    out.append(dict(WINDOW_CASES[1], D=64, dtype=BF16, rows=None, dlse=False))
    out.append(dict(WINDOW_CASES[2], D=256, dtype=BF16, rows=None, dlse=False))
    out.append(dict(WINDOW_CASES[1], D=128, dtype=F16, rows=128, dlse=False))       # the forward's option "rows"
    out.append(dict(WINDOW_CASES[1], D=128, dtype=F16, rows=256, dlse=False))
    return out


def _wid(w):
    return "%dx%dx%d-%s-off%d%s-%s%s%s" % (w["Nq"], w["Nkv"], w["D"], w["window"], w["q_offset"], "-causal" if w["causal"] else "", "f16" if w["dtype"] == F16 else "bf16",
                                         "-rows%d" % w["rows"] if w["rows"] else "", "-lse" if w["dlse"] else "")


def window_d_inputs(w, kind, device=None, B=2, H=4, Hkv=2, dlse=None):
    lo, hi, vis = _band_of(w["Nq"], w["Nkv"], causal=w["causal"], window=w["window"], q_offset=w["q_offset"], device=device)
    pa, pb = kp.two_pointer_maps(lo, hi, w["Nkv"], seed=SEED_D + 2, kind=kind)
    return kp.two_pointer_inputs(B, H, Hkv, w["Nq"], w["Nkv"], w["D"], w["dtype"], pa, pb, seed=SEED_D + 3, device=device, visible=vis, dlse=dlse, per_query_head=True)


@pytest.mark.gpu
@pytest.mark.parametrize("w", window_d_cases(), ids=_wid)
def test_window_backward_resolves_the_band_edges(w):
    """fa2_bwd_window (grouped k / v B2 H4 Hkv2 in the forward, expanded for the backward, which has no grouped form: dK / dV per query head)."""
    dev = _dev()
    B, H, Hkv = 2, 4, 2
    win = (w["window"][0], w["window"][1], w["q_offset"])
    fails = []
    for kind in D_KINDS:
        dlse = _dlse_of(B, H, w["Nq"], 143, dev) if w["dlse"] else None
        inp = window_d_inputs(w, kind, dev, B, H, Hkv, dlse)
        with _fa2_lib.options(**({"rows": w["rows"]} if w["rows"] else {})):
            plan = _fa2_lib.window_plan(inp["q"], inp["k"], w["causal"], *win)
        assert plan.kernel == _fa2_lib.FA2_KERNEL_HIP_WINDOW and plan.heads_main == B * H, plan.as_dict()
        assert plan.rows == (w["rows"] or 128), plan.as_dict()               # (the option reached the plan; D = 256 has no 256-row form and is not asked for one)
        o, dq, dk, dv = bhnd_call(inp, causal=w["causal"], window=win, dlse=dlse, opts={"rows": w["rows"]} if w["rows"] else None)
        fails += _report("window %s %s" % (_wid(w), kind), *kp.check_two_pointer(inp, w["dtype"], o, dq, dk, dv))
    assert fails == [], fails


GROUPED_D = [(32, 8, F16, False), (32, 8, BF16, True), (16, 1, F16, True), (16, 1, BF16, False)]


def grouped_d_inputs(g, kind, device=None, H=None, Hkv=None):
    B, Nq, Nkv, D = 1, 1100, 1984, 128
    lo, hi, vis = _band_of(Nq, Nkv, causal=g[3], device=device)
    pa, pb = kp.two_pointer_maps(lo, hi, Nkv, seed=SEED_D + 4, kind=kind)
    return kp.two_pointer_inputs(B, H or g[0], Hkv or g[1], Nq, Nkv, D, g[2], pa, pb, seed=SEED_D + 5, device=device, visible=vis if g[3] else None,
                                 spread_group=g[2] == BF16)           # (bf16: one pointing head per row, see the builder)


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPED_D, ids=lambda g: "h%d-hkv%d-%s%s" % (g[0], g[1], "f16" if g[2] == F16 else "bf16", "-causal" if g[3] else ""))
def test_grouped_backward_sums_every_head_of_a_group(g):
    """fa2_bwd_gqa through the C-ABI at 1100 x 1984 (the in-kernel group sum: every query head of a group points at the same two keys, a head left out of the
    sum takes 1 / g of dK_a and dV_a with it); H16 / Hkv1 causal also through the operator's expanded path."""
    H, Hkv, dtype, causal = g
    dev = _dev()
    B, Nq, Nkv, D = 1, 1100, 1984, 128
    lib = _fa2_lib.load()
    plan = _fa2_lib.BwdPlan()
    s = lambda h, n: _fa2_lib.strides3(h * n * D, n * D, D)  # noqa: E731
    _fa2_lib.check(lib.fa2_bwd_plan(_code(dtype), B, H, Hkv, Nq, Nkv, D, s(H, Nq), s(Hkv, Nkv), s(Hkv, Nkv), s(H, Nq), s(H, Nq), float(D ** -0.5), int(causal), 0, None,
                                    ctypes.byref(plan)))
    # as the dense "plain" rows of this size: the hand-scheduled dQ pass per query head, the compiler-scheduled dK / dV pass with the in-kernel group sum
    assert (plan.dq_kernel, plan.dkv_kernel) == (BWD_KERNEL["asm"], BWD_KERNEL["hip"]), (plan.dq_kernel, plan.dkv_kernel)
    fails = []
    for kind in D_KINDS if causal else D_KINDS[:1]:
        inp = grouped_d_inputs(g, kind, dev)
        o, dq, dk, dv = bhnd_call(inp, causal=causal, gqa=True)
        fails += _report("gqa h%d/%d %s%s %s" % (H, Hkv, _dt(dtype), " causal" if causal else "", kind), *kp.check_two_pointer(inp, dtype, o, dq, dk, dv))
        if (H, Hkv, causal) == (16, 1, True) and kind == "edge":
            ret = flash_attn_wmma.forward_py(inp["q"], inp["k"], inp["v"], 64, 128, CAUSAL | EXACT, inp["scale"], False)
            dq2, dk2, dv2 = flash_attn_wmma.backward_py(ret[1], ret[2], ret[3], ret[4], inp["do"], ret[5], Nq, Nkv, D, 64, 128, True, inp["scale"], False)
            torch.cuda.synchronize()
            fails += _report("gqa h%d/%d %s causal operator" % (H, Hkv, _dt(dtype)), *kp.check_two_pointer(inp, dtype, ret[0], dq2, dk2, dv2))
    assert fails == [], fails


def _packed_d(align, dtype, dev, H=4, Hkv=2, D=128, window=(-1, -1), dropout=None, smod=None, dlse_seed=None):
    """Per sequence of PACKED_Q / PACKED_K: class-D inputs of its own band -> packed q, k, v, do, the per-sequence inputs (None where a sequence has no row
    or no key) and the per-sequence modifiers."""
    g = torch.Generator().manual_seed(151)
    parts, seqs = dict(q=[], k=[], v=[], do=[]), []
    kept_all = dropout_keep_mask(dropout[1], dropout[0], len(PACKED_Q), H, max(PACKED_Q), max(PACKED_K)) if dropout else None
    for s_, (nq, nk) in enumerate(zip(PACKED_Q, PACKED_K)):
        inp = None
        if nq and nk:
            lo, hi, vis = _band_of(nq, nk, causal=align != "full", bottom_right=align == "bottom_right", window=window, device=dev)
            kw = dict(visible=vis)
            if dropout:
                kept = kept_all[s_:s_ + 1, :, :nq, :nk].to(dev)
                pa, pb = kp.two_pointer_maps(None, None, nk, 0, keep=(vis & kept)[0].view(Hkv, H // Hkv, nq, nk).all(1)[None])
                kw.update(kept=kept, rs=1.0 / (1.0 - round(dropout[0] * 65536) / 65536.0))
            else:
                pa, pb = kp.two_pointer_maps(lo, hi, nk, seed=SEED_D + 6 + s_, kind="edge")
            if smod:
                kw["softcap"] = smod[0]
                if smod[1] is not None:
                    kw["bias"] = alibi_bias(smod[1], nq, nk, (nk - nq) if align == "bottom_right" else 0)
            if dlse_seed is not None:
                kw["dlse"] = _dlse_of(1, H, nq, dlse_seed + s_, dev)
            inp = kp.two_pointer_inputs(1, H, Hkv, nq, nk, D, dtype, pa, pb, seed=SEED_D + 20 + s_, device=dev, per_query_head=True, **kw)
        seqs.append(inp)
        parts["q"].append(inp["q"][0] if inp else torch.zeros((H, nq, D), dtype=dtype, device=dev))
        parts["do"].append(inp["do"][0] if inp else torch.randn((H, nq, D), generator=g).to(dtype).to(dev))
        for n in "kv":
            parts[n].append(inp[n][0] if inp else torch.randn((Hkv, nk, D), generator=g).to(dtype).to(dev))
    packed = {n: torch.cat(ts, dim=1).transpose(0, 1).contiguous() for n, ts in parts.items()}           # [total, heads, D]
    return packed, seqs


def packed_call(p, H, Hkv, D, flags, window=(-1, -1), dropout=None, smod=None, dlse=None):
    """fa2_fwd_varlen* / fa2_bwd_varlen* on [total, heads, D] tensors (k / v expanded for the backward) -> (o, dq, dk, dv per query head)."""
    lib = _fa2_lib.load(build_if_missing=False)
    dev = p["q"].device
    cu_q = torch.tensor([0] + PACKED_Q, dtype=torch.int32).cumsum(0).to(torch.int32).to(dev)
    cu_k = torch.tensor([0] + PACKED_K, dtype=torch.int32).cumsum(0).to(torch.int32).to(dev)
    q, k, v, do = p["q"], p["k"], p["v"], p["do"]
    dt, scale, nseq = _code(q.dtype), float(D ** -0.5), len(PACKED_Q)
    s2 = lambda t: _fa2_lib.strides2(t.stride(1), t.stride(0))  # noqa: E731
    o, = _nan_like(q)
    lse = torch.full((H, q.shape[0]), float("nan"), dtype=torch.float32, device=dev)
    extra = ()
    if smod is not None:
        extra = (float(smod[0]), None, 0) if smod[1] is None else (float(smod[0]), smod[1].data_ptr(), 0)
    elif dropout is not None:
        extra = (float(dropout[0]), int(dropout[1]))
    name = "_scoremod" if smod is not None else "_dropout" if dropout is not None else ""
    _fa2_lib.check(getattr(lib, "fa2_fwd_varlen" + name)(dt, q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), nseq, H, Hkv, max(PACKED_Q), max(PACKED_K), D,
                                                         cu_q.data_ptr(), cu_k.data_ptr(), s2(q), s2(k), s2(v), s2(o), lse.stride(0), scale, flags | EXACT, window[0], window[1],
                                                         _stream(), *extra))
    torch.cuda.synchronize()
    k, v = (t.repeat_interleave(H // Hkv, dim=1) for t in (k, v))
    dq, dk, dv = _nan_like(q, k, v)
    delta = torch.full_like(lse, float("nan"))
    args = (dt, q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), nseq, H,
            max(PACKED_Q), max(PACKED_K), D, cu_q.data_ptr(), cu_k.data_ptr(), *(s2(t) for t in (q, k, v, o, do, dq, dk, dv)), lse.stride(0), scale, flags, window[0], window[1], _stream())
    if dlse is not None:
        g = (dlse.float() * LN2).contiguous()
        rc = lib.fa2_bwd_varlen_lse(*args, *((0.0, 0) if dropout is None else extra), *((0.0, None, 0) if smod is None else extra), g.data_ptr(), g.stride(0))
    else:
        rc = getattr(lib, "fa2_bwd_varlen" + name)(*args, *extra)
    _fa2_lib.check(rc)
    torch.cuda.synchronize()
    return o, dq, dk, dv


def _check_packed(tag, seqs, dtype, o, dq, dk, dv):
    """Per sequence, as the forward test: class D where the sequence has rows and keys; O = dQ = 0 for rows without keys, dK = dV = 0 for keys without rows."""
    fails, q0, k0 = [], 0, 0
    for s_, (nq, nk) in enumerate(zip(PACKED_Q, PACKED_K)):
        sl = lambda t, a, n: t[a:a + n].transpose(0, 1)[None]  # noqa: E731
        if seqs[s_] is not None:
            fails += _report("%s seq %d (%d x %d)" % (tag, s_, nq, nk), *kp.check_two_pointer(seqs[s_], dtype, sl(o, q0, nq), sl(dq, q0, nq), sl(dk, k0, nk), sl(dv, k0, nk)))
        else:
            for name, t in (("O", sl(o, q0, nq)), ("dQ", sl(dq, q0, nq)), ("dK", sl(dk, k0, nk)), ("dV", sl(dv, k0, nk))):
                if not bool((t == 0).all()):
                    fails.append("%s seq %d (%d x %d): %s is not exactly 0" % (tag, s_, nq, nk, name))
        q0, k0 = q0 + nq, k0 + nk
    return fails


PACKED_D = [("full", (-1, -1), False), ("top_left", (-1, -1), False), ("bottom_right", (-1, -1), True), ("bottom_right", (40, 0), False)]


@pytest.mark.gpu
@pytest.mark.parametrize("pc", PACKED_D, ids=lambda pc: "%s%s%s" % (pc[0], "-w%d" % pc[1][0] if pc[1][0] >= 0 else "", "-lse" if pc[2] else ""))
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_packed_backward_resolves_every_sequences_edges(pc, dtype):
    """fa2_bwd_varlen on the lengths 0, 1, 63, 64, 65, 700 against 65, 0, 64, 63, 700, 1: the targets sit on the first and last key each row of each sequence
    may see under the alignment, so a sequence read one key early or late, or a row placed under the other alignment, drops a pair."""
    align, window, with_lse = pc
    dev = _dev()
    H, Hkv, D = 4, 2, 128
    flags = {"full": 0, "top_left": CAUSAL, "bottom_right": CAUSAL | BOTTOM_RIGHT}[align]
    packed, seqs = _packed_d(align, dtype, dev, H, Hkv, D, window=window, dlse_seed=161 if with_lse else None)
    plan = _fa2_lib.varlen_plan(packed["q"], packed["k"], max(PACKED_Q), max(PACKED_K), len(PACKED_Q), flags=flags, window_left=window[0], window_right=window[1])
    assert plan.kernel == _fa2_lib.FA2_KERNEL_HIP_VARLEN, plan.as_dict()
    dlse = None
    if with_lse:
        dlse = torch.cat([s["dlse"][0] if s is not None else torch.zeros((H, nq), device=dev) for s, nq in zip(seqs, PACKED_Q)], dim=1)      # [H, total_q]
    o, dq, dk, dv = packed_call(packed, H, Hkv, D, flags, window=window, dlse=dlse)
    fails = _check_packed("packed %s%s%s %s" % (align, " w%d" % window[0] if window[0] >= 0 else "", " lse" if with_lse else "", _dt(dtype)), seqs, dtype, o, dq, dk, dv)
    assert fails == [], fails


MASK_D = [("bool_broadcast", 2, 3, 300, 700, False), ("bool_per_head", 2, 3, 300, 700, False), ("f32_additive", 2, 3, 300, 700, False), ("bool_broadcast", 1, 2, 1100, 1984, True),
          ("bool_per_head_lse", 2, 3, 300, 700, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("m", MASK_D, ids=lambda m: "%s-%dx%dx%dx%d%s" % (m[0], m[1], m[2], m[3], m[4], "-ws" if m[5] else ""))
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_masked_backward_resolves_the_first_and_last_kept_key(m, dtype):
    """fa2_bwd_bias / fa2_bwd_bias_ws under a bool keep mask (broadcast over the heads, or one per head) and an additive f32 mask (-inf where the same
    pattern drops a key, N(0, 1/4) elsewhere): the targets are each row's first and last kept key.  The mask is a random half of a band of 101 keys that
    moves along the rows — of a random half of ALL keys the first kept one is key 0 or 1 for three rows in four, and no element of dK_0 resolves one of
    150 summands (the builder refuses it: the power condition)."""
    kind, B, H, Nq, Nkv, ws = m
    dev = _dev()
    D = 128
    inp, mask, bias_kind, dlse = mask_d_inputs(m, dtype, dev)
    plan = _fa2_lib.fwd_plan(inp["q"], inp["k"], False, bias_kind=bias_kind)
    assert plan.kernel == _fa2_lib.FA2_KERNEL_HIP_BIAS, plan.as_dict()
    need = _fa2_lib.load().fa2_bwd_bias_workspace_bytes(_code(dtype), B, H, Nq, Nkv, D, 0) if ws else 0
    assert (need > 0) == ws
    o, dq, dk, dv = bhnd_call(inp, bias=mask, ws_bytes=need, dlse=dlse)
    fails = _report("mask %s%s %s" % (kind, " ws" if ws else "", _dt(dtype)), *kp.check_two_pointer(inp, dtype, o, dq, dk, dv))
    assert fails == [], fails


def mask_d_inputs(m, dtype, dev=None, B=None, H=None):
    kind, B0, H0, Nq, Nkv, ws = m
    B, H, D = B or B0, H or H0, 128
    gen = torch.Generator().manual_seed(171)
    keep = (torch.rand((B, 1 if kind == "bool_broadcast" else H, Nq, Nkv), generator=gen) < 0.5).to(dev or "cpu") & _band_of(Nq, Nkv, window=(70, 30), q_offset=(Nkv - Nq) // 2, device=dev)[2]
    pa, pb = kp.two_pointer_maps(None, None, Nkv, 0, keep=keep)
    if kind == "f32_additive":
        mask = torch.where(keep, (torch.randn(keep.shape, generator=gen) * 0.5).to(dev), torch.full(keep.shape, float("-inf"), device=dev)).float()
        kw, bias_kind = dict(bias=mask), _fa2_lib.FA2_BIAS_F32
    else:
        mask, kw, bias_kind = keep, dict(visible=keep), _fa2_lib.FA2_BIAS_BOOL
    dlse = _dlse_of(B, H, Nq, 173, dev) if kind.endswith("_lse") else None
    return kp.two_pointer_inputs(B, H, H, Nq, Nkv, D, dtype, pa, pb, seed=SEED_D + 40, device=dev, dlse=dlse, **kw), mask, bias_kind, dlse


DROP_P, DROP_SEED = 0.25, 1234


@pytest.mark.gpu
@pytest.mark.parametrize("with_lse", [False, True], ids=["plain", "lse"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_dropout_backward_regenerates_the_forwards_mask(dtype, with_lse):
    """fa2_bwd_dropout at p = 0.25 (B1 H2 300 x 700, band (70, 30) at offset 200: without a band three rows in four have key 0 as their first kept key,
    and the builder refuses such a fan-in): the targets are each row's first and last visible key that the library's host keep mask keeps,
    P kept / (1 - p_eff) multiplies V and dO.  A backward that regenerates another mask (transposed, another head's) drops a target."""
    dev = _dev()
    inp, win, dlse = dropout_d_inputs(dtype, with_lse, dev)
    o, dq, dk, dv = bhnd_call(inp, window=win, dropout=(DROP_P, DROP_SEED), dlse=dlse)
    fails = _report("dropout%s %s" % (" lse" if with_lse else "", _dt(dtype)), *kp.check_two_pointer(inp, dtype, o, dq, dk, dv))
    assert fails == [], fails


def dropout_d_inputs(dtype, with_lse, dev=None):
    B, H, Nq, Nkv, D = 1, 2, 300, 700, 128
    win = (70, 30, 200)
    vis = _band_of(Nq, Nkv, window=win[:2], q_offset=win[2], device=dev)[2]
    kept = dropout_keep_mask(DROP_SEED, DROP_P, B, H, Nq, Nkv).to(dev or "cpu")
    pa, pb = kp.two_pointer_maps(None, None, Nkv, 0, keep=kept & vis)
    dlse = _dlse_of(B, H, Nq, 175, dev) if with_lse else None
    inp = kp.two_pointer_inputs(B, H, H, Nq, Nkv, D, dtype, pa, pb, seed=SEED_D + 50, device=dev, visible=vis, kept=kept, rs=1.0 / (1.0 - round(DROP_P * 65536) / 65536.0), dlse=dlse)
    return inp, win, dlse


def _slopes(H, width, device):
    """Geometric slopes 3 / width, halved from head to head: slope * width of order 1 (ALiBi balance: the nearer target wins by exp(slope * the difference of
    the two distances), and the farther one must keep its power: the builder checks it)."""
    return (torch.tensor([2.0 ** -(h % 4) for h in range(H)], dtype=torch.float32) * (3.0 / width)).to(device or "cpu")


SCOREMOD_D = [("softcap", (-1, -1), 0, False, False), ("slopes", (70, 30), 5, False, False), ("both", (70, 30), 5, False, False), ("both_lse", (60, 40), 200, False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("sm", SCOREMOD_D, ids=lambda sm: sm[0])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_scoremod_backward_carries_the_cap_and_the_slopes(dtype, sm):
    """fa2_bwd_scoremod (B2 H4 Hkv2, 700 x 900): soft-capping at 1.5 times the targets' score (tanh' = 0.6 on the targets: a backward without 1 - tanh^2 is
    1.6 times off on every pair), ALiBi slopes of 1 / width .. 1 / (8 width) under a band (P_a != P_b; a distance off by one moves the ratio by e^slope)."""
    kind, window, off, causal, with_lse = sm
    dev = _dev()
    inp, cap, slopes, dlse = scoremod_d_inputs(sm, dtype, dev)
    o, dq, dk, dv = bhnd_call(inp, causal=causal, window=(window[0], window[1], off), smod=(cap, slopes), dlse=dlse)
    fails = _report("scoremod %s %s" % (kind, _dt(dtype)), *kp.check_two_pointer(inp, dtype, o, dq, dk, dv))
    assert fails == [], fails


def scoremod_d_inputs(sm, dtype, dev=None, B=2):
    kind, window, off, causal, with_lse = sm
    H, Hkv, Nq, Nkv, D = 4, 2, 700, 900, 128
    lo, hi, vis = _band_of(Nq, Nkv, causal=causal, window=window, q_offset=off, device=dev)
    pa, pb = kp.two_pointer_maps(lo, hi, Nkv, seed=SEED_D + 60, kind="edge")
    width = 101 if window[0] >= 0 else Nkv
    slopes = _slopes(H, width, dev) if kind != "softcap" else None
    cap = 0.0 if kind == "slopes" else 1.5 * 4.0 * D * D ** -0.5          # (the targets score about scale c D at c = 4)
    dlse = _dlse_of(B, H, Nq, 177, dev) if with_lse else None
    inp = kp.two_pointer_inputs(B, H, Hkv, Nq, Nkv, D, dtype, pa, pb, seed=SEED_D + 61, device=dev, visible=vis, softcap=cap,
                                bias=alibi_bias(slopes, Nq, Nkv, off) if slopes is not None else None, dlse=dlse, per_query_head=True)
    return inp, cap, slopes, dlse


def tiny_p_inputs(softcap, dtype=F16, device=None, N=192, D=128, i0=148, j0=150, c=4.0):
    """One (row, key) pair whose P is below half of fp16's smallest subnormal, alone under its key.  Every row points at its own key (q_i = c K_i, K of +-1:
    P_ii = 1 - 1e-19), row j0 at key j0 - 1; k_j0 is K_i0 with m signs flipped, so row i0 scores it scale c 2 m below its own key: P = 1.0e-8 (2^-26.5) with m = 26, and
    with m = 33 under a cap of 1.5 times the own score.  dO_i0 = 2 (v_j0 - v_i0) makes dP - delta ~ 500, so dS / scale is 5e-6, some 80 fp16 subnormal
    steps, and dK_j0 = scale dS q_i0 is 2e-6 per element.  Under the band (3, 3) six other rows see key j0, each with P ~ e^-45: dK_j0 is that one pair."""
    g = torch.Generator().manual_seed(191)
    scale = D ** -0.5
    k = torch.where(torch.rand((1, 1, N, D), generator=g) < 0.5, -1.0, 1.0)
    m = 33 if softcap else 26
    k[0, 0, j0] = k[0, 0, i0]
    k[0, 0, j0, :m] *= -1.0
    q = c * k
    q[0, 0, j0] = q[0, 0, j0 - 1]                  # (row j0 points at its neighbour's key: no row puts weight on key j0)
    v = torch.randn((1, 1, N, D), generator=g)
    do = torch.randn((1, 1, N, D), generator=g)
    do[0, 0, i0] = 2.0 * (v[0, 0, j0] - v[0, 0, i0])
    q, k, v, do = (t.to(dtype).to(device or "cpu") for t in (q, k, v, do))
    vis = _band_of(N, N, window=(3, 3), device=device)[2]
    ref = kp.dense64(q, k, v, scale, keep=vis, do=do, softcap=softcap)
    return dict(q=q, k=k, v=v, do=do, scale=scale, ref=ref, Hkv=1, per_query_head=True, i0=i0, j0=j0)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["window", "scoremod"])
def test_pair_pass_keeps_a_pair_whose_p_is_below_fp16(family):
    """The reduced form of the class-D failure of fa2_bwd_scoremod in fp16: the wave-pair dK / dV pass (head dims 65..128) handed round16(P) from its P
    wave to its dS wave, so a pair with P below 2^-25 gave dK nothing, and a key resting on one such pair came back 0 against a true 2.2e-7.  The pass now
    hands over round16(2^14 P).  Here dK of key j0 is one pair of P = 1e-8: the reference alone puts it above 4 of its bars, so a 0 fails; fa2_bwd_window
    runs the plain form of the pass, fa2_bwd_scoremod (soft-capping) the one that carries P (1 - tanh^2)."""
    dev = _dev()
    cap = 1.5 * 4.0 * 128 * 128 ** -0.5 if family == "scoremod" else 0.0
    inp = tiny_p_inputs(cap, F16, dev)
    ref, i0, j0 = inp["ref"], inp["i0"], inp["j0"]
    bar = kp.dk_bar_d(ref, F16)[0, 0, j0]
    assert float((ref["dk"][0, 0, j0].abs() / bar).min()) >= kp.POWER_D, "the inputs do not resolve the pair"
    plan = _fa2_lib.window_plan(inp["q"], inp["k"], False, 3, 3, 0)
    assert plan.kernel == _fa2_lib.FA2_KERNEL_HIP_WINDOW, plan.as_dict()
    o, dq, dk, dv = bhnd_call(inp, window=(3, 3, 0), smod=(cap, None) if cap else None)
    fails = _report("tiny P %s f16" % family, *kp.check_two_pointer(inp, F16, o, dq, dk, dv))
    assert fails == [], fails


@pytest.mark.gpu
@pytest.mark.parametrize("twin", ["dropout", "scoremod"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_packed_twins_of_dropout_and_scoremod(dtype, twin):
    """fa2_bwd_varlen_dropout (the mask is keyed by the sequence and the positions inside it) and fa2_bwd_varlen_scoremod (soft-capping and slopes [H], the
    distances counted inside the sequence, bottom-right) on the packed lengths."""
    dev = _dev()
    H, Hkv, D = 4, 2, 128
    align, flags = "bottom_right", CAUSAL | BOTTOM_RIGHT
    window = (40, 0)          # (a band: of all keys the first kept one is key 0 for most rows, too many for one dK element; slopes 3 / 101 .. 3 / 808 on distances up to 40)
    dropout = (DROP_P, DROP_SEED) if twin == "dropout" else None
    smod = (1.5 * 4.0 * D * D ** -0.5, _slopes(H, 101, dev)) if twin == "scoremod" else None
    packed, seqs = _packed_d(align, dtype, dev, H, Hkv, D, window=window, dropout=dropout, smod=smod)
    o, dq, dk, dv = packed_call(packed, H, Hkv, D, flags, window=window, dropout=dropout, smod=smod)
    fails = _check_packed("packed %s %s" % (twin, _dt(dtype)), seqs, dtype, o, dq, dk, dv)
    assert fails == [], fails
