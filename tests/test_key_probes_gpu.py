"""GPU tests (`-m gpu`) of the dense forward and backward on the inputs of tests/key_probes.py: counting inputs (A), pointer inputs (B) and random inputs
with per-element bars (C).  The bars do not grow with the sweep: one (row, key) pair missed at Nkv = 4096 fails A's LSE (one count) or B's O (the row
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
