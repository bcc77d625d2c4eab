"""The compiled shell of the hand-scheduled forward kernels (csrc/fa2_fwd_d128.hip.h) on the GPU: the persistent loop that locates and describes
each item once, the interior / ragged O stores, the LDS flag words and the redo path.

Every case is checked against dense float64 attention.  O and LSE live inside larger buffers filled with a NaN sentinel, and nothing outside rows
< Nq and columns < D may change: the unpredicated store of interior tiles and the predicated one of ragged tiles are where a stray store would
come from.

Tolerances are conftest's, by the contract fa2_fwd_plan reports:
  O    |O - O_true| <= FLOOR[dt] + RTOL[dt] * |O_true| — the floor of the truth comparison, plus the one-ulp relative term of the oracle comparison
       (it only matters in the large-logit case, whose rows are near one-hot and return values of |V| up to 4: one ulp there is above the floor);
  LSE  a launch that pre-scales Q in the I/O dtype: LSE_TRUTH_TOL[dt]; bf16 row sums of rounded P: LSE_TOL_P16_BF16; otherwise LSE_TOL.
The large-logit case (scores of hundreds of log2 units) takes its float64 attention under the planned contract: where the launch pre-scales Q, the
reference rounds Q * scale * log2(e) once to the I/O dtype, as the kernel does, and goes on in float64.  That rounding is 2^-11 of a score — 0.1
log2 units here, a tenth of every softmax weight — and belongs to the contract, not to the shell under test.
The shapes are the smallest at which the shell can go wrong: several trips per workgroup under both head -> XCD mappings, ragged and empty waves,
one trip, head dims below the body's, causal pair units with an odd number of blocks and with 32 blocks, KV-split parts, the redo.
"""
import ctypes
import functools

import pytest
import torch

from conftest import FLOOR, LSE_TOL, LSE_TOL_P16_BF16, LSE_TRUTH_TOL, RTOL
from rocwmma_fattn import _fa2_lib

pytestmark = pytest.mark.gpu

TORCH_DT = {0: torch.float16, 1: torch.bfloat16}
LOG2E = 1.4426950408889634
PAD_ROWS, PAD_COLS = 3, 8


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run the CPU suite with -m 'not gpu'"
    return torch.device("cuda", 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _truth(q, k, v, causal, group=1, prescale=False):
    """Dense float64 attention, a head at a time: (O [B, H, Nq, D] f64, LSE in log2 units [B, H, Nq] f64).  q, k, v: [B, H(kv), N, D] views.
    prescale: Q * scale * log2(e) rounded once to the I/O dtype first (FA2_CONTRACT_PRESCALE_Q)."""
    B, H, Nq, D = q.shape
    Nkv = k.shape[2]
    o = torch.empty((B, H, Nq, v.shape[3]), dtype=torch.float64, device=q.device)
    lse = torch.empty((B, H, Nq), dtype=torch.float64, device=q.device)
    keep = torch.ones(Nq, Nkv, dtype=torch.bool, device=q.device).tril() if causal else None
    for b in range(B):
        for h in range(H):
            if prescale:
                s = ((q[b, h].double() * (D ** -0.5 * LOG2E)).to(q.dtype).double() @ k[b, h // group].double().T) / LOG2E
            else:
                s = (q[b, h].double() @ k[b, h // group].double().T) * D ** -0.5
            if causal:
                s = s.masked_fill(~keep, float("-inf"))
            lse[b, h] = torch.logsumexp(s, -1) * LOG2E
            o[b, h] = torch.softmax(s, -1) @ v[b, h // group].double()
    return o, lse


@functools.lru_cache(maxsize=4)
def _case(B, H, N, D, dt, causal, seed, bnhd=False, hkv=None):
    """Seeded inputs with their float64 reference, computed once per shape and shared (never modified).  The tensors are 128 (64) columns wide
    whatever D is: a head dim below the body's is a column slice, so every row pitch stays a multiple of 64 bytes."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    W = 128 if D > 64 else 64
    Hk = hkv or H
    mk = lambda h: torch.randn((B, N, h, W) if bnhd else (B, h, N, W), generator=g).to(TORCH_DT[dt]).to(_dev())  # noqa: E731
    q, k, v = mk(H), mk(Hk), mk(Hk)
    if bnhd:
        q, k, v = (t.transpose(1, 2) for t in (q, k, v))
    q, k, v = q[..., :D], k[..., :D], v[..., :D]
    o_true, lse_true = _truth(q, k, v, causal, H // Hk)
    return q, k, v, o_true, lse_true


def _asm_everywhere():
    """Option `rows` = 256 pins the 256-row hand-scheduled kernels (no 128-row workgroups for a partly filled round, no minimum sweep length) and
    option `asm` bit 4 sends every head-dim-64 launch to them: the planner's speed thresholds aside, the shapes below are served by the
    hand-scheduled kernels, whose shell is what these tests are about."""
    return _fa2_lib.options(rows=256, asm=_fa2_lib.load(build_if_missing=False).fa2_get_option(b"asm") | 16)


def _lse_tol(plan_contract, dt):
    if plan_contract & _fa2_lib.FA2_CONTRACT_PRESCALE_Q:
        return LSE_TRUTH_TOL[dt]
    if dt == 1 and plan_contract & _fa2_lib.FA2_CONTRACT_LSUM_P16:
        return LSE_TOL_P16_BF16
    return LSE_TOL


def _run(q, k, v, causal, Nq=None, ws=False, hkv=None, bnhd_o=False):
    """One forward through the C-ABI into sentinel-padded buffers.  Returns (o view, lse view, o buffer, lse buffer, plan)."""
    lib = _fa2_lib.load(build_if_missing=False)
    B, H, N, D = q.shape
    Nq = N if Nq is None else Nq
    Nkv = k.shape[2]
    dt = 0 if q.dtype == torch.float16 else 1
    q = q[:, :, :Nq]
    W = 128 if D > 64 else 64
    if bnhd_o:
        obuf = torch.full((B, Nq + PAD_ROWS, H, W + PAD_COLS), float("nan"), dtype=q.dtype, device=q.device).transpose(1, 2)
    else:
        obuf = torch.full((B, H, Nq + PAD_ROWS, W + PAD_COLS), float("nan"), dtype=q.dtype, device=q.device)
    lbuf = torch.full((B, H, Nq + PAD_ROWS), float("nan"), dtype=torch.float32, device=q.device)
    o, lse = obuf[:, :, :Nq, :D], lbuf[:, :, :Nq]
    s3 = lambda t: _fa2_lib.strides3(t.stride(0), t.stride(1), t.stride(2))  # noqa: E731
    s2 = _fa2_lib.strides2(lse.stride(0), lse.stride(1))
    ptrs = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr())
    strides = (s3(q), s3(k), s3(v), s3(o), s2)
    need = lib.fa2_fwd_workspace_bytes(dt, B, H, Nq, Nkv, D, int(causal)) if ws else 0
    w = torch.empty(max(need, 16), dtype=torch.uint8, device=q.device)
    wp = w.data_ptr() if need else None
    if hkv is not None:
        plan = _fa2_lib.gqa_plan(q, k, causal, workspace_bytes=need)
        rc = lib.fa2_fwd_gqa(dt, *ptrs, B, H, hkv, Nq, Nkv, D, *strides, float(D ** -0.5), int(causal), wp, need, _stream())
    else:
        plan = _fa2_lib.fwd_plan(q, k, causal, workspace_bytes=need)
        rc = lib.fa2_fwd_ws(dt, *ptrs, B, H, Nq, Nkv, D, *strides, float(D ** -0.5), int(causal), wp, need, _stream())
    _fa2_lib.check(rc)
    torch.cuda.synchronize()
    return o, lse, obuf, lbuf, plan


def _check(res, o_true, lse_true, dt, Nq, D, expect_asm=True):
    o, lse, obuf, lbuf, plan = res
    # nothing outside rows < Nq, columns < D was written
    outside = torch.ones(obuf.shape, dtype=torch.bool, device=obuf.device)
    outside[:, :, :Nq, :D] = False
    assert torch.isnan(obuf[outside]).all(), "a store outside the O tile: %d elements" % int((~torch.isnan(obuf[outside])).sum())
    assert torch.isnan(lbuf[:, :, Nq:]).all(), "a store past the last LSE row"
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    o_ref, l_ref = o_true[:, :, :Nq, :D], lse_true[:, :, :Nq]
    err = (o.double() - o_ref).abs()
    bad = err > FLOOR[dt] + RTOL[dt] * o_ref.abs()
    assert not bad.any(), "O: %d elements beyond tolerance, max |diff| %.3g" % (int(bad.sum()), float(err.max()))
    lerr = (lse.double() - l_ref).abs()
    assert float(lerr.max()) <= _lse_tol(plan.contract, dt), "LSE: max |diff| %.3g (tol %.3g)" % (float(lerr.max()), _lse_tol(plan.contract, dt))
    if expect_asm:          # the case is about the hand-scheduled kernel's shell: it must have been that kernel
        assert plan.kernel == _fa2_lib.FA2_KERNEL_ASM, plan.as_dict()


# ---------------------------------------------------------------- several trips per workgroup, non-causal

@pytest.mark.parametrize("cut", [0, 37, 200])
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("H", [40, 33])
def test_several_trips_per_workgroup(H, dt, cut):
    """B1 N2048 D128: H40 is 320 items under the heads-in-eights mapping, H33 264 items under the other; Nq = 2048 - 37 leaves a ragged last block,
    Nq = 2048 - 200 waves whose rows all lie past Nq."""
    q, k, v, o_true, lse_true = _case(1, H, 2048, 128, dt, False, 1000 + H)
    Nq = 2048 - cut
    _check(_run(q, k, v, False, Nq=Nq), o_true, lse_true, dt, Nq, 128)


@pytest.mark.parametrize("N,seed,asm", [(512, 1100, False), (4096, 1400, True)])
def test_one_trip_persistent_matches_one_item_per_workgroup(N, seed, asm):
    """B1 H8: every workgroup makes one trip; persist = 0 (a grid of items) and persist = 1 bit-identical.  N512 (16 items) is served by a
    compiler-scheduled kernel — the planner keeps so short a sweep off the hand-scheduled one, and the call must not care about `persist`;
    N4096 (128 items on 256 CUs) is the same thing on the kernel under test."""
    q, k, v, o_true, lse_true = _case(1, 8, N, 128, 0, False, seed)
    res1 = _run(q, k, v, False)
    with _fa2_lib.options(persist=0):
        res0 = _run(q, k, v, False)
    _check(res1, o_true, lse_true, 0, N, 128, expect_asm=asm)
    _check(res0, o_true, lse_true, 0, N, 128, expect_asm=asm)
    assert torch.equal(res0[0], res1[0]) and torch.equal(res0[1], res1[1])


@pytest.mark.parametrize("D", [120, 88, 64, 56])
def test_head_dims_below_the_body(D):
    """The 16 x 16 bodies with a trimmed head dim, H40 with a ragged Nq: the stores are predicated by column too."""
    q, k, v, o_true, lse_true = _case(1, 40, 2048, D, 0, False, 1200 + D)
    Nq = 2048 - 37
    with _asm_everywhere():
        res = _run(q, k, v, False, Nq=Nq)
    _check(res, o_true, lse_true, 0, Nq, D)


# ---------------------------------------------------------------- causal pair units

@pytest.mark.parametrize("B,H,N", [(2, 43, 1280), (1, 1, 8192)])
def test_causal_pair_units(B, H, N):
    """Persistent pairs (nqblk - 1 - i, i): an odd number of blocks (86 x 3 units, the middle block alone in its unit) and a head of 32 blocks."""
    q, k, v, o_true, lse_true = _case(B, H, N, 128, 0, True, 1300 + H)
    with _asm_everywhere():
        res = _run(q, k, v, True)
    _check(res, o_true, lse_true, 0, N, 128)


# ---------------------------------------------------------------- KV-split parts inside the persistent workgroups

@pytest.mark.parametrize("H,N", [(8, 4096), (40, 2048)])
def test_kv_split_parts(H, N):
    """Through the workspace call: a grid of parts only (B1 H8 N4096: 128 items on 256 CUs), and a partly filled last round beside whole items."""
    q, k, v, o_true, lse_true = _case(1, H, N, 128, 0, False, 1000 + H if N == 2048 else 1400)
    res = _run(q, k, v, False, ws=True)
    assert res[4].nsplit > 1 and res[4].split_items > 0, res[4].as_dict()
    _check(res, o_true, lse_true, 0, N, 128)


# ---------------------------------------------------------------- the redo and the sticky bit

@functools.lru_cache(maxsize=1)
def _large_logit_case():
    """The recipe of test_sum_check_bodies_repair_in_place_and_redo_in_safe_mode (kind "redo") at B1 H40 N2048: inputs three times as large, planted
    rows, and a growth of exactly 126.5 octaves over a row's tile-0 maximum in every fifth head."""
    B, H, N, D = 1, 40, 2048, 128
    g = torch.Generator(device="cpu").manual_seed(1500)
    q, k, v = (torch.randn((B, H, N, D), generator=g) for _ in range(3))
    q, k = q * 3, k * 3
    k[:, :, 200] = q[:, :, 5] * 4
    k[:, :, 70] = q[:, :, 40] * 2
    k[:, :, 600] = q[:, :, 800] * 4
    q, k, v = (t.to(torch.float16) for t in (q, k, v))
    c = D ** -0.5 * LOG2E
    for h in range(0, H, 5):
        for row, kv in ((300, 520), (77, 333)):
            qr = q[0, h, row].double()
            ref = float((k[0, h, :64].double() @ qr).max()) * c
            k[0, h, kv] = (qr * ((ref + 126.5) / (float((qr ** 2).sum()) * c))).to(torch.float16)
    q, k, v = (t.to(_dev()) for t in (q, k, v))
    prescale = bool(_fa2_lib.fwd_plan(q, k, False).contract & _fa2_lib.FA2_CONTRACT_PRESCALE_Q)
    return (q, k, v) + _truth(q, k, v, False, prescale=prescale)


@pytest.mark.parametrize("lm", [1, 0])
def test_redo_and_sticky_bit(lm):
    """Items that are run again in safe mode (`continue` behind the flag read) and items that start in safe mode after them: with the default bodies
    (row sums on the matrix pipe) and with option `asm` bit 9 clear (the sum-check bodies)."""
    q, k, v, o_true, lse_true = _large_logit_case()
    lib = _fa2_lib.load(build_if_missing=False)
    full = lib.fa2_get_option(b"asm")
    with _fa2_lib.options(asm=full if lm else full & ~512):
        res = _run(q, k, v, False)
        res2 = _run(q, k, v, False)
    _check(res, o_true, lse_true, 0, 2048, 128)
    assert torch.equal(res[0], res2[0]) and torch.equal(res[1], res2[1])


# ---------------------------------------------------------------- layouts

def test_bnhd_strides():
    q, k, v, o_true, lse_true = _case(1, 40, 2048, 128, 0, False, 1600, bnhd=True)
    _check(_run(q, k, v, False, bnhd_o=True), o_true, lse_true, 0, 2048, 128)


def test_grouped_query_heads():
    q, k, v, o_true, lse_true = _case(1, 40, 2048, 128, 0, False, 1700, hkv=10)
    _check(_run(q, k, v, False, hkv=10), o_true, lse_true, 0, 2048, 128)
