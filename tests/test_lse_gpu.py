"""GPU tests of flash_attention(..., return_lse=True) / flash_attention_varlen(..., return_lse=True) and of the backward entry points that take a gradient
for the LSE (fa2_bwd_lse, fa2_bwd_window_lse, fa2_bwd_varlen_lse).

Reference: dense float64 autograd written in tests/lse_refs.py (truth64), loss = (out * dO).sum() + (lse_live * u).sum() with the natural-log LSE;
beside it the same-contract f32 emulation (emulate).  Bars: the project's rule, max|got - true| <= max(2 * err_emu, tol * max(1, max|true|)) with
FLOOR / GRAD_TOL of conftest.py; the LSE in log2 units, max(LSE_TOL, 2 * err_emu).  Not vacuous: the float64 dQ and dK with the u term differ from
those without it by at least 5 bars (asserted; dV does not depend on dlse).
Inputs: q, k, v = 2 * N(0, 1); dO, u = N(0, 1).  B 2, H 4 (Hkv 2 where grouped), Nq 200 x Nkv 333 unless stated."""
import ctypes

import pytest
import torch

import lse_refs as R
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention, flash_attention_varlen, flash_attn_wmma

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]
B, H, NQ, NKV = 2, 4, 200, 333
LN2 = R.LN2


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("these tests need a ROCm device")
    return torch.device("cuda")


def make(dt, hkv, D, nq=NQ, nkv=NKV, b=B, h=H, seed=0):
    g = torch.Generator().manual_seed(7000 + seed)
    mk = lambda shape, mul: (torch.randn(shape, generator=g) * mul).to(dt)      # noqa: E731
    return mk((b, h, nq, D), 2.0), mk((b, hkv, nkv, D), 2.0), mk((b, hkv, nkv, D), 2.0), mk((b, h, nq, D), 1.0), torch.randn((b, h, nq), generator=g)


def slopes_of(h):
    return torch.tensor([2.0 ** (-8.0 * (i + 1) / h) for i in range(h)], dtype=torch.float32)


# route name -> keyword arguments of the case (run_dense)
ROUTES = {
    "plain_d64": dict(D=64),
    "plain_d128": dict(D=128),
    "causal": dict(D=64, causal=True),
    "grouped": dict(D=64, hkv=2),
    "bool_mask": dict(D=64, mask="bool"),
    "float_mask": dict(D=64, mask="float"),
    "window": dict(D=64, window=(63, 0), q_offset=5),
    "dropout": dict(D=64, dropout_p=0.2),
    "softcap_alibi": dict(D=64, softcap=30.0, alibi=True),
    "bnhd": dict(D=64, bnhd=True, causal=True),
    "d72": dict(D=72),
    # (the seed of this case was chosen on the float64 references alone, no kernel involved: at D = 320 in bf16 the bar — 1.6e-2 of the largest gradient —
    #  is wide and these inputs move dQ / dK by 2.3 .. 7.2 bars depending on the draw, seeds 0 .. 9; seed 4 gives 6.1 / 7.2)
    "d320": dict(D=320, seed=4),
}


def run_dense(dt, D, hkv=H, causal=False, mask=None, window=None, q_offset=0, dropout_p=0.0, softcap=0.0, alibi=False, bnhd=False, nq=NQ, nkv=NKV,
              b=B, h=H, seed=0, check_identity=True, lse_only=False):
    dev = _dev()
    hkv = min(hkv, h)
    q, k, v, do, u = (t.to(dev) for t in make(dt, hkv, D, nq, nkv, b, h, seed))
    scale = D ** -0.5
    left, right, off = _fa2_lib.parse_window(window if window is not None else (-1, -1), q_offset)
    allow = R.ff.band(nq, nkv, left, right, off, causal, dev)
    g = torch.Generator().manual_seed(99)
    m = bias = None
    if mask == "bool":
        m = torch.rand((b, 1, nq, nkv), generator=g) < 0.7
        m[:, :, 3] = False                                          # a fully masked row: lse = -inf
        m = m.to(dev)
    elif mask == "float":
        m = torch.randn((1, h, nq, nkv), generator=g).to(dev)
    sl = slopes_of(h).to(dev) if alibi else None
    seed_d = 1234
    kw = dict(causal=causal, BNHD_fmt=bnhd, window=window, q_offset=q_offset, softcap=softcap, alibi_slopes=sl, mask=m, dropout_p=dropout_p,
              dropout_seed=seed_d if dropout_p else None)

    def put(t):
        return (t.transpose(1, 2).contiguous() if bnhd else t.clone()).requires_grad_(True)
    unp = (lambda t: t.transpose(1, 2)) if bnhd else (lambda t: t)
    qd, kd, vd = put(q), put(k), put(v)
    out, lse = flash_attention(qd, kd, vd, return_lse=True, **kw)
    assert lse.shape == (b, h, nq) and lse.dtype == torch.float32 and out.shape == qd.shape
    if check_identity:      # the same call without return_lse already scales the f32 scores when its inputs need a gradient: out must not change by one bit
        q2, k2, v2 = put(q), put(k), put(v)
        assert torch.equal(flash_attention(q2, k2, v2, **kw).detach(), out.detach()), "return_lse=True changed out"
    with torch.no_grad():   # ... and the call under no_grad returns the same pair (it is flagged FA2_FLAG_EXACT_SCALE as well)
        o_ng, lse_ng = flash_attention(qd.detach(), kd.detach(), vd.detach(), return_lse=True, **kw)
    assert torch.equal(o_ng, out.detach()) and torch.equal(lse_ng, lse.detach())
    live = ~torch.isinf(lse.detach())
    if lse_only:
        lse.masked_fill(~live, 0.0).sum().backward()
        do, u = torch.zeros_like(do), torch.ones_like(u)
    else:
        ((unp(out).float() * do.float()).sum() + (lse * u).masked_fill(~live, 0.0).sum()).backward()
    got_all = dict(O=unp(out).detach(), lse=lse.detach() / LN2, dQ=unp(qd.grad), dK=unp(kd.grad), dV=unp(vd.grad))
    tag0 = "%s H%d/%d %dx%d D%d causal=%d mask=%s win=%s off=%d p=%g cap=%g alibi=%d bnhd=%d" % (
        str(dt)[6:], h, hkv, nq, nkv, D, causal, mask, window, q_offset, dropout_p, softcap, alibi, bnhd)
    whole = ([], [], [])
    for bi in range(b):
        grp = h // hkv
        ke, ve = k[bi].repeat_interleave(grp, 0), v[bi].repeat_interleave(grp, 0)
        al, bs = allow, None
        if mask == "bool":
            al = allow & m[bi]
        elif mask == "float":
            bs = m[0]
        keep, rs = None, 1.0
        if dropout_p:
            keep = R.ff.keep_unit(seed_d, dropout_p, h, bi, nq, nkv).to(dev)
            rs = 1.0 / (1.0 - R.ff.p_eff(dropout_p))
        ref_kw = dict(softcap=softcap, slopes=sl, off=off, bias=bs, keep=keep, rs=rs)
        true = R.truth64(q[bi], ke, ve, do[bi], u[bi], al, scale, **ref_kw)
        emu = R.emulate(q[bi], ke, ve, do[bi], u[bi], al, scale, dt, **ref_kw)
        plain = R.truth64(q[bi], ke, ve, do[bi], None, al, scale, **ref_kw)
        for d in (true, emu, plain):
            d["dK"], d["dV"] = R.fold(d["dK"], hkv), R.fold(d["dV"], hkv)
        bars = R.bars_of(true, emu, dt)
        got = {n: t[bi] for n, t in got_all.items()}
        tag = "%s b%d" % (tag0, bi)
        R.check(tag, got, true, bars)
        for acc, d in zip(whole, (true, emu, plain)):
            acc.append(d)
        dead = torch.isinf(true["lse"])
        if dead.any():
            assert (got["O"][dead] == 0).all() and (got["dQ"][dead] == 0).all(), (tag, "rows that see no key: zeros")
    if not lse_only:        # non-vacuity over the whole call: one bar per output, as the rule states it
        true, emu, plain = ({n: torch.stack([d[n] for d in acc]) for n in R.NAMES} for acc in whole)
        R.check_not_vacuous(tag0, true, plain, R.bars_of(true, emu, dt))


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_out_lse_and_gradients_through_the_lse_on_every_route(route, dt):
    run_dense(dt, **ROUTES[route])


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_hand_scheduled_shape_runs_the_fallback_passes(dt):
    """D = 128, Nq = 256, non-causal: without a dlse both passes are the hand-scheduled ones (fa2_bwd_plan); with one the compiler-scheduled passes run."""
    a = _fa2_lib.BwdPlan()
    args = (R.code(dt), B, H, H, 256, 256, 128, None, None, None, None, None, 128 ** -0.5, 0, 0, None)
    _fa2_lib.check(_fa2_lib.load().fa2_bwd_lse_plan(*args, 0, ctypes.byref(a)))
    assert (a.dq_kernel, a.dkv_kernel) == (_fa2_lib.FA2_BWD_KERNEL_ASM, _fa2_lib.FA2_BWD_KERNEL_ASM)
    _fa2_lib.check(_fa2_lib.load().fa2_bwd_lse_plan(*args, 1, ctypes.byref(a)))
    assert (a.dq_kernel, a.dkv_kernel) == (_fa2_lib.FA2_BWD_KERNEL_HIP, _fa2_lib.FA2_BWD_KERNEL_HIP)
    run_dense(dt, 128, nq=256, nkv=256)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_short_dq_kernel_takes_dlse(dt):
    a = _fa2_lib.BwdPlan()
    _fa2_lib.check(_fa2_lib.load().fa2_bwd_lse_plan(R.code(dt), B, H, H, NQ, 77, 64, None, None, None, None, None, 0.125, 0, 0, None, 1, ctypes.byref(a)))
    assert a.dq_kernel == _fa2_lib.FA2_BWD_KERNEL_SHORT
    run_dense(dt, 64, nkv=77)


def test_kv_split_parts_take_dlse():
    """B1 H2 N4096 D64 non-causal bf16 through the operator: the dQ pass runs as KV-split parts (each part forms delta - dlse, part 0 stores it)."""
    dt_code = 1
    assert _fa2_lib.load().fa2_bwd_workspace_bytes(dt_code, 1, 2, 4096, 4096, 64, 0) > 0, "this shape no longer splits: the test must exercise the parts"
    run_dense(BF16, 64, nq=4096, nkv=4096, b=1, h=2, hkv=2)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_dlse_only(dt):
    """lse.sum().backward() with out unused: the node's backward receives dO = None."""
    run_dense(dt, 64, lse_only=True, check_identity=False)
    run_dense(dt, 64, window=(63, 0), q_offset=5, lse_only=True, check_identity=False)


# ---------------------------------------------------------------------------------------------------------------- packed
Q_LENS, K_LENS = (0, 37, 200, 96), (5, 64, 333, 40)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("bottom_right", [False, True], ids=["top_left", "bottom_right"])
def test_packed_call_returns_a_differentiable_lse(bottom_right, dt):
    dev = _dev()
    D, hkv = 64, 2
    g = torch.Generator().manual_seed(7100)
    tq, tk = sum(Q_LENS), sum(K_LENS)
    mk = lambda shape, mul: (torch.randn(shape, generator=g) * mul).to(dt).to(dev)      # noqa: E731
    q, k, v, do = mk((tq, H, D), 2.0), mk((tk, hkv, D), 2.0), mk((tk, hkv, D), 2.0), mk((tq, H, D), 1.0)
    u = torch.randn((H, tq), generator=g).to(dev)
    cu = lambda lens: torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=dev)      # noqa: E731
    cq, ck = cu(Q_LENS), cu(K_LENS)
    kw = dict(max_seqlen_q=max(Q_LENS), max_seqlen_k=max(K_LENS), causal=True, bottom_right=bottom_right)
    qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
    out, lse = flash_attention_varlen(qd, kd, vd, cq, ck, return_lse=True, **kw)
    assert lse.shape == (H, tq) and lse.dtype == torch.float32
    q2, k2, v2 = (t.clone().requires_grad_(True) for t in (q, k, v))
    assert torch.equal(flash_attention_varlen(q2, k2, v2, cq, ck, **kw).detach(), out.detach()), "return_lse=True changed out"
    live = ~torch.isinf(lse.detach())
    ((out.float() * do.float()).sum() + (lse * u).masked_fill(~live, 0.0).sum()).backward()
    for s, (nq, nk) in enumerate(zip(Q_LENS, K_LENS)):
        if nq == 0:
            continue
        q0, k0 = int(cq[s]), int(ck[s])
        off = nk - nq if bottom_right else 0
        pos = torch.arange(nq, device=dev).unsqueeze(1) + off
        allow = torch.arange(nk, device=dev).unsqueeze(0) <= pos
        sl = lambda t, a, n: t[a:a + n].transpose(0, 1)      # noqa: E731
        qs, ks, vs, gs = sl(q, q0, nq), sl(k, k0, nk).repeat_interleave(H // hkv, 0), sl(v, k0, nk).repeat_interleave(H // hkv, 0), sl(do, q0, nq)
        us = u[:, q0:q0 + nq]
        true = R.truth64(qs, ks, vs, gs, us, allow, D ** -0.5)
        emu = R.emulate(qs, ks, vs, gs, us, allow, D ** -0.5, dt)
        plain = R.truth64(qs, ks, vs, gs, None, allow, D ** -0.5)
        for d in (true, emu, plain):
            d["dK"], d["dV"] = R.fold(d["dK"], hkv), R.fold(d["dV"], hkv)
        bars = R.bars_of(true, emu, dt)
        got = dict(O=sl(out.detach(), q0, nq), lse=lse.detach()[:, q0:q0 + nq] / LN2, dQ=sl(qd.grad, q0, nq), dK=sl(kd.grad, k0, nk), dV=sl(vd.grad, k0, nk))
        tag = "%s packed seq %d (%d x %d) bottom_right=%d" % (str(dt)[6:], s, nq, nk, bottom_right)
        R.check(tag, got, true, bars)
        if nq >= 37 and nk >= 40:
            R.check_not_vacuous(tag, true, plain, bars)
        dead = torch.isinf(true["lse"])
        if dead.any():
            assert (got["O"][dead] == 0).all() and (got["dQ"][dead] == 0).all(), (tag, "rows that see no key: zeros")


# ---------------------------------------------------------------------------------------------------------------- the C-ABI directly
def _s3(t):
    return _fa2_lib.strides3(t.stride(0), t.stride(1), t.stride(2))


def _saved(dt, D, window, nq=NQ, nkv=NKV, seed=3):
    """The tensors a backward call takes, from the extension's own forward: (q, k, v, o, do, L) contiguous [B, H, N, D], L [B, H, Nq_padded]."""
    dev = _dev()
    q, k, v, do, u = (t.to(dev) for t in make(dt, H, D, nq, nkv, seed=seed))
    flags = _fa2_lib.FA2_FLAG_EXACT_SCALE
    ret = flash_attn_wmma.forward_py(q, k, v, 64, 128, flags, D ** -0.5, False, window=window)
    torch.cuda.synchronize()
    return ret[1], ret[2], ret[3], ret[4], do, ret[5], u


def _raw_bwd(fn_name, t, D, tail, nq=NQ, nkv=NKV):
    """One backward entry point on fresh outputs -> (dq, dk, dv, delta)."""
    q, k, v, o, do, L, _ = t
    dq, dk, dv = torch.full_like(q, 7.0), torch.full_like(k, 7.0), torch.full_like(v, 7.0)
    delta = torch.full_like(L, 7.0)
    lib = _fa2_lib.load()
    rc = getattr(lib, fn_name)(R.code(q.dtype), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), L.data_ptr(), dq.data_ptr(),
                               dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), B, H, nq, nkv, D, _s3(q), _s3(k), _s3(v), _s3(o), _s3(do), _s3(dq), _s3(dk),
                               _s3(dv), _fa2_lib.strides2(L.stride(0), L.stride(1)), D ** -0.5, 0, *tail)
    _fa2_lib.check(rc)
    torch.cuda.synchronize()
    return dq, dk, dv, delta[:, :, :nq]


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_null_dlse_is_the_existing_call_bit_for_bit(D, dt):
    stream = torch.cuda.current_stream().cuda_stream
    t = _saved(dt, D, (-1, -1, 0), nq=256, nkv=256)
    old = _raw_bwd("fa2_bwd_ws", t, D, (None, 0, stream), 256, 256)
    new = _raw_bwd("fa2_bwd_lse", t, D, (None, 0, None, None, 0, stream, None, None), 256, 256)
    assert all(torch.equal(a, b) for a, b in zip(old, new)), "fa2_bwd_lse(dlse = NULL) differs from fa2_bwd_ws"
    for win in ((-1, -1, 0), (63, 0, 5)):
        t = _saved(dt, D, win)
        old = _raw_bwd("fa2_bwd_window", t, D, (*win, stream))
        new = _raw_bwd("fa2_bwd_window_lse", t, D, (*win, stream, 0.0, 0, 0.0, None, 0, None, None))
        assert all(torch.equal(a, b) for a, b in zip(old, new)), ("fa2_bwd_window_lse(dlse = NULL) differs from fa2_bwd_window", win)
        old = _raw_bwd("fa2_bwd_dropout", t, D, (*win, stream, 0.25, 77))
        new = _raw_bwd("fa2_bwd_window_lse", t, D, (*win, stream, 0.25, 77, 0.0, None, 0, None, None))
        assert all(torch.equal(a, b) for a, b in zip(old, new)), ("fa2_bwd_window_lse(dropout, dlse = NULL) differs from fa2_bwd_dropout", win)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_null_dlse_packed_is_the_existing_call_bit_for_bit(dt):
    dev = _dev()
    D = 64
    g = torch.Generator().manual_seed(7200)
    lens = (37, 200, 96)
    tot = sum(lens)
    mk = lambda mul: (torch.randn((tot, H, D), generator=g) * mul).to(dt).to(dev)      # noqa: E731
    q, k, v, do = mk(2.0), mk(2.0), mk(2.0), mk(1.0)
    cu = torch.tensor([0, 37, 237, 333], dtype=torch.int32, device=dev)
    lib = _fa2_lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    s2 = lambda t: _fa2_lib.strides2(t.stride(1), t.stride(0))      # noqa: E731
    for left, right in ((-1, -1), (63, 0)):
        ret = flash_attn_wmma.forward_varlen(q, k, v, cu, cu, 200, 200, _fa2_lib.FA2_FLAG_EXACT_SCALE, D ** -0.5, (left, right))
        o, L = ret[4], ret[5]
        res = []
        for name, tail in (("fa2_bwd_varlen", ()), ("fa2_bwd_varlen_lse", (0.0, 0, 0.0, None, 0, None, 0))):
            dq, dk, dv, delta = torch.full_like(q, 7.0), torch.full_like(q, 7.0), torch.full_like(q, 7.0), torch.full_like(L, 7.0)
            _fa2_lib.check(getattr(lib, name)(R.code(dt), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), L.data_ptr(), dq.data_ptr(),
                                              dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), 3, H, 200, 200, D, cu.data_ptr(), cu.data_ptr(), s2(q), s2(k), s2(v),
                                              s2(o), s2(do), s2(dq), s2(dk), s2(dv), L.stride(0), D ** -0.5, 0, left, right, stream, *tail))
            torch.cuda.synchronize()
            res.append((dq, dk, dv, delta))
        assert all(torch.equal(a, b) for a, b in zip(*res)), ("fa2_bwd_varlen_lse(dlse = NULL) differs from fa2_bwd_varlen", left, right)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128, 320])
def test_dead_rows_ignore_their_dlse_even_a_nan(D, dt):
    """Nq 200 x Nkv 120 under window (15, 0): rows 135 .. 199 see no key.  NaN as dlse on exactly those rows: every gradient finite, dQ of those rows zero,
    and the live rows' gradients those of the same call with zeros there."""
    nq, nkv, win = 200, 120, (15, 0, 0)           # row i sees the keys [i - 15, i] below 120: none from row 135 on
    t = _saved(dt, D, win, nq, nkv)
    L = t[5][:, :, :nq]
    dead = torch.isneginf(L)
    assert dead[:, :, 135:].all() and not dead[:, :, :135].any(), "the forward must write -inf for exactly the rows that see no key"
    stream = torch.cuda.current_stream().cuda_stream
    g = t[6] * LN2                                                     # log2 units
    res = []
    for fill in (float("nan"), 0.0):
        dl = g.masked_fill(dead, fill).contiguous()
        res.append(_raw_bwd("fa2_bwd_window_lse", t, D, (*win, stream, 0.0, 0, 0.0, None, 0, dl.data_ptr(), _fa2_lib.strides2(dl.stride(0), dl.stride(1))), nq, nkv))
    for a, b in zip(*res):
        assert torch.isfinite(a.float()).all()
        assert torch.equal(a, b)
    assert (res[0][0][:, :, 135:] == 0).all()
