"""GPU tests of the score modifiers (fa2_fwd_scoremod / fa2_bwd_scoremod and their packed twins; flash_attention(softcap=..., alibi_slopes=...)).

The reference is dense float64 autograd of the contract (include/fa2_gfx950.h), written here (truth64): x = q.k * scale, s = softcap * tanh(x / softcap),
s -= slope[b, h] * |pos - j|, then the band as -inf.  The oracle is not involved.  Beside it stands a same-contract torch emulation (emulate): f32 scores,
transform and sums; P rounded to the I/O dtype; dS * (1 - t^2) rounded to the I/O dtype; outputs rounded once.
Bars: the project's rule, tools/fuzz_features.py: error_and_bar with FLOOR / GRAD_TOL of conftest.py,
    max|got - true| <= max(2 * err_emu, tol * max(1, max|true|));
the LSE (log2 units): max(LSE_TOL, 2 * the emulation's LSE error).
Not vacuous: in every parity case the float64 result WITH the feature differs from the float64 result WITHOUT it by at least 5 x that output's bar
(asserted: a kernel that ignored the keyword would fail every check by a wide margin).
Inputs: q, k, v = 2 * N(0, 1), dO = N(0, 1); Nq 200 x Nkv 333 (a ragged tail, two workgroups at rows = 128, masked and plain tiles per wave); B 2, H 4."""
import importlib.util
import math
import os

import pytest
import torch

from conftest import FLOOR, GRAD_TOL, LSE_TOL
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention, flash_attention_varlen, flash_attn_wmma

pytestmark = pytest.mark.gpu

LN2 = math.log(2.0)
F16, BF16 = torch.float16, torch.bfloat16
B, H, NQ, NKV = 2, 4, 200, 333
NAMES = ("O", "lse", "dQ", "dK", "dV")

_spec = importlib.util.spec_from_file_location("_fuzz_features", os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "tools", "fuzz_features.py"))
_ff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ff)


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("these tests need a ROCm device")
    return torch.device("cuda")


def _code(dt):
    return 0 if dt == F16 else 1


def alibi_slopes(h, mul=1.0):
    return torch.tensor([mul * 2.0 ** (-8.0 * (i + 1) / h) for i in range(h)], dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------- the references (any device)
def _dist(nq, nk, off, device):
    return (torch.arange(nq, device=device).unsqueeze(1) + off - torch.arange(nk, device=device).unsqueeze(0)).abs()


def _softmax_parts(S, band):
    S = S.masked_fill(~band, float("-inf"))
    m = S.max(-1, keepdim=True).values.detach()
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    E = torch.exp(S - m)
    l = E.sum(-1, keepdim=True)
    l1 = torch.where(l > 0, l, torch.ones_like(l))
    lse = ((m + torch.log(l)) / LN2).squeeze(-1).detach()
    lse[..., ~band.any(-1)] = float("-inf")
    return E, l1, lse


def truth64(q, k, v, do, band, scale, softcap, slopes, off):
    """float64 autograd of the contract for [H, Nq, D] q and [H, Nkv, D] k / v (grouped k / v already expanded); slopes: [H] or None.
    -> dict O, lse (log2 units), dQ, dK, dV."""
    q, k, v = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    S = (q @ k.transpose(-1, -2)) * scale
    if softcap > 0:
        S = softcap * torch.tanh(S / softcap)
    if slopes is not None:
        S = S - slopes.double().to(q.device)[:, None, None] * _dist(q.shape[1], k.shape[1], off, q.device)
    E, l1, lse = _softmax_parts(S, band)
    O = (E / l1) @ v
    O.backward(do.double())
    return dict(O=O.detach(), lse=lse, dQ=q.grad, dK=k.grad, dV=v.grad)


def emulate(q, k, v, do, band, scale, softcap, slopes, off, dt):
    """The kernels' contract in torch: f32 scores, transform and sums; P rounded to the I/O dtype; dS (1 - t^2) rounded to the I/O dtype; outputs rounded once."""
    qf, kf, vf, gf = q.float(), k.float(), v.float(), do.float()
    S = (qf @ kf.transpose(-1, -2)) * scale
    fac = torch.ones_like(S)
    if softcap > 0:
        t = torch.tanh(S / softcap)
        S, fac = softcap * t, 1.0 - t * t
    if slopes is not None:
        S = S - slopes.float().to(q.device)[:, None, None] * _dist(q.shape[1], k.shape[1], off, q.device).float()
    E, l1, lse = _softmax_parts(S, band)
    O = ((E.to(dt).float() @ vf) / l1).to(dt)
    Pn = E / l1
    dV = (Pn.to(dt).float().transpose(-1, -2) @ gf).to(dt)
    dP = gf @ vf.transpose(-1, -2)
    delta = (gf * O.float()).sum(-1, keepdim=True)
    dX = (Pn * (dP - delta) * fac).to(dt).float()
    dQ = ((dX @ kf) * scale).to(dt)
    dK = ((dX.transpose(-1, -2) @ qf) * scale).to(dt)
    return dict(O=O.double(), lse=lse.double(), dQ=dQ.double(), dK=dK.double(), dV=dV.double())


def fold(t, hkv):
    return t.unflatten(0, (hkv, t.shape[0] // hkv)).sum(1)


def bars_of(true, emu, dt):
    """name -> (bar, err_emu)."""
    code, out = _code(dt), {}
    for n in NAMES:
        if n == "lse":
            live = ~torch.isinf(true["lse"])
            e = (emu["lse"][live] - true["lse"][live]).abs().max().item() if live.any() else 0.0
            out[n] = (max(LSE_TOL, 2 * e), e)
        else:
            _, e, bar = _ff.error_and_bar(emu[n], true[n], emu[n], FLOOR[code] if n == "O" else GRAD_TOL[code])
            out[n] = (bar, e)
    return out


def unit_refs(q, k, v, do, band, scale, softcap, slopes, off, dt, hkv):
    """Truth with the feature, truth without it, the emulation and the bars of one batch / sequence; dK / dV folded to the hkv K / V heads."""
    g = q.shape[0] // hkv
    ke, ve = k.repeat_interleave(g, 0), v.repeat_interleave(g, 0)
    true = truth64(q, ke, ve, do, band, scale, softcap, slopes, off)
    plain = truth64(q, ke, ve, do, band, scale, 0.0, None, off)
    emu = emulate(q, ke, ve, do, band, scale, softcap, slopes, off, dt)
    for d in (true, plain, emu):
        d["dK"], d["dV"] = fold(d["dK"], hkv), fold(d["dV"], hkv)
    return true, plain, emu, bars_of(true, emu, dt)


def margin(true, plain, bars, n):
    """(float64 with the feature - float64 without) / the output's bar."""
    a, b = true[n], plain[n]
    if n == "lse":
        live = ~torch.isinf(a)
        a, b = a[live], b[live]
    return ((a - b).abs().max().item() if a.numel() else 0.0) / bars[n][0]


def check_unit(tag, got, true, plain, emu, bars, vacuous_ok=False):
    for n in NAMES:
        bar, e_emu = bars[n]
        x, t = got[n].double(), true[n]
        if n == "lse":
            dead = torch.isinf(t)
            assert torch.isneginf(got[n][dead]).all(), (tag, "rows that see no key: lse = -inf")
            x, t = x[~dead], t[~dead]
        assert torch.isfinite(x).all(), (tag, n, "non-finite")
        err = (x - t).abs().max().item() if x.numel() else 0.0
        mg = margin(true, plain, bars, n)
        print("%s %s: err %.3g, emulation %.3g, bar %.3g, feature margin %.0fx" % (tag, n, err, e_emu, bar, mg))
        assert err <= bar, (tag, n, err, bar)
        if not vacuous_ok:
            assert mg >= 5.0, (tag, n, "the feature moves this output by only %.1f bars: louder inputs needed" % mg)
    dead = torch.isinf(true["lse"])
    if dead.any():
        assert (got["O"][dead] == 0).all() and (got["dQ"][dead] == 0).all(), (tag, "rows that see no key: zeros")


def make_inputs(dt, hkv, D, nq=NQ, nkv=NKV, b=B, seed=0, qk_mul=2.0):
    g = torch.Generator().manual_seed(4000 + seed)
    mk = lambda shape, mul: (torch.randn(shape, generator=g) * mul).to(dt)      # noqa: E731
    return mk((b, H, nq, D), qk_mul), mk((b, hkv, nkv, D), qk_mul), mk((b, hkv, nkv, D), 2.0), mk((b, H, nq, D), 1.0)


# ---------------------------------------------------------------------------------------------------------------- dense parity
def run_dense(dt, hkv, D, softcap=0.0, slopes=None, causal=False, window=None, q_offset=0, bnhd=False, rows=0, inputs=None, vacuous_ok=False, seed=0):
    dev = _dev()
    q, k, v, do = inputs if inputs is not None else make_inputs(dt, hkv, D, seed=seed)
    nq, nkv, scale = q.shape[2], k.shape[2], D ** -0.5
    left, right, off = _fa2_lib.parse_window(window if window is not None else (-1, -1), q_offset)
    band = _ff.band(nq, nkv, left, right, off, causal, dev)

    def put(t):
        t = t.to(dev)
        return (t.transpose(1, 2).contiguous() if bnhd else t).requires_grad_(True)
    qd, kd, vd = put(q), put(k), put(v)
    sl = None if slopes is None else slopes.to(dev)
    kw = dict(causal=causal, BNHD_fmt=bnhd, window=window, q_offset=q_offset, softcap=softcap, alibi_slopes=sl)
    with _fa2_lib.options(rows=rows):
        o = flash_attention(qd, kd, vd, **kw)
        o.backward(do.to(dev).transpose(1, 2).contiguous() if bnhd else do.to(dev))
        flags = (_fa2_lib.FA2_FLAG_CAUSAL if causal else 0) | _fa2_lib.FA2_FLAG_EXACT_SCALE
        ret = flash_attn_wmma.forward_py(qd.detach(), kd.detach(), vd.detach(), 32 if D > 384 else 64, 128, flags, scale, bnhd, window=(left, right, off), scoremod=(float(softcap), sl))
    assert torch.equal(ret[0], o.detach()), "the operator and the extension's forward differ"
    lse = ret[5][:, :, :nq]
    unp = (lambda t: t.transpose(1, 2)) if bnhd else (lambda t: t)
    O, dQ, dK, dV = (unp(t).detach() for t in (o, qd.grad, kd.grad, vd.grad))
    tag0 = "%s H%d/%d %dx%d D%d cap=%g alibi=%s causal=%d win=%s off=%d bnhd=%d rows=%d" % (
        str(dt)[6:], H, hkv, nq, nkv, D, softcap, None if slopes is None else tuple(slopes.shape), causal, window, q_offset, bnhd, rows)
    for b in range(q.shape[0]):
        sb = None if slopes is None else (slopes[b] if slopes.dim() == 2 else slopes)
        refs = unit_refs(q[b].to(dev), k[b].to(dev), v[b].to(dev), do[b].to(dev), band, scale, softcap, sb, off, dt, hkv)
        check_unit("%s b%d" % (tag0, b), dict(O=O[b], lse=lse[b], dQ=dQ[b], dK=dK[b], dV=dV[b]), *refs, vacuous_ok=vacuous_ok)


DIMS = [64, 128, 256]


@pytest.mark.parametrize("softcap", [1.0, 30.0])
@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("D", DIMS)
def test_softcap_alone(D, dt, softcap):
    run_dense(dt, 4 if softcap == 1.0 else 2, D, softcap=softcap)


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("nkv", [1, NKV])
def test_a_large_softcap_leaves_the_scores_alone(nkv, dt):
    """softcap = 1e4 over scores of a few units: s = x to 1e-7 relative, so every output — the LSE within LSE_TOL — is that of the uncapped call.  The
    reduced form of what tools/fuzz_lse.py's first runs flagged: the tanh of csrc/fa2_scoremod.h was 1 - 2 / (1 + e^2y) everywhere, a few 2^-24 off in
    ABSOLUTE terms, which softcap = 1e4 turned into 1e-3 in every score (LSE errors of 1.0e-3 .. 1.6e-3 log2 units; with one key the LSE is that score)."""
    run_dense(dt, 2, 64, softcap=1e4, inputs=make_inputs(dt, 2, 64, nq=64, nkv=nkv, seed=11), vacuous_ok=True)


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("D", DIMS)
def test_alibi_alone_keys_on_both_sides(D, dt):
    run_dense(dt, 2 if dt == F16 else 4, D, slopes=alibi_slopes(H))


@pytest.mark.parametrize("D,dt,hkv", [(64, F16, 4), (128, BF16, 2), (256, F16, 2)])
def test_alibi_slopes_per_batch(D, dt, hkv):
    run_dense(dt, hkv, D, slopes=torch.stack([alibi_slopes(H), alibi_slopes(H, 0.5).flip(0)]))


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("D", DIMS)
def test_both_causal_with_offset(D, dt):
    run_dense(dt, 2 if dt == F16 else 4, D, softcap=30.0, slopes=alibi_slopes(H), causal=True, q_offset=NKV - NQ)


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("D", DIMS)
def test_both_under_a_window(D, dt):
    run_dense(dt, 4 if dt == F16 else 2, D, softcap=30.0, slopes=alibi_slopes(H), window=(63, 0))


@pytest.mark.parametrize("D,rows,dt", [(64, 128, F16), (64, 256, BF16), (128, 128, BF16), (128, 256, F16)])
def test_option_rows(D, rows, dt):
    run_dense(dt, 2, D, softcap=30.0, slopes=alibi_slopes(H), causal=True, q_offset=NKV - NQ, rows=rows)


@pytest.mark.parametrize("D,dt", [(512, F16), (72, BF16)])
def test_head_dims_512_and_72(D, dt):
    run_dense(dt, 2, D, softcap=30.0, slopes=alibi_slopes(H), causal=True, q_offset=NKV - NQ)


def test_bnhd_layout():
    run_dense(F16, 2, 128, softcap=30.0, slopes=torch.stack([alibi_slopes(H), alibi_slopes(H, 0.5)]), window=(63, 0), bnhd=True)


@pytest.mark.parametrize("dt", [F16, BF16])
def test_saturation(dt):
    """q, k = 16 * N(0, 1), D 64, softcap 1: |x / softcap| is in the hundreds — every output finite and within the bars.  Then the same inputs with
    one feature column of q and k set to 128, which pushes EVERY score beyond saturation (x ~ 2048 +- 8 sigma of 254): t = 1 exactly, so dQ and dK
    are exactly zero, P is uniform and dV is within its bar."""
    dev = _dev()
    inputs = make_inputs(dt, 4, 64, qk_mul=16.0, seed=7)
    run_dense(dt, 4, 64, softcap=1.0, inputs=inputs)
    q, k, v, do = (t.clone() for t in inputs)
    q[..., 0] = 128.0
    k[..., 0] = 128.0
    x = (q.double() @ k.double().transpose(-1, -2)) * 64 ** -0.5
    assert x.min().item() > 20.0
    run_dense(dt, 4, 64, softcap=1.0, inputs=(q, k, v, do))
    qd, kd, vd = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    flash_attention(qd, kd, vd, softcap=1.0).backward(do.to(dev))
    assert (qd.grad == 0).all() and (kd.grad == 0).all(), "gradients through saturated scores are zero"
    assert torch.isfinite(vd.grad).all() and (vd.grad != 0).any()


@pytest.mark.parametrize("D,dt", [(64, F16), (128, BF16), (256, F16)])
def test_negative_slopes(D, dt):
    """Slopes of either sign are served.  With a negative slope the modified score GROWS with the distance, so nothing bounds 2^(s log2e) of the rows
    >= Nq that a ragged last Q tile (200 = 3 * 64 + 8; |slope| * distance reaches 100 and more there) brings into the dK / dV passes: those rows have to be masked, not left to Q = dO = 0 (inf * 0).
    Full attention (no left bound: the case in which the windowed passes treat that tile as a plain one); every dK / dV shape: fused, wave pairs, sweeps."""
    run_dense(dt, 2, D, slopes=-torch.tensor([0.5, 0.4, 0.45, 0.5]))


# ---------------------------------------------------------------------------------------------------------------- packed
LENS_Q = [70, 1, 130, 0, 257]
LENS_K2 = [333, 5, 64, 9, 257]


@pytest.mark.parametrize("bottom_right", [False, True])
@pytest.mark.parametrize("same_keys", [True, False])
@pytest.mark.parametrize("D,dt,rows", [(64, F16, 128), (128, BF16, 256)])
def test_packed(D, dt, rows, same_keys, bottom_right):
    """Both features with per-sequence slopes on a packed batch, causal.  Each sequence's forward is bit-identical to the dense score-modifier call on that
    sequence alone with q_offset = the sequence's offset and the same `rows` (where the offset is >= 0: the dense entry point takes no negative one);
    each sequence is within the bars against float64; the call as a whole is not vacuous."""
    dev = _dev()
    hkv, softcap, scale = 2, 30.0, D ** -0.5
    lq, lk = LENS_Q, (LENS_Q if same_keys else LENS_K2)
    g = torch.Generator().manual_seed(5000 + D)
    mk = lambda n, h, mul: (torch.randn((n, h, D), generator=g) * mul).to(dt).to(dev)      # noqa: E731
    q, k, v, do = mk(sum(lq), H, 2.0), mk(sum(lk), hkv, 2.0), mk(sum(lk), hkv, 2.0), mk(sum(lq), H, 1.0)
    slopes = torch.stack([alibi_slopes(H, 1.0 + 0.25 * s) for s in range(len(lq))]).to(dev)
    cu = lambda lens: torch.tensor([0] + [sum(lens[:i + 1]) for i in range(len(lens))], dtype=torch.int32, device=dev)      # noqa: E731
    cu_q, cu_k = cu(lq), cu(lk)
    qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
    with _fa2_lib.options(rows=rows):
        o = flash_attention_varlen(qd, kd, vd, cu_q, cu_k, max(lq), max(lk), causal=True, bottom_right=bottom_right, softcap=softcap, alibi_slopes=slopes)
        o.backward(do)
        flags = _fa2_lib.FA2_FLAG_CAUSAL | (_fa2_lib.FA2_FLAG_BOTTOM_RIGHT if bottom_right else 0) | _fa2_lib.FA2_FLAG_EXACT_SCALE
        ret = flash_attn_wmma.forward_varlen(q, k, v, cu_q, cu_k, max(lq), max(lk), flags, scale, (-1, -1), scoremod=(softcap, slopes))
    assert torch.equal(ret[0], o.detach())
    lse = ret[5]
    hm = lambda t, a, n: t[a:a + n].transpose(0, 1)                                          # noqa: E731 - [n, heads, D] -> [heads, n, D]
    q0 = k0 = 0
    worst = {n: 0.0 for n in NAMES}
    for s, (nq, nk) in enumerate(zip(lq, lk)):
        tag = "%s D%d rows=%d br=%d seq %d (%d x %d)" % (str(dt)[6:], D, rows, bottom_right, s, nq, nk)
        if nq and nk:
            off = nk - nq if bottom_right else 0
            band = _ff.band(nq, nk, -1, 0, off, False, dev)
            refs = unit_refs(hm(q, q0, nq), hm(k, k0, nk), hm(v, k0, nk), hm(do, q0, nq), band, scale, softcap, slopes[s], off, dt, hkv)
            got = dict(O=hm(o.detach(), q0, nq), lse=lse[:, q0:q0 + nq], dQ=hm(qd.grad, q0, nq), dK=hm(kd.grad, k0, nk), dV=hm(vd.grad, k0, nk))
            # The >= 5x margin is not asked of every sequence: a 1 x 1 sequence, or a causal row with one visible key, has a softmax of 1 whatever the
            # score, so no modifier can move it.  It is asked of the call (the best sequence per output, after the loop).
            check_unit(tag, got, *refs, vacuous_ok=True)
            for n in NAMES:
                worst[n] = max(worst[n], margin(refs[0], refs[1], refs[3], n))
            # Bit-identity to the dense call, O and LSE.  Only where the sequence's offset is >= 0: the dense entry points refuse a negative q_offset
            # (bottom-right with fewer keys than queries exists in packed calls only); such a sequence is held to float64 above.
            if off >= 0:
                with _fa2_lib.options(rows=rows):
                    dense = flash_attn_wmma.forward_py(hm(q, q0, nq).unsqueeze(0), hm(k, k0, nk).unsqueeze(0), hm(v, k0, nk).unsqueeze(0), 64, 128,
                                                       _fa2_lib.FA2_FLAG_CAUSAL | _fa2_lib.FA2_FLAG_EXACT_SCALE, scale, False, window=(-1, -1, off),
                                                       scoremod=(softcap, slopes[s]))
                assert torch.equal(dense[0][0], got["O"]), (tag, "the packed forward differs from the dense call on the sequence alone")
                assert torch.equal(dense[5][0, :, :nq], got["lse"]), (tag, "the packed LSE differs from the dense call's")
        q0, k0 = q0 + nq, k0 + nk
    assert all(w >= 5.0 for w in worst.values()), worst


# ---------------------------------------------------------------------------------------------------------------- defaults
def test_default_keywords_take_today_s_path():
    dev = _dev()
    for dt, D, kw in ((F16, 128, dict(causal=True)), (BF16, 64, dict(window=(63, 0), q_offset=5)), (F16, 64, dict())):
        q, k, v, do = (t.to(dev) for t in make_inputs(dt, 2, D))
        outs = []
        for extra in (dict(), dict(softcap=0.0, alibi_slopes=None), dict(softcap=0)):
            qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
            o = flash_attention(qd, kd, vd, **kw, **extra)
            o.backward(do)
            outs.append((o.detach(), qd.grad, kd.grad, vd.grad))
        for other in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(outs[0], other)), (dt, D, kw)
    lq = [70, 1, 130, 0, 257]
    q, k, v, do = (t[0].transpose(0, 1).contiguous().to(dev) for t in make_inputs(F16, 2, 64, nq=sum(lq), nkv=sum(lq), b=1))
    cu = torch.tensor([0, 70, 71, 201, 201, 458], dtype=torch.int32, device=dev)
    outs = []
    for extra in (dict(), dict(softcap=0.0, alibi_slopes=None)):
        qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
        o = flash_attention_varlen(qd, kd, vd, cu, cu, 257, 257, causal=True, **extra)
        o.backward(do)
        outs.append((o.detach(), qd.grad, kd.grad, vd.grad))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("window", [(-1, -1, 0), (63, 0, 5)])
def test_c_abi_with_nothing_switched_on_is_the_windowed_call(window):
    dev = _dev()
    lib = _fa2_lib.load()
    D = 64
    q, k, v, _ = (t.to(dev) for t in make_inputs(F16, 2, D))
    s3 = lambda t: _fa2_lib.strides3(t.stride(0), t.stride(1), t.stride(2))      # noqa: E731
    outs = []
    for smod in (False, True):
        o = torch.full_like(q, float("nan"))
        lse = torch.full((B, H, NQ), float("nan"), dtype=torch.float32, device=dev)
        args = (0, q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, 2, NQ, NKV, D, s3(q), s3(k), s3(v), s3(o),
                _fa2_lib.strides2(H * NQ, NQ), D ** -0.5, 0, *window, torch.cuda.current_stream().cuda_stream)
        rc = lib.fa2_fwd_scoremod(*args, 0.0, None, 0) if smod else lib.fa2_fwd_window(*args)
        assert rc == 0, _fa2_lib.error_string(rc)
        torch.cuda.synchronize()
        outs.append((o, lse))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.isfinite(outs[0][0]).all()
