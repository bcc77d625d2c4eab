"""GPU tests of the merge of partial attention results: merge_attention (C-ABI fa2_merge_fwd / fa2_merge_bwd) and the ring pattern built from
flash_attention(..., return_lse=True) + merge_attention.

References: float64, written in tests/lse_refs.py.  The ring pattern is compared with the float64 result of the ONE full call (truth64) under the
project's bar rule; its emulation follows the path itself: the parts from the f32 emulation of each partial call (outputs rounded to the I/O dtype),
merged in f32, rounded once, and the gradients of the emulated full call.  The kernel contract is compared directly with the float64 merge and its
autograd: the forward's only roundings are the f32 arithmetic and the final one (bar: one rounding of the I/O dtype at the largest magnitude, FLOOR-style
2^-11 / 2^-8 relative, written out below); the LSE in log2 units within LSE_TOL."""
import ctypes

import pytest
import torch

import lse_refs as R
from conftest import LSE_TOL
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention, merge_attention

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]
LN2 = R.LN2
EPS = R.MERGE_EPS                                # half an ulp at 1: one round-to-nearest of the I/O dtype


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("these tests need a ROCm device")
    return torch.device("cuda")


# ---------------------------------------------------------------------------------------------------------------- ring pattern
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_ring_pattern_matches_the_full_call(D, dt):
    """Three blocks of 80 rows, causal band of 100 keys: Q block r against KV block s <= r with q_offset = (r - s) * 80, the r + 1 parts merged, the blocks
    concatenated.  The (2, 0) part has rows 20 .. 79 dead (zero-weight parts); the loss on out alone already sends gradient through the partial LSEs."""
    dev = _dev()
    Hh, n, nb, W = 4, 80, 3, 100
    N = n * nb
    g = torch.Generator().manual_seed(0)
    mk = lambda shape, mul: (torch.randn(shape, generator=g) * mul).to(dt).to(dev)      # noqa: E731
    q, k, v, do = mk((1, Hh, N, D), 2.0), mk((1, Hh, N, D), 2.0), mk((1, Hh, N, D), 2.0), mk((1, Hh, N, D), 1.0)
    u = torch.randn((1, Hh, N), generator=g).to(dev)
    scale = D ** -0.5
    qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
    blk = lambda t, i: t[:, :, i * n:(i + 1) * n]      # noqa: E731
    outs, lses, dead_part_rows = [], [], 0
    for r in range(nb):
        po, pl = [], []
        for s in range(r + 1):
            o_, l_ = flash_attention(blk(qd, r), blk(kd, s), blk(vd, s), causal=True, window=(W, 0), q_offset=(r - s) * n, return_lse=True)
            dead_part_rows += int(torch.isneginf(l_).sum())
            po.append(o_)
            pl.append(l_)
        o_, l_ = merge_attention(po, pl)
        outs.append(o_)
        lses.append(l_)
    out, lse = torch.cat(outs, 2), torch.cat(lses, 2)
    assert dead_part_rows == Hh * 60, "the (2, 0) part must have rows 20 .. 79 dead in every head"
    ((out.float() * do.float()).sum() + (lse * u).sum()).backward()

    allow = R.ff.band(N, N, W, 0, 0, True, dev)
    true = R.truth64(q[0], k[0], v[0], do[0], u[0], allow, scale)
    plain = R.truth64(q[0], k[0], v[0], do[0], None, allow, scale)
    emu = R.emulate(q[0], k[0], v[0], do[0], u[0], allow, scale, dt)
    # the emulation of out / lse follows the path: emulated parts (rounded to the I/O dtype), merged in f32, rounded once
    eo, el = [], []
    for r in range(nb):
        po, pl = [], []
        for s in range(r + 1):
            a = R.ff.band(n, n, W, 0, (r - s) * n, True, dev)
            e = R.emulate(blk(q, r)[0], blk(k, s)[0], blk(v, s)[0], blk(do, r)[0], None, a, scale, dt)
            po.append(e["O"].to(dt).float())
            pl.append((e["lse"] * LN2).float())
        L = torch.stack(pl)
        m = L.max(0).values
        w = torch.exp(L - m)
        eo.append(((w.unsqueeze(-1) * torch.stack(po)).sum(0) / w.sum(0).unsqueeze(-1)).to(dt).double())
        el.append(((m + torch.log(w.sum(0))) / LN2).double())
    emu["O"], emu["lse"] = torch.cat(eo, 1), torch.cat(el, 1)
    bars = R.bars_of(true, emu, dt)
    tag = "ring %s D%d" % (str(dt)[6:], D)
    R.check(tag, dict(O=out.detach()[0], lse=lse.detach()[0] / LN2, dQ=qd.grad[0], dK=kd.grad[0], dV=vd.grad[0]), true, bars)
    R.check_not_vacuous(tag, true, plain, bars)


# ---------------------------------------------------------------------------------------------------------------- the kernel contract
def _merge_case(dt, nparts, D, nq, layout, natural, dev, seed=0):
    """Parts with LSEs spread over ~40 log2 units, one all -inf row, -inf parts holding large-finite garbage -> (outs, lses) in the kernel's layout;
    layout: 'bhnd', 'bnhd' or 'packed'."""
    Bb, Hh = (1, 3) if layout == "packed" else (2, 3)
    g = torch.Generator().manual_seed(500 + seed)
    outs, lses = [], []
    for kx in range(nparts):
        o = torch.randn((Bb, Hh, nq, D), generator=g)
        l = torch.randn((Bb, Hh, nq), generator=g) * 6.0
        drop = torch.rand((Bb, Hh, nq), generator=g) < (0.3 if nparts > 1 else 0.0)
        l[drop] = float("-inf")
        o[drop] = 65504.0 if kx % 2 else -3.0e4                        # garbage under weight 0
        if nq > 1:
            l[:, :, 0] = float("-inf")                                 # row 0: no part saw a key
        outs.append(o.to(dt))
        lses.append(l if natural else l / LN2)
    if layout == "bnhd":
        outs = [o.transpose(1, 2).contiguous().to(dev) for o in outs]
    elif layout == "packed":
        outs = [o[0].transpose(0, 1).contiguous().to(dev) for o in outs]
        lses = [l[0] for l in lses]
    else:
        outs = [o.to(dev) for o in outs]
    return outs, [l.contiguous().to(dev) for l in lses]


def _raw_merge(outs, lses, layout, natural, dout, dlse):
    """fa2_merge_fwd, then fa2_merge_bwd, straight through the C-ABI -> (out, lse, do_parts, dlse_parts)."""
    lib = _fa2_lib.load()
    n = len(outs)
    o0 = outs[0]
    if layout == "packed":
        geo, s3, s2 = (1, o0.shape[1], o0.shape[0], o0.shape[2]), (lambda t: _fa2_lib.strides3(0, t.stride(1), t.stride(0))), (lambda t: _fa2_lib.strides2(0, t.stride(0)))
    elif layout == "bnhd":
        geo, s3, s2 = (o0.shape[0], o0.shape[2], o0.shape[1], o0.shape[3]), (lambda t: _fa2_lib.strides3(t.stride(0), t.stride(2), t.stride(1))), (lambda t: _fa2_lib.strides2(t.stride(0), t.stride(1)))
    else:
        geo, s3, s2 = tuple(o0.shape), (lambda t: _fa2_lib.strides3(t.stride(0), t.stride(1), t.stride(2))), (lambda t: _fa2_lib.strides2(t.stride(0), t.stride(1)))
    arr = lambda ts: (ctypes.c_void_p * n)(*(t.data_ptr() for t in ts))      # noqa: E731
    out, lse = torch.full_like(o0, 7.0), torch.full_like(lses[0], 7.0)
    flags = _fa2_lib.FA2_MERGE_NATURAL_LSE if natural else 0
    stream = torch.cuda.current_stream().cuda_stream
    code = R.code(o0.dtype)
    _fa2_lib.check(lib.fa2_merge_fwd(code, n, arr(outs), arr(lses), out.data_ptr(), lse.data_ptr(), *geo, s3(o0), s2(lses[0]), s3(out), s2(lse), flags, stream))
    dos, dls = [torch.full_like(o0, 7.0) for _ in range(n)], [torch.full_like(lse, 7.0) for _ in range(n)]
    _fa2_lib.check(lib.fa2_merge_bwd(code, n, arr(outs), arr(lses), lse.data_ptr(), dout.data_ptr(), None if dlse is None else dlse.data_ptr(), arr(dos), arr(dls),
                                     *geo, s3(o0), s2(lses[0]), s2(lse), s3(dout), None if dlse is None else s2(dlse), s3(dos[0]), s2(dls[0]), flags, stream))
    torch.cuda.synchronize()
    return out, lse, dos, dls


CONTRACT_CASES = [(1, 64, 203, "bhnd"), (2, 8, 203, "bhnd"), (5, 136, 203, "bnhd"), (16, 512, 1, "bhnd"), (16, 64, 203, "packed"), (2, 512, 203, "bhnd"),
                  (5, 64, 1, "packed")]


def _views(layout):
    """(outs' view as [B, H, N, D], lses' view as [B, H, N]) of the kernel's layout."""
    if layout == "packed":
        return (lambda t: t.transpose(0, 1).unsqueeze(0)), (lambda t: t.unsqueeze(0))
    if layout == "bnhd":
        return (lambda t: t.transpose(1, 2)), (lambda t: t)
    return (lambda t: t), (lambda t: t)


@pytest.mark.parametrize("natural", [True, False], ids=["natural", "log2"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("nparts,D,nq,layout", CONTRACT_CASES)
def test_merge_kernels_match_the_float64_contract(nparts, D, nq, layout, dt, natural):
    dev = _dev()
    outs, lses = _merge_case(dt, nparts, D, nq, layout, natural, dev)
    g = torch.Generator().manual_seed(900)
    dout = torch.randn(outs[0].shape, generator=g).to(dt).to(dev)
    dlse = torch.randn(lses[0].shape, generator=g).to(dev)
    out, lse, dos, dls = _raw_merge(outs, lses, layout, natural, dout, dlse)
    vo, vl = _views(layout)
    tag = "merge %s n%d D%d Nq%d %s %s" % (str(dt)[6:], nparts, D, nq, layout, "natural" if natural else "log2")
    R.merge_check(tag, dt, natural, [vo(o) for o in outs], [vl(l) for l in lses], vo(dout), vl(dlse), vo(out), vl(lse), [vo(t) for t in dos], [vl(t) for t in dls])


@pytest.mark.parametrize("natural", [True, False], ids=["natural", "log2"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_one_part_with_large_lses_is_the_identity(dt, natural):
    """One part whose LSEs sit near -200: the merged LSE is the part's bit for bit and the backward's weight exactly 1, so dO_0 = dO and dlse_0 = dlse.
    The reduced form of what tools/fuzz_lse.py's merge runs flagged (seed 203, six one-part cases, D 216 .. 384): the kernels converted every LSE to
    log2 units BEFORE subtracting, two roundings at the LSEs' magnitude, so the weight came out as 1 +- 4e-5 and dlse_0 carried (dO.O_0) times that —
    4e-4 against a bar of 1e-4.  They now subtract in the LSEs' own unit and scale the difference."""
    dev = _dev()
    outs, lses = _merge_case(dt, 1, 272, 129, "bhnd", natural, dev, seed=4)
    lses = [l - 200.0 for l in lses]
    g = torch.Generator().manual_seed(901)
    dout = torch.randn(outs[0].shape, generator=g).to(dt).to(dev)
    dlse = torch.randn(lses[0].shape, generator=g).to(dev)
    out, lse, dos, dls = _raw_merge(outs, lses, "bhnd", natural, dout, dlse)
    live = ~torch.isneginf(lses[0])
    assert live.any() and not live.all()
    assert torch.equal(lse, lses[0]) and torch.equal(out[live], outs[0][live])
    assert torch.equal(dos[0][live], dout[live]) and torch.equal(dls[0][live], dlse[live]) and (dls[0][~live] == 0).all()
    R.merge_check("one part %s %s" % (str(dt)[6:], "natural" if natural else "log2"), dt, natural, outs, lses, dout, dlse, out, lse, dos, dls)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_seventeen_parts_fold_in_groups(dt):
    dev = _dev()
    outs, lses = _merge_case(dt, 17, 64, 203, "bhnd", True, dev, seed=1)
    out, lse = merge_attention(outs, lses)
    O64, L64 = R.merge64(outs, lses)
    dead = torch.isneginf(L64)
    assert torch.isneginf(lse[dead]).all() and (out[dead] == 0).all()
    err_o, err_l = (out.double() - O64).abs().max().item(), ((lse.double() - L64)[~dead] / LN2).abs().max().item()
    bar_o = 4 * EPS[dt] * max(1.0, O64.abs().max().item())               # two folds: the first group's out is rounded, then the result
    print("17 parts %s: O err %.3g (bar %.3g), lse err %.3g" % (str(dt)[6:], err_o, bar_o, err_l))
    assert err_o <= bar_o and err_l <= LSE_TOL


def test_merge_operator_is_differentiable_in_outs_and_lses():
    dev = _dev()
    outs, lses = _merge_case(BF16, 3, 72, 50, "bhnd", True, dev, seed=2)
    outs = [o[..., :68].clone().requires_grad_(True) for o in outs]        # a head dim that is no multiple of 8: padded inside
    lses = [l.clone().requires_grad_(True) for l in lses]
    out, lse = merge_attention(outs, lses)
    live = ~torch.isneginf(lse.detach())
    g = torch.Generator().manual_seed(5)
    do, u = torch.randn(out.shape, generator=g).to(dev), torch.randn(lse.shape, generator=g).to(dev)
    ((out.float() * do).sum() + (lse * u).masked_fill(~live, 0.0).sum()).backward()
    o64 = [torch.where(torch.isneginf(l).unsqueeze(-1), torch.zeros_like(o), o).detach().double().requires_grad_(True) for o, l in zip(outs, lses)]
    l64 = [l.detach().double().requires_grad_(True) for l in lses]
    O64, L64 = R.merge64(o64, l64)
    ((O64 * do.to(BF16).double()).sum() + (L64.masked_fill(~live, 0.0) * u.double()).masked_fill(~live, 0.0).sum()).backward()
    for a, b, c, d in zip(outs, o64, lses, l64):
        assert a.grad.shape == a.shape
        assert (a.grad.double() - b.grad).abs().max().item() <= 2 * EPS[BF16] * max(1.0, b.grad.abs().max().item())
        assert (c.grad.double() - d.grad).abs().max().item() <= 1e-4 * max(1.0, d.grad.abs().max().item())


def test_merge_call_replays_from_a_graph():
    """The parts' pointers travel by value in the kernel's argument block: a captured call replays without any host array."""
    dev = _dev()
    outs, lses = _merge_case(F16, 5, 128, 203, "bhnd", True, dev, seed=3)
    eager_o, eager_l = merge_attention(outs, lses)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        merge_attention(outs, lses)                                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        go, gl = merge_attention(outs, lses)
    go.zero_()
    gl.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(go, eager_o) and torch.equal(gl, eager_l)
