"""KV-cache decode attention on the GPU: fa2_fwd_decode and flash_attention_decode.

The reference is the repository's oracle run PER SEQUENCE on k[:len_b], the bottom-right causal band given as a -inf bias (fa2_oracle.fwd_c: the same
contract 0 arithmetic; fwd_numpy: dense float64), as tests/test_varlen_gpu.py does.  Tolerances are tests/conftest.py's: ATOL / RTOL / LSE_TOL
against the oracle, 2 * FLOOR against float64.  One batch of nine sequences covers a length of 0, lengths below Nq, both sides of the 32- and
64-key tile edges and a long one; every cache row at or beyond a sequence's length holds NaN in K and in V, outputs and the workspace are
pre-filled with NaN.  The references of a shape are computed once and shared by every split, the paged and the strided calls.
No test feeds an out-of-range length or page id to the GPU: the clamps are checked on the CPU (tests/test_decode.py)."""
import functools
import math

import numpy as np
import pytest
import torch

import decode_calls as dc
import decode_refs as dr
from conftest import ATOL, LSE_TOL, RTOL
from rocwmma_fattn.FlashAttn import flash_attention_decode, flash_attention_varlen, merge_attention

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
LENS = (1, 63, 64, 65, 127, 129, 1000, 0, 2)
NMAX = 1024
SPLITS = (0, 1, 2, 3, 16)
LOG2E = 1.4426950408889634
# (H, Hkv, Nq, D, dtype): rows per K / V head 1, 4, 12 (one tile), 9, 16, 20 (two tiles, a ragged last one), 48 (three: the four-tile kernel), 64
SHAPES = [(8, 8, 1, 128, F16), (8, 8, 4, 64, BF16), (8, 8, 3, 128, F16), (8, 2, 3, 128, BF16), (8, 2, 1, 64, F16), (12, 4, 4, 128, F16), (12, 4, 3, 64, BF16),
          (16, 1, 4, 128, BF16), (16, 1, 3, 64, F16), (16, 1, 1, 128, F16), (10, 2, 4, 128, F16), (10, 2, 4, 64, BF16)]
IDS = ["H%d_Hkv%d_Nq%d_D%d_%s" % (s[0], s[1], s[2], s[3], "f16" if s[4] == F16 else "bf16") for s in SHAPES]


@functools.lru_cache(maxsize=None)
def _case(H, Hkv, Nq, D, dt):
    """CPU tensors of one shape (cache rows at or beyond len_b are NaN) and, per sequence, the oracle's and the float64 results.  Computed once."""
    g = torch.Generator(device="cpu").manual_seed(1000 * H + 100 * Hkv + 10 * Nq + D)
    B = len(LENS)
    q = torch.randn((B, Nq, H, D), generator=g).to(dt)
    k = torch.randn((B, NMAX, Hkv, D), generator=g).to(dt)
    v = torch.randn((B, NMAX, Hkv, D), generator=g).to(dt)
    for b, n in enumerate(LENS):
        k[b, n:] = float("nan")
        v[b, n:] = float("nan")
    refs = dr.refs16(q, k, v, LENS, dc.code(dt))
    return q, k, v, refs


def _check(o, lse2, refs, dt, tag):
    """o [B, Nq, H, D] and the log2 lse [B, H, Nq] (device) against the shared references; dead rows exactly 0 / -inf, every element written."""
    dr.check(o, lse2, refs, LENS, dc.code(dt), tag)


_same_lse = dr.same_lse


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_lengths_shapes_and_splits(shape):
    dev = dc.dev()
    H, Hkv, Nq, D, dt = shape
    q, k, v, refs = _case(*shape)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    lse1 = None
    for ns in SPLITS:
        o, lse = dc.decode_c("plain", qd, kd, vd, lens, ns)
        _check(o, lse, refs, dt, (shape[:4], "splits", ns))
        if ns == 1:
            lse1 = lse
        elif ns > 1:
            assert _same_lse(lse, lse1), (shape[:4], ns, "LSE of the split against split 1")


@pytest.mark.parametrize("page", [64, 128])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[8], SHAPES[11]], ids=[IDS[0], IDS[3], IDS[8], IDS[11]])
def test_paged_is_bit_identical_to_contiguous(shape, page):
    dev = dc.dev()
    q, k, v, refs = _case(*shape)
    pk, pv, bt = dc.paged(k, v, LENS, page, torch.Generator(device="cpu").manual_seed(page))
    qd, lens = q.to(dev), torch.tensor(LENS, dtype=torch.int32, device=dev)
    kd, vd, pkd, pvd, btd = k.to(dev), v.to(dev), pk.to(dev), pv.to(dev), bt.to(dev)
    for ns in SPLITS[1:]:
        o, lse = dc.decode_c("plain", qd, kd, vd, lens, ns)
        po, plse = dc.decode_c("plain", qd, pkd, pvd, lens, ns, block_table=btd)
        assert torch.equal(po.view(torch.int16), o.view(torch.int16)) and torch.equal(plse, lse), (shape[:4], page, ns)
    po, plse = dc.decode_c("plain", qd, pkd, pvd, lens, 0, block_table=btd)          # the plan's own split of the paged call (its capacity is the block table's)
    _check(po, plse, refs, shape[4], (shape[:4], "paged", page))


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[9], SHAPES[10]], ids=[IDS[3], IDS[9], IDS[10]])
def test_strided_views_are_bit_identical(shape):
    dev = dc.dev()
    H, Hkv, Nq, D, dt = shape
    q, k, v, _ = _case(*shape)
    B = q.shape[0]
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    qw = torch.full((B, Nq, H + 2, D), float("nan"), dtype=dt, device=dev)
    qw[:, :, :H] = qd
    kw = torch.full((B, NMAX + 40, Hkv, D), float("nan"), dtype=dt, device=dev)       # a padded Nmax stride
    kw[:, :NMAX] = kd
    for ns in (1, 3):
        o, lse = dc.decode_c("plain", qd, kd, vd, lens, ns)
        ow = torch.full((B, Nq, H + 2, D), float("nan"), dtype=dt, device=dev)
        so, slse = dc.decode_c("plain", qw[:, :, :H], kw[:, :NMAX], vd, lens, ns, o=ow[:, :, :H])
        assert not qw[:, :, :H].is_contiguous() and not kw[:, :NMAX].is_contiguous()
        assert torch.equal(so.view(torch.int16), o.view(torch.int16)) and torch.equal(slse, lse), (shape[:4], ns)
        assert torch.isnan(ow[:, :, H:]).all(), "the call wrote outside its view of o"
        # the operator: a strided q and cache view, o of its own
        po, pl = flash_attention_decode(qw[:, :, :H], kw[:, :NMAX], vd, lens, return_lse=True, num_splits=ns)
        assert torch.equal(po.view(torch.int16), o.view(torch.int16)), (shape[:4], ns, "flash_attention_decode")
        assert _same_lse(pl * LOG2E, lse)


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[5], SHAPES[7]], ids=[IDS[3], IDS[5], IDS[7]])
def test_against_packed_varlen(shape):
    """flash_attention_varlen(causal=True, bottom_right=True) on a packed copy of the valid keys: the route the library had before."""
    dev = dc.dev()
    H, Hkv, Nq, D, dt = shape
    q, k, v, _ = _case(*shape)
    code = dc.code(dt)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    o = flash_attention_decode(q.to(dev), k.to(dev), v.to(dev), lens)
    cu_q = torch.arange(0, (len(LENS) + 1) * Nq, Nq, dtype=torch.int32, device=dev)
    cu_k = torch.tensor(np.concatenate([[0], np.cumsum(LENS)]), dtype=torch.int32, device=dev)
    kp = torch.cat([k[b, :n] for b, n in enumerate(LENS)]).to(dev)
    vp = torch.cat([v[b, :n] for b, n in enumerate(LENS)]).to(dev)
    want = flash_attention_varlen(q.reshape(-1, H, D).to(dev), kp, vp, cu_q, cu_k, Nq, max(LENS), causal=True, bottom_right=True)
    got, want = o.reshape(-1, H, D).float().cpu().numpy(), want.float().cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(want).all()
    assert np.all(np.abs(got - want) <= ATOL[code] + RTOL[code] * np.abs(want)), float(np.abs(got - want).max())


@pytest.mark.parametrize("ns", [0, 3])
def test_graph_replay_follows_lengths_changed_in_place(ns):
    """The host never reads cache_seqlens: one captured call, replayed after the lengths were overwritten in place, gives the eager result for the
    contents at that time (a fully valid cache here, so that every permutation of the lengths is a legal call)."""
    dev = dc.dev()
    H, Hkv, Nq, D, dt = 8, 2, 3, 128, F16
    g = torch.Generator(device="cpu").manual_seed(77)
    q = torch.randn((len(LENS), Nq, H, D), generator=g).to(dt).to(dev)
    k, v = (torch.randn((len(LENS), NMAX, Hkv, D), generator=g).to(dt).to(dev) for _ in range(2))
    first = torch.tensor(LENS, dtype=torch.int32, device=dev)
    second = torch.tensor(LENS[3:] + LENS[:3], dtype=torch.int32, device=dev)
    want = [tuple(t.clone() for t in flash_attention_decode(q, k, v, x, return_lse=True, num_splits=ns)) for x in (first, second)]
    assert not torch.equal(want[0][0], want[1][0])
    lens = first.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flash_attention_decode(q, k, v, lens, return_lse=True, num_splits=ns)           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            go, gl = flash_attention_decode(q, k, v, lens, return_lse=True, num_splits=ns)
    torch.cuda.current_stream().wait_stream(side)
    for x, (wo, wl) in ((first, want[0]), (second, want[1]), (first, want[0])):
        lens.copy_(x)
        go.zero_()
        gl.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(go.view(torch.int16), wo.view(torch.int16)) and torch.equal(gl, wl)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_return_lse_composes_with_merge_attention(dt):
    """A cache of 512 keys as two 256-key halves (Nq = 1: no causal interaction): merge_attention of the two decode results is the one-call result."""
    dev = dc.dev()
    B, H, Hkv, D = 3, 8, 2, 128
    code = dc.code(dt)
    g = torch.Generator(device="cpu").manual_seed(5)
    q = torch.randn((B, 1, H, D), generator=g).to(dt).to(dev)
    k, v = (torch.randn((B, 512, Hkv, D), generator=g).to(dt).to(dev) for _ in range(2))
    full = torch.full((B,), 512, dtype=torch.int32, device=dev)
    half = torch.full((B,), 256, dtype=torch.int32, device=dev)
    o, lse = flash_attention_decode(q, k, v, full, return_lse=True)
    parts = [flash_attention_decode(q, k[:, s:s + 256], v[:, s:s + 256], half, return_lse=True) for s in (0, 256)]
    assert lse.shape == (B, H, 1) and lse.dtype == torch.float32
    mo, ml = merge_attention([p[0] for p in parts], [p[1] for p in parts], BNHD_fmt=True)
    got, want = mo.float().cpu().numpy(), o.float().cpu().numpy()
    assert np.all(np.abs(got - want) <= ATOL[code] + RTOL[code] * np.abs(want)), float(np.abs(got - want).max())
    assert float((ml - lse).abs().max()) * LOG2E <= LSE_TOL
    # ... and the natural-log LSE is the float64 one
    s = torch.einsum("bqhd,bkhd->bhqk", q.double().cpu(), k.double().cpu().repeat_interleave(H // Hkv, dim=2)) * D ** -0.5
    assert float((lse.cpu().double() - torch.logsumexp(s, dim=-1)).abs().max()) * LOG2E <= LSE_TOL
    assert math.isclose(float(lse[0, 0, 0]), float(torch.logsumexp(s, dim=-1)[0, 0, 0]), abs_tol=1e-3)
