"""References and the check of the decode tests (tests/test_decode_gpu.py, tests/test_decode_fp8_gpu.py, the decode cases of the far-offset tests).

Per sequence, on k[:len_b]: the repository's oracle with the bottom-right causal band given as a -inf bias (fa2_oracle.fwd_c: the same contract 0
arithmetic) and dense float64 (fwd_numpy).  FP8 caches with power-of-two descales: every finite e4m3 value is a f16 and a bf16 value and a power
of two commutes with every rounding, so the oracle runs unchanged on the cache upcast to q's dtype and multiplied by k_descale (exact), its O
multiplied by v_descale (exact).  Bars: conftest's ATOL / RTOL / LSE_TOL against the oracle, 2 * FLOOR and LSE_TOL against float64.  Plain CPU code:
nothing here touches a device."""
import numpy as np
import torch

from conftest import ATOL, FLOOR, LSE_TOL, RTOL
from oracle import fa2_oracle as fo


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def band(n, Nq):
    """keep [Nq, n]: row i at position n - Nq + i sees keys j <= it; the same as a -inf bias"""
    keep = np.arange(n)[None, :] <= (n - Nq + np.arange(Nq))[:, None]
    return keep, np.where(keep, 0.0, -np.inf).astype(np.float32)


def refs16(q, k, v, lens, code):
    """q [B, Nq, H, D], k / v [B, Nmax, Hkv, D] (CPU, the I/O dtype) -> per sequence None (no keys) or (oracle O, oracle LSE, float64 O, float64 LSE,
    dead rows)."""
    Nq, G, refs = q.shape[1], q.shape[2] // k.shape[2], []
    for b, n in enumerate(lens):
        if n == 0:
            refs.append(None)
            continue
        keep, bias = band(n, Nq)
        qs = q[b].transpose(0, 1).unsqueeze(0).contiguous()                               # [1, H, Nq, D]
        ks, vs = (t[b, :n].transpose(0, 1).repeat_interleave(G, dim=0).unsqueeze(0).contiguous() for t in (k, v))
        o_bits, lse_ref = fo.fwd_c(bits16(qs), bits16(ks), bits16(vs), code, False, bias=bias)
        o_true, lse_true = fo.fwd_numpy(qs.float().numpy(), ks.float().numpy(), vs.float().numpy(), False, bias=bias)
        refs.append((fo.bits_to_f32(o_bits, code), lse_ref, o_true, lse_true, ~keep.any(1)))
    return refs


def seq_inputs_fp8(q, k8, v8, kd, vd, b, n, Nq, G):
    """sequence b: q [1, H, Nq, D]; f32 K * k_descale and V (no descale), V * v_descale, [1, H, n, D], heads repeated; the causal band as a bias"""
    keep, bias = band(n, Nq)
    qs = q[b].transpose(0, 1).unsqueeze(0).contiguous()
    rep = lambda t: t.transpose(0, 1).repeat_interleave(G, dim=0).unsqueeze(0).contiguous()      # noqa: E731
    one = torch.ones(k8.shape[2])
    ks = rep(k8[b, :n].float() * (one if kd is None else kd[b])[None, :, None])
    vraw = rep(v8[b, :n].float())
    vs = rep(v8[b, :n].float() * (one if vd is None else vd[b])[None, :, None])
    return qs, ks, vraw, vs, keep, bias


def refs_fp8(q, k8, v8, kd, vd, lens, code):
    """The same for e4m3 caches k8 / v8 with power-of-two descales kd / vd [B, Hkv] (None = 1).  The oracle's own result on these inputs is checked
    against float64 here, on the CPU."""
    dt, Nq, G, refs = q.dtype, q.shape[1], q.shape[2] // k8.shape[2], []
    for b, n in enumerate(lens):
        if n == 0:
            refs.append(None)
            continue
        qs, ks, vraw, vs, keep, bias = seq_inputs_fp8(q, k8, v8, kd, vd, b, n, Nq, G)
        assert torch.equal(ks.to(dt).float(), ks) and torch.equal(vraw.to(dt).float(), vraw), "the upcast, descaled cache is exact in q's dtype"
        o_bits, lse_ref = fo.fwd_c(bits16(qs), bits16(ks.to(dt)), bits16(vraw.to(dt)), code, False, bias=bias)
        vdh = (torch.ones(k8.shape[2]) if vd is None else vd[b]).repeat_interleave(G).numpy()[None, :, None, None]
        o_ref = fo.bits_to_f32(o_bits, code) * vdh                                        # a power of two: exact, commutes with the oracle's rounding
        o_true, lse_true = fo.fwd_numpy(qs.float().numpy(), ks.numpy(), vs.numpy(), False, bias=bias)
        live = keep.any(1)
        assert np.abs(o_ref - o_true)[:, :, live].max() <= FLOOR[code], "the oracle itself against float64 (CPU, before any GPU run)"
        assert np.abs(lse_ref[..., live] - lse_true[..., live]).max() <= LSE_TOL
        refs.append((o_ref, lse_ref, o_true, lse_true, ~live))
    return refs


def check(o, lse2, refs, lens, code, tag, oracle=True, verbose=False):
    """o [B, Nq, H, D] and the log2 lse [B, H, Nq] against the references; dead rows exactly 0 / -inf, every element written."""
    got_o, got_l = o.float().cpu(), lse2.cpu()
    assert torch.isfinite(got_o).all(), (tag, "O not finite: an element was not written, or a NaN beyond a length leaked")
    assert not torch.isnan(got_l).any(), (tag, "LSE not written")
    for b, ref in enumerate(refs):
        go = got_o[b].transpose(0, 1).unsqueeze(0).numpy()
        gl = got_l[b].unsqueeze(0).numpy()
        if ref is None:
            assert np.all(go == 0.0) and np.all(np.isneginf(gl)), (tag, b, "a sequence without keys")
            continue
        o_ref, lse_ref, o_true, lse_true, dead = ref
        assert np.all(go[:, :, dead] == 0.0) and np.all(np.isneginf(gl[:, :, dead])), (tag, b, "rows at a negative position")
        err_t = np.abs(go - o_true)
        if verbose:
            print(tag, "len", lens[b], "float64 O err %.3g" % err_t.max(), "" if not oracle else "oracle O err %.3g" % np.abs(go - o_ref).max())
        if oracle:
            err_o = np.abs(go - o_ref)
            assert np.all(err_o <= ATOL[code] + RTOL[code] * np.abs(o_ref)), (tag, b, lens[b], "oracle O", float(err_o.max()))
        assert err_t.max() <= 2 * FLOOR[code], (tag, b, lens[b], "float64 O", float(err_t.max()))
        if (~dead).any():
            if oracle:
                assert np.abs(gl[..., ~dead] - lse_ref[..., ~dead]).max() <= LSE_TOL, (tag, b, lens[b], "oracle LSE")
            assert np.abs(gl[..., ~dead] - lse_true[..., ~dead]).max() <= LSE_TOL, (tag, b, lens[b], "float64 LSE")


def same_lse(a, b):
    """two log2 LSE tensors agree within LSE_TOL, -inf in the same places"""
    fa, fb = torch.isfinite(a), torch.isfinite(b)
    return torch.equal(fa, fb) and torch.equal(a[~fa], b[~fb]) and (not fa.any() or float((a[fa] - b[fb]).abs().max()) <= LSE_TOL)
