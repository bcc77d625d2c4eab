"""References, inputs and the C-ABI call of the latent-cache (MLA) decode tests (tests/test_decode_mla.py, tests/test_decode_mla_gpu.py,
tests/test_decode_mla_far_gpu.py).

Per sequence, on kv[:len_b]: the repository's oracle at head dim 576 with v = k, whose first 512 O columns are the contract-0 result (O's columns are
independent), under decode's band as a -inf bias, and dense float64 (fwd_numpy takes the 512-wide V beside the 576-wide K).  For every case it builds,
refs() asserts on the CPU that the oracle alone meets the float64 bar, before any GPU result is looked at.  The bars are decode_refs.check's, unchanged.
mla_f64 is the float64 formula again with switches that break it one way each: tests/test_decode_mla.py shows that the check refuses every one.
Plain CPU code; mla_c alone touches a device."""
import ctypes

import numpy as np
import torch

import decode_calls as dc
from conftest import FLOOR, LSE_TOL
from decode_refs import band, bits16
from oracle import fa2_oracle as fo
from rocwmma_fattn import _fa2_lib

D, DV = 576, 512
SCALE = D ** -0.5
LOG2E = 1.4426950408889634
CPU_CASES = ((16, 1, 1), (16, 2, 33), (5, 3, 97), (128, 1, 300), (16, 4, 1000))       # (H, Nq, len): the cases the bars were checked on


def inputs(B, H, Nq, nmax, lens, dtype, seed, poison=True):
    """N(0, 1) q [B, Nq, H, 576] and latent cache [B, nmax, 576] in `dtype`; rows at or beyond a length hold NaN."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn((B, Nq, H, D), generator=g).to(dtype)
    kv = torch.randn((B, nmax, D), generator=g).to(dtype)
    if poison:
        for b, n in enumerate(lens):
            kv[b, n:] = float("nan")
    return q, kv


def refs(q, kv, lens, code, scale=SCALE):
    """q [B, Nq, H, 576], kv [B, Nmax, 576] (CPU, the I/O dtype) -> per sequence None (no keys) or (oracle O, oracle LSE, float64 O, float64 LSE, dead rows)"""
    Nq, H, out = q.shape[1], q.shape[2], []
    for b, n in enumerate(lens):
        if n == 0:
            out.append(None)
            continue
        keep, bias = band(n, Nq)
        qs = q[b].transpose(0, 1).unsqueeze(0).contiguous()                               # [1, H, Nq, 576]
        ks = kv[b, :n].unsqueeze(0).expand(H, n, D).unsqueeze(0).contiguous()             # [1, H, n, 576]: the one latent row under every head
        o_bits, lse_ref = fo.fwd_c(bits16(qs), bits16(ks), bits16(ks), code, False, scale=scale, bias=bias)
        o_ref = fo.bits_to_f32(o_bits, code)[..., :DV]
        o_true, lse_true = fo.fwd_numpy(qs.float().numpy(), ks.float().numpy(), ks[..., :DV].float().numpy(), False, scale=scale, bias=bias)
        live = keep.any(1)
        assert np.abs(o_ref - o_true)[:, :, live].max() <= 2 * FLOOR[code], "the oracle itself against float64 (CPU, before any GPU run)"
        assert np.abs(lse_ref[..., live] - lse_true[..., live]).max() <= LSE_TOL
        out.append((o_ref, lse_ref, o_true, lse_true, ~live))
    return out


def mla_f64(q, kv, lens, scale=SCALE, mutant=None, parts=1):
    """The formula in float64, key by key as the kernel sees it -> (o [B, Nq, H, 512] f32, log2 lse [B, H, Nq] f32).  mutant: None, or one of
    'k512' (scores from the first 512 columns), 'v64' (V from columns 64 .. 575), 'rowmap' (packed row r = h * Nq + i), 'dropkey' (one key missing),
    'diag' (the causal diagonal one key too far), 'norescale' (two parts merged without rescaling the accumulators; needs parts = 2)."""
    B, Nq, H, _ = q.shape
    o = np.zeros((B, Nq, H, DV))
    lse = np.full((B, H, Nq), -np.inf)
    for b, n in enumerate(lens):
        if n == 0:
            continue
        qb, kb = q[b].double().numpy(), kv[b, :n].double().numpy()
        kk = kb[:, :DV] if mutant == "k512" else kb
        s = np.einsum("ihd,jd->ihj", qb[..., :kk.shape[1]], kk) * (scale * LOG2E)
        pos = n - Nq + np.arange(Nq) + (1 if mutant == "diag" else 0)
        keep = np.arange(n)[None, :] <= pos[:, None]
        if mutant == "dropkey":
            keep[:, n // 2] = False
        s = np.where(keep[:, None, :], s, -np.inf)
        v = kb[:, 64:] if mutant == "v64" else kb[:, :DV]
        edges = np.linspace(0, n, parts + 1).astype(int)
        M = np.full((Nq, H), -np.inf)
        L = np.zeros((Nq, H))
        A = np.zeros((Nq, H, DV))
        for j0, j1 in zip(edges[:-1], edges[1:]):
            if j1 == j0:
                continue
            sp = s[..., j0:j1]
            m = sp.max(-1)
            mu = np.where(np.isneginf(m), 0.0, m)
            p = np.exp2(sp - mu[..., None])
            Mn = np.maximum(M, m)
            Mu = np.where(np.isneginf(Mn), 0.0, Mn)
            f_old, f_new = np.exp2(M - Mu), np.exp2(m - Mu)
            L = L * f_old + p.sum(-1) * f_new
            acc = np.einsum("ihj,jd->ihd", p, v[j0:j1])
            A = (A + acc) if mutant == "norescale" else A * f_old[..., None] + acc * f_new[..., None]
            M = Mn
        live = L > 0
        ob = np.where(live[..., None], A / np.where(live, L, 1.0)[..., None], 0.0)
        lb = np.where(live, M + np.log2(np.where(live, L, 1.0)), -np.inf)
        if mutant == "rowmap":
            r = (np.arange(H)[None, :] * Nq + np.arange(Nq)[:, None])                     # the row the wrong map reads for (i, h)
            ob, lb = ob.reshape(Nq * H, DV)[r], lb.reshape(Nq * H)[r]
        o[b], lse[b] = ob, lb.T
    return torch.from_numpy(o).float(), torch.from_numpy(lse).float()


# ---------------------------------------------------------------------------------------------------------------- the C-ABI call
def kv4(kv):
    """the latent cache as the [.., .., 1, 576] tensor whose strides the entry takes"""
    return kv.unsqueeze(2) if kv.dim() == 3 else kv


def tensor_kw(q, kv, o, lse, lens, block_table=None, scale=SCALE):
    B, Nq, H, _ = q.shape
    k = kv4(kv)
    cap, page, pages = (k.shape[1], 0, 0) if block_table is None else (block_table.shape[1], k.shape[1], k.shape[0])
    return dict(dtype=dc.code(q.dtype), q=q.data_ptr(), k=k.data_ptr(), o=o.data_ptr(), lse=lse.data_ptr(), lens=lens.data_ptr(),
                bt=None if block_table is None else block_table.data_ptr(), B=B, H=H, Nq=Nq, D=D, Dv=DV, cap=cap, page=page, pages=pages, qs=dc.s3(q), ks=dc.s3(k),
                os=dc.s3(o), ls=dc.s2(lse), bts=0 if block_table is None else block_table.stride(0), scale=scale)


def nan_out(q):
    B, Nq, H, _ = q.shape
    return (torch.full((B, Nq, H, DV), float("nan"), dtype=q.dtype, device=q.device), torch.full((B, H, Nq), float("nan"), dtype=torch.float32, device=q.device))


def mla_c(q, kv, lens, num_splits, block_table=None, o=None, lse=None, ws=None, scale=SCALE):
    """fa2_fwd_decode_mla with NaN-filled outputs and a NaN-filled workspace sized by the entry's own query: every element the contract names must be
    written, nothing unwritten read.  -> (o, log2 lse)"""
    no, nl = nan_out(q)
    o, lse = no if o is None else o, nl if lse is None else lse
    kw = tensor_kw(q, kv, o, lse, lens, block_table, scale)
    need = _fa2_lib.load().fa2_fwd_decode_mla_workspace_bytes(*[kw[n] for n in ("dtype", "B", "H", "Nq", "D", "Dv", "cap", "page")], num_splits)
    if ws is None:
        ws = torch.full((max(need, 16) // 4,), float("nan"), dtype=torch.float32, device=q.device)
    assert ws.numel() * 4 >= need
    _fa2_lib.check(dc.call("mla", **kw, ns=num_splits, ws=ws.data_ptr() if need else None, wsb=need,
                           stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return o, lse


def paged(kv, lens, page, g, spare=3):
    """The [B, Nmax, 576] cache scattered into NaN-filled pages in shuffled physical order (decode_calls.paged on the one-head view) -> pool, block table"""
    pool, _, bt = dc.paged(kv4(kv), kv4(kv), lens, page, g, spare)
    return pool[:, :, 0], bt
