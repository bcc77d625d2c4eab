"""The call layer of the prefill tests (tests/test_prefill.py, test_prefill_gpu.py, test_prefill_far_gpu.py): fa2_fwd_prefill and its packed twins
through ctypes on NaN-filled outputs, the builders of contiguous and paged caches that hold NaN wherever no valid key lies, the gather of a cache into the
packed copy the twins take, and the float64 reference with tools/key_bars.py's bars.  A plain module: nothing here touches a device until asked."""
import ctypes
import os
import sys

import torch

from conftest import LSE_TOL, ROOT
from rocwmma_fattn import _fa2_lib

if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.append(os.path.join(ROOT, "tools"))
import decode_abi  # noqa: E402
import key_bars  # noqa: E402

LOG2E = 1.4426950408889634
FLAGS_TWIN = _fa2_lib.FA2_FLAG_CAUSAL | _fa2_lib.FA2_FLAG_BOTTOM_RIGHT
BAD_PAGES = (-1, 2 ** 30)            # what unused block-table entries hold


def code(dtype):
    return _fa2_lib.FA2_DTYPE_F16 if dtype == torch.float16 else _fa2_lib.FA2_DTYPE_BF16


def ptr(t):
    return None if t is None else t.data_ptr()


def s3(t):
    """{page | batch, head, row} element strides of a [pages, rows, heads, D] cache."""
    return _fa2_lib.strides3(t.stride(0), t.stride(2), t.stride(1))


def s2(t):
    return _fa2_lib.strides2(t.stride(1), t.stride(0))


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def nan_out(q):
    o = torch.full_like(q, float("nan"))
    lse = torch.full((q.shape[1], q.shape[0]), float("nan"), dtype=torch.float32, device=q.device)
    return o, lse


def prefill_kw(q, kc, vc, o, lse, cu, lens, bt, max_q, scale, window_left=-1, softcap=0.0, slopes=None):
    """What the tensors of a prefill call say, by decode_abi's keywords (16-bit or e4m3 caches; the descales are the caller's to add)."""
    paged = bt is not None
    return dict(dtype=code(q.dtype), fmt=_fa2_lib.FA2_CACHE_16BIT if kc.element_size() == 2 else _fa2_lib.FA2_CACHE_E4M3, q=ptr(q), k=ptr(kc), v=ptr(vc), o=ptr(o),
                lse=ptr(lse), cu=ptr(cu), lens=ptr(lens), bt=ptr(bt), B=lens.numel(), H=q.shape[1], Hkv=kc.shape[2], max_q=int(max_q), D=q.shape[2],
                cap=bt.shape[1] if paged else kc.shape[1], page=kc.shape[1] if paged else 0, pages=kc.shape[0] if paged else 0, qs=s2(q), ks=s3(kc), vs=s3(vc),
                os=s2(o), lss=lse.stride(0), bts=bt.stride(0) if paged else 0, scale=float(scale), wl=int(window_left), cap_=float(softcap), sl=ptr(slopes),
                st=0 if slopes is None or slopes.dim() == 1 else slopes.stride(0), stream=stream())


def prefill_c(q, kc, vc, cu, lens, bt, max_q, scale, window_left=-1, softcap=0.0, slopes=None, out=None, check=True):
    """fa2_fwd_prefill on NaN-filled o / lse (or `out`) -> o [total_q, H, D], lse f32 [H, total_q] in log2 units."""
    o, lse = out if out is not None else nan_out(q)
    rc = decode_abi.call("prefill", **prefill_kw(q, kc, vc, o, lse, cu, lens, bt, max_q, scale, window_left, softcap, slopes))
    if check:
        _fa2_lib.check(rc)
        return o, lse
    return rc


def varlen_c(q, kp, vp, cu_q, cu_k, max_q, max_k, scale, window_left=-1, softcap=0.0, slopes=None):
    """The packed twin: fa2_fwd_varlen (fa2_fwd_varlen_scoremod with a cap or slopes), causal, bottom-right, the same window."""
    o, lse = nan_out(q)
    lib = _fa2_lib.load()
    args = (code(q.dtype), ptr(q), ptr(kp), ptr(vp), ptr(o), ptr(lse), cu_q.numel() - 1, q.shape[1], kp.shape[1], max(int(max_q), 1), max(int(max_k), 1),
            q.shape[2], ptr(cu_q), ptr(cu_k), s2(q), s2(kp), s2(vp), s2(o), lse.stride(0), float(scale), FLAGS_TWIN, int(window_left), -1, stream())
    if softcap > 0 or slopes is not None:
        rc = lib.fa2_fwd_varlen_scoremod(*args, float(softcap), ptr(slopes), 0 if slopes is None or slopes.dim() == 1 else slopes.stride(0))
    else:
        rc = lib.fa2_fwd_varlen(*args)
    _fa2_lib.check(rc)
    return o, lse


def bits_equal(a, b):
    """Bit for bit, NaN patterns included."""
    ia = a.view(torch.int16 if a.element_size() == 2 else torch.int32)
    ib = b.view(torch.int16 if b.element_size() == 2 else torch.int32)
    return a.shape == b.shape and bool(torch.equal(ia, ib))


# ---------------------------------------------------------------------------------------------------------------- caches
def make_inputs(lens, nqs, H, Hkv, D, dtype, seed, device):
    """q [total_q, H, D], cu_seqlens_q, and per-sequence keys / values [len_s, Hkv, D] (lists), all on the device."""
    g = torch.Generator().manual_seed(seed)
    total = sum(nqs)
    q = torch.randn((max(total, 1), H, D), generator=g).to(dtype)[:total].to(device)
    ks = [torch.randn((n, Hkv, D), generator=g).to(dtype).to(device) for n in lens]
    vs = [torch.randn((n, Hkv, D), generator=g).to(dtype).to(device) for n in lens]
    cu = torch.tensor([0] + list(torch.tensor(nqs).cumsum(0).tolist()), dtype=torch.int32, device=device)
    return q, cu, ks, vs


def contiguous_cache(ks, vs, nmax):
    """[B, nmax, Hkv, D] caches, NaN at and beyond every length."""
    outs = []
    for seqs in (ks, vs):
        c = torch.full((len(seqs), nmax) + tuple(seqs[0].shape[1:]), float("nan"), dtype=seqs[0].dtype, device=seqs[0].device)
        for b, t in enumerate(seqs):
            c[b, :t.shape[0]] = t
        outs.append(c)
    return outs


def paged_cache(ks, vs, page, per, seed, spare=3, share=None, visible=None):
    """A shuffled pool [num_pages, page, Hkv, D]: NaN at and beyond every length, in spare pages, and (visible(b, j) False) in pages no row sees, whose
    block-table entries — like the entries past a sequence's pages — hold BAD_PAGES in turn.  share = (a, b): sequences a and b, whose first page of
    keys must be equal, share that physical page.  -> pool K, pool V, block table int32 [B, per] (all on the keys' device)"""
    g = torch.Generator().manual_seed(seed)
    used = [-(-t.shape[0] // page) for t in ks]
    total = sum(used) + spare
    order = torch.randperm(total, generator=g).tolist()
    bt = torch.empty((len(ks), per), dtype=torch.int32)
    bt.view(-1)[:] = torch.tensor([BAD_PAGES[i % 2] for i in range(bt.numel())], dtype=torch.int32)
    dev = ks[0].device
    pools = [torch.full((total, page) + tuple(ks[0].shape[1:]), float("nan"), dtype=ks[0].dtype, device=dev) for _ in range(2)]
    nxt = 0
    for b, u in enumerate(used):
        for j in range(u):
            pid = order[nxt]
            nxt += 1
            if visible is not None and not visible(b, j):
                continue
            if share is not None and b == share[1] and j == 0:
                pid = int(bt[share[0], 0])
            bt[b, j] = pid
            for pool, seqs in zip(pools, (ks, vs)):
                rows = seqs[b][j * page:(j + 1) * page]
                pool[pid, :rows.shape[0]] = rows
    return pools[0], pools[1], bt.to(dev)


def packed_copy(ks, vs):
    """The keys gathered into the packed copy of the twins -> K, V [total_k, Hkv, D], cu_seqlens_k."""
    dev = ks[0].device
    cu = torch.tensor([0] + list(torch.tensor([t.shape[0] for t in ks]).cumsum(0).tolist()), dtype=torch.int32, device=dev)
    pad = ks[0].new_zeros((8,) + tuple(ks[0].shape[1:]))           # (never addressed: the twins want a non-null buffer when every sequence is empty)
    return torch.cat(list(ks) + [pad]), torch.cat(list(vs) + [pad]), cu


# ---------------------------------------------------------------------------------------------------------------- float64
def reference(q, cu, ks, vs, scale, window_left=-1, softcap=0.0, slopes=None):
    """float64 per sequence (tools/key_bars.py: dense64) -> o [total_q, H, D], log2 lse [H, total_q], the per-element O bar."""
    total, H, D = q.shape
    o = torch.zeros((total, H, D), dtype=torch.float64, device=q.device)
    bar = torch.zeros_like(o)
    lse = torch.full((H, total), float("-inf"), dtype=torch.float64, device=q.device)
    cul = cu.tolist()
    for s, (k, v) in enumerate(zip(ks, vs)):
        q0, q1 = cul[s], cul[s + 1]
        nq, nk = q1 - q0, k.shape[0]
        if nq == 0 or nk == 0:
            continue
        g = H // k.shape[1]
        pos = torch.arange(nq, device=q.device)[:, None] + (nk - nq)
        j = torch.arange(nk, device=q.device)[None, :]
        keep = (j <= pos) & ((j >= pos - window_left) if window_left >= 0 else torch.ones_like(j, dtype=torch.bool))
        bias = None
        if slopes is not None:
            sl = (slopes if slopes.dim() == 1 else slopes[s]).double()
            bias = -sl[None, :, None, None] * (pos - j).abs().double()[None, None]
        ref = key_bars.dense64(q[q0:q1].transpose(0, 1)[None], k.transpose(0, 1).repeat_interleave(g, 0)[None], v.transpose(0, 1).repeat_interleave(g, 0)[None],
                               scale, keep=keep[None, None], bias=bias, softcap=softcap)
        o[q0:q1] = ref["o"][0].transpose(0, 1)
        bar[q0:q1] = key_bars.o_bar(ref, q.dtype)[0].transpose(0, 1)
        lse[:, q0:q1] = ref["lse"][0]
    return o, lse, bar


def check_float64(tag, o, lse, ref):
    """-> failures of (o, log2 lse) against reference()'s triple: the per-element O bar, LSE_TOL on live rows, -inf exactly on dead ones."""
    ro, rl, bar = ref
    fails = []
    if not torch.isfinite(o.double()).all():
        return ["%s: O non-finite" % tag]
    worst = key_bars.ratio_max((o.double() - ro).abs(), bar)
    if not worst <= 1.0:
        fails.append("%s: O at %.2f bars" % (tag, worst))
    dead = torch.isinf(rl)
    if not torch.equal(torch.isinf(lse) & (lse < 0), dead):
        fails.append("%s: dead rows differ" % tag)
    lerr = float((lse.double() - rl)[~dead].abs().max()) if bool((~dead).any()) else 0.0
    if not lerr <= LSE_TOL:
        fails.append("%s: LSE off by %.3e" % (tag, lerr))
    return fails
