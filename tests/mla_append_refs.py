"""The expected byte images of the latent-cache (MLA) append tests (tests/test_kvappend_mla.py, tests/test_kvappend_mla_gpu.py): what
fa2_kvcache_append_mla / fa2_kvcache_append_mla_varlen leave in the cache and in q_out, built on the CPU from the contract alone.

Every stored element is a source element bit for bit or ONE rounding of kvappend_refs.rotary_f32 (the append's f32 arithmetic, held to
fa2_rotary_eval's bits in tests/test_kvappend.py and, on the 64-wide tail, in tests/test_kvappend_mla.py), so the tests compare int16 images: the
WHOLE cache and the WHOLE q_out, which both start from POISON.  Plain CPU code; nothing here touches a device."""
import torch

import kvappend_refs as kr
import mla_refs as mr

D, DV = mr.D, mr.DV
ROT = D - DV
POISON = 0x5A5B                     # a finite value in both formats that no test input holds


def bits(t):
    return t.contiguous().view(torch.int16)


def poisoned(shape, dtype):
    return torch.full(shape, POISON, dtype=torch.int16).view(dtype)


def tables(seqlen_ro, dtype=torch.float32, seed=3):
    """cos / sin [seqlen_ro, 32] of angles far from the identity, in `dtype` (f32 or a 16-bit format: rounded once, here)"""
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(seqlen_ro, ROT // 2, generator=g, dtype=torch.float64) * 200.0
    return ang.cos().float().to(dtype), ang.sin().float().to(dtype)


def inputs(tokens, H, dtype, seed, tiny=True):
    """N(0, 1) kv_c [tokens, 512], k_pe [tokens, 64] and q [tokens, H, 576] (None for H = 0) in `dtype`; a few subnormals and zeros among them"""
    g = torch.Generator().manual_seed(seed)
    kv_c = torch.randn(tokens, DV, generator=g).to(dtype)
    k_pe = (torch.randn(tokens, ROT, generator=g) * 3.0).to(dtype)
    q = torch.randn(tokens, H, D, generator=g).to(dtype) if H else None
    if tiny and tokens:
        k_pe[0, 0::7] = 1e-40 if dtype == torch.bfloat16 else 3e-7       # subnormal in the format
        k_pe[0, 1::7] = 0.0
        if q is not None:
            q[0, 0, DV::5] = -(1e-40 if dtype == torch.bfloat16 else 3e-7)
    return kv_c, k_pe, q


def rotated_tail(x, rows, cos, sin, inter):
    """x [T, ..., 64] (16-bit) rotated by table rows `rows` [T] (clamped already): rotary_f32, rounded once to x's dtype"""
    c, s = cos[rows], sin[rows]
    while c.dim() < x.dim():
        c, s = c.unsqueeze(1), s.unsqueeze(1)
    return kr.rotary_f32(x, c, s, ROT, inter).to(x.dtype)


def uniform_owners(B, nnew):
    return [(b, i, nnew) for b in range(B) for i in range(nnew)]


def expect(cache, kv_c, k_pe, owners, lens, block_table=None, q=None, cos=None, sin=None, inter=True):
    """The image after the append and q_out.  cache [B | pages, rows, 576]: the image before (CPU; a strided view is fine); kv_c [T, 512], k_pe [T, 64],
    q [T, H, 576] or None: the tokens, flat; owners[t] = (s, i, nnew) — token t is new token i of sequence s's nnew — or None: no sequence owns it;
    lens [B]: the lengths AFTER the append, any ints.  -> (cache image, q_out or None), new tensors."""
    img = cache.clone()
    q_out = None if q is None else q.clone()                    # columns 0 .. 511, and the rows no sequence owns: bit for bit
    T = len(owners)
    assert kv_c.shape[0] == k_pe.shape[0] == T
    pos = [None if o is None else int(lens[o[0]]) - o[2] + o[1] for o in owners]
    tail = k_pe.clone()
    if cos is not None:
        own = [t for t in range(T) if owners[t] is not None]
        if own:
            rows = torch.tensor([min(max(pos[t], 0), cos.shape[0] - 1) for t in own])
            idx = torch.tensor(own)
            tail[idx] = rotated_tail(k_pe[idx], rows, cos, sin, inter)
            if q is not None:
                q_out[idx, :, DV:] = rotated_tail(q[idx][:, :, DV:], rows, cos, sin, inter)
    paged = block_table is not None
    page = cache.shape[1]
    cap_keys = block_table.shape[1] * page if paged else cache.shape[1]
    for t, o in enumerate(owners):
        if o is None or not 0 <= pos[t] < cap_keys:
            continue                                            # skipped: nothing is written
        if paged:
            pid = int(block_table[o[0], pos[t] // page])
            if not 0 <= pid < cache.shape[0]:
                continue                                        # a page id outside the pool: skipped, never clamped
            row = img[pid, pos[t] % page]
        else:
            row = img[o[0], pos[t]]
        row[:DV] = kv_c[t]
        row[DV:] = tail[t]
    return img, q_out
