"""The packed (ragged) KV-cache append on the GPU: fa2_kvcache_append_varlen through kvcache_append_varlen and the k / v / rotary_* keywords of
flash_attention_prefill.

The ragged batch brings (0, 1, 3, 64, 65, 130, 0, 2) new tokens to eight sequences of a 512-key cache.  The lengths AFTER the append make the appends
start in the middle of a 64-key page and cross one (36 .. 99, 63 .. 64) and two page edges (70 .. 199), put a leading token at a negative position
(length 2 for 3 tokens), two trailing tokens behind the capacity (length 514) and one token into the cache's last slot (length 512).  Caches start as
a per-byte pattern; after a call the WHOLE pool is compared byte for byte with the expected image — the pattern with the rows kvappend_refs.append_rows
gives, sequence by sequence, at their targets — so a write outside the targets, into a spare page or behind an unused block-table entry fails, and so
does a skipped token that wrote something.  Unused block-table entries hold ids outside the pool, and so does one entry under live tokens."""
import ctypes

import numpy as np
import pytest
import torch

import decode_calls as dc
import prefill_calls as pc
from kvappend_refs import append_rows, rotary_bar, rotary_ref64
from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention_prefill, kvcache_append, kvcache_append_varlen
from test_kvappend_varlen import HOSTILE

pytestmark = pytest.mark.gpu

F16, BF16, E4M3 = torch.float16, torch.bfloat16, torch.float8_e4m3fn
COUNTS = (0, 1, 3, 64, 65, 130, 0, 2)
LENS = (17, 512, 2, 100, 514, 200, 0, 65)
NMAX = 512
# page size -> ((sequence, page), tokens above it): one block-table entry under live tokens names no page of the pool — sequence 3's positions 64 .. 99,
# or (pages of 128) sequence 5's positions 128 .. 199
BAD_UNDER = {64: ((3, 1), 36), 128: ((5, 1), 72)}
# (H, Hkv, D, dtype, q): R * UR units <= 64, <= 128, 256, and 384 — two blockIdx.y slices
SHAPES = [(8, 8, 128, F16, False), (8, 2, 64, BF16, False), (16, 1, 128, F16, True), (32, 8, 128, BF16, True)]
IDS = ["H%d_Hkv%d_D%d_%s%s" % (s[0], s[1], s[2], "f16" if s[3] == F16 else "bf16", "_q" if s[4] else "") for s in SHAPES]


def _pattern(nbytes, salt=0):
    """a per-byte poison pattern without a short period"""
    i = torch.arange(nbytes, dtype=torch.int64)
    return ((i * 131 + (i >> 8) * 7 + (i >> 16) * 3 + 89 + salt) % 251).to(torch.uint8)


def _pool(shape, dt, salt=0):
    """a cache tensor of `shape` and dtype `dt` (16-bit or e4m3) whose bytes are the pattern"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
    return _pattern(n, salt).view(dt).reshape(shape)


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _cu(counts):
    return [0] + [int(x) for x in np.cumsum(counts)]


def _tokens(total, H, Hkv, D, dt, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return tuple(torch.randn((total, h, D), generator=g).to(dt) for h in (H, Hkv, Hkv))


def _tables(rot, dt, seqlen_ro=NMAX):
    inv = 10000.0 ** (-torch.arange(0, rot, 2, dtype=torch.float64) / rot)
    ang = torch.arange(seqlen_ro, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().to(dt), ang.sin().to(dt)


def _block_table(counts, lens, page, seed, bad_under=None, spare=3):
    """Shuffled physical pages under every page a written token touches, BAD_PAGES everywhere else — and under `bad_under`.  -> table, pool pages"""
    per = NMAX // page
    need = []
    for s, (c, n) in enumerate(zip(counts, lens)):
        for pg in sorted({p // page for p in range(n - c, n) if 0 <= p < NMAX}):
            if (s, pg) != bad_under:
                need.append((s, pg))
    total = len(need) + spare
    order = torch.randperm(total, generator=torch.Generator().manual_seed(seed)).tolist()
    bt = torch.tensor([pc.BAD_PAGES[i % 2] for i in range(len(counts) * per)], dtype=torch.int32).reshape(len(counts), per)
    for (s, pg), pid in zip(need, order):
        bt[s, pg] = pid
    return bt, total


def _expected(kimg, vimg, k, v, q, cu, lens, page=0, bt=None, hkv=None, **modes):
    """The images [B | pages, rows, heads, bytes] (uint8 clones) after the call, and q_out: append_rows per sequence, written at the targets a valid page
    lies under; a token behind cu[B] writes nothing and keeps its q row."""
    kimg, vimg = kimg.clone(), vimg.clone()
    hkv = k.shape[1] if hkv is None else hkv
    q_out = None if q is None else q.clone()
    pages = kimg.shape[0]
    kd, vd = modes.pop("kd", None), modes.pop("vd", None)
    for s in range(len(lens)):
        c0, c1 = cu[s], cu[s + 1]
        if c1 <= c0:
            continue
        rk, rv, rq = append_rows(k[None, c0:c1], v[None, c0:c1], [lens[s]], q=None if q is None else q[None, c0:c1], kd=None if kd is None else kd[s:s + 1],
                                 vd=None if vd is None else vd[s:s + 1], **modes)
        if rq is not None:
            q_out[c0:c1] = rq[0]
        for i in range(c1 - c0):
            p = lens[s] - (c1 - c0) + i
            if not 0 <= p < NMAX:
                continue
            base, r = s, p
            if page:
                base, r = int(bt[s, p // page]), p % page
                if not 0 <= base < pages:
                    continue
            kimg[base, r, :hkv] = _bytes(rk)[0, i]
            vimg[base, r, :hkv] = _bytes(rv)[0, i]
    return kimg, vimg, q_out


def _same(got, want, tag):
    assert torch.equal(got, want), (tag, (got != want).nonzero()[:4].tolist())


LAYOUTS = ["contiguous", "paged64", "paged128", "strided"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_image_ragged(shape, layout):
    dev = dc.dev()
    H, Hkv, D, dt, with_q = shape
    B, cu = len(COUNTS), _cu(COUNTS)
    q, k, v = _tokens(cu[-1], H, Hkv, D, dt, 11 + H)
    page, bt, hk = 0, None, Hkv
    if layout.startswith("paged"):
        page = int(layout[5:])
        bt, total = _block_table(COUNTS, LENS, page, 7 + D, BAD_UNDER[page][0])
        cshape = (total, page, Hkv, D)
    elif layout == "strided":                                  # a padded Nmax stride and a padded head stride
        cshape, hk = (B, NMAX + 48, Hkv + 1, D), Hkv
    else:
        cshape = (B, NMAX, Hkv, D)
    kc, vc = _pool(cshape, dt), _pool(cshape, dt, 5)
    kfull, vfull = kc.to(dev), vc.to(dev)
    kview, vview = (kfull[:, :NMAX, :Hkv], vfull[:, :NMAX, :Hkv]) if layout == "strided" else (kfull, vfull)
    kd_, vd_ = k.to(dev), v.to(dev)
    if layout == "strided":                                    # the new tokens as views with a padded head stride and a padded row stride, too
        wide = torch.zeros((cu[-1] + 3, Hkv + 2, D), dtype=dt, device=dev)
        wide[:cu[-1], :Hkv] = kd_
        kd_ = wide[:cu[-1], :Hkv]
        assert not kd_.is_contiguous() and not kview.is_contiguous()
    modes = {}
    if with_q:
        cos, sin = _tables(D, torch.float32)
        modes = dict(cos=cos, sin=sin, inter=True)
    got_q = kvcache_append_varlen(kview, vview, kd_, vd_, torch.tensor(cu, dtype=torch.int32, device=dev), torch.tensor(LENS, dtype=torch.int32, device=dev),
                                  block_table=None if bt is None else bt.to(dev), rotary_cos=modes["cos"].to(dev) if with_q else None,
                                  rotary_sin=modes["sin"].to(dev) if with_q else None, q=q.to(dev) if with_q else None)
    torch.cuda.synchronize()
    want_k, want_v, want_q = _expected(_bytes(kc), _bytes(vc), k, v, q if with_q else None, cu, LENS, page, bt, hkv=hk, **modes)
    _same(_bytes(kfull.cpu()), want_k, ("k", layout))
    _same(_bytes(vfull.cpu()), want_v, ("v", layout))
    assert not torch.equal(want_k, _bytes(kc)), "something was written"
    written = int((want_v != _bytes(vc)).any(dim=-1).any(dim=-1).sum())
    assert written == (1 + 2 + 64 + 63 + 130 + 2) - (BAD_UNDER[page][1] if page else 0), "the skipped tokens: one leading, two trailing, those above the bad page id"
    if with_q:
        _same(got_q.cpu().view(torch.int16), want_q.view(torch.int16), "q_out")
        assert not torch.equal(want_q, q)
    else:
        assert got_q is None


@pytest.mark.parametrize("nnew", [1, 3, 130])
def test_equals_the_uniform_call(nnew):
    """Equal counts: the cache images and q_out of the packed call are kvcache_append's bit for bit — 16-bit and e4m3 caches, both pairings, f32 and
    16-bit tables, and head dim 96 with rotary_dim 32."""
    dev = dc.dev()
    lens_t = (nnew, 200, 512, 100 if nnew < 100 else 131, 515)
    B = len(lens_t)
    lens = torch.tensor(lens_t, dtype=torch.int32, device=dev)
    cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * nnew
    ran = 0
    for (H, Hkv, D, dt, rot) in ((4, 2, 64, F16, 64), (4, 2, 96, BF16, 32)):
        q, k, v = (t.to(dev) for t in _tokens(B * nnew, H, Hkv, D, dt, 40 + nnew))
        g = torch.Generator().manual_seed(nnew)
        for cdt in ((dt, E4M3) if D % 16 == 0 else (dt,)):
            kd, vd = ((0.02 + 0.03 * torch.rand((B, Hkv), generator=g)).to(dev) for _ in range(2)) if cdt == E4M3 else (None, None)
            for inter in (True, False):
                for tdt in (torch.float32, dt):
                    cos, sin = (t.to(dev) for t in _tables(rot, tdt))
                    ka, va, kb, vb = (_pool((B, NMAX, Hkv, D), cdt, s).to(dev) for s in (0, 5, 0, 5))
                    qa = kvcache_append_varlen(ka, va, k, v, cu, lens, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=inter, k_descale=kd, v_descale=vd, q=q)
                    qb = kvcache_append(kb, vb, k.view(B, nnew, Hkv, D), v.view(B, nnew, Hkv, D), lens, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=inter,
                                        k_descale=kd, v_descale=vd, q=q.view(B, nnew, H, D))
                    torch.cuda.synchronize()
                    tag = (D, str(cdt), inter, str(tdt))
                    _same(_bytes(ka), _bytes(kb), tag + ("k",))
                    _same(_bytes(va), _bytes(vb), tag + ("v",))
                    _same(qa.view(torch.int16), qb.view(B * nnew, H, D).view(torch.int16), tag + ("q",))
                    assert not torch.equal(_bytes(ka).cpu(), _bytes(_pool((B, NMAX, Hkv, D), cdt)))
                    ran += 1
    assert ran == 16


@pytest.mark.parametrize("table", ["f32", "io"])
@pytest.mark.parametrize("inter", [True, False], ids=["gptj", "neox"])
def test_rotary_on_the_ragged_batch(inter, table):
    """Rotated K and q_out: byte for byte the append's own arithmetic (kvappend_refs.rotary_f32, through append_rows), and within rotary_bar of float64."""
    dev = dc.dev()
    H, Hkv, D, dt, rot = 10, 2, 128, BF16 if inter else F16, 64
    B, cu = len(COUNTS), _cu(COUNTS)
    q, k, v = _tokens(cu[-1], H, Hkv, D, dt, 23)
    cos, sin = _tables(rot, torch.float32 if table == "f32" else dt)
    bt, total = _block_table(COUNTS, LENS, 64, 29)
    kc, vc = _pool((total, 64, Hkv, D), dt), _pool((total, 64, Hkv, D), dt, 5)
    kcd, vcd = kc.to(dev), vc.to(dev)
    q_rot = kvcache_append_varlen(kcd, vcd, k.to(dev), v.to(dev), torch.tensor(cu, dtype=torch.int32, device=dev), torch.tensor(LENS, dtype=torch.int32, device=dev),
                                  block_table=bt.to(dev), rotary_cos=cos.to(dev), rotary_sin=sin.to(dev), rotary_interleaved=inter, q=q.to(dev))
    torch.cuda.synchronize()
    want_k, want_v, want_q = _expected(_bytes(kc), _bytes(vc), k, v, q, cu, LENS, 64, bt, cos=cos, sin=sin, inter=inter)
    _same(_bytes(kcd.cpu()), want_k, "k")
    _same(_bytes(vcd.cpu()), want_v, "v")
    _same(q_rot.cpu().view(torch.int16), want_q.view(torch.int16), "q_out")
    # float64: every q row at its position, every written K row read back from its page
    pos = torch.tensor([LENS[s] - COUNTS[s] + i for s in range(B) for i in range(COUNTS[s])])
    rows = pos.clamp(0, cos.shape[0] - 1)
    c64, s64 = cos[rows].double()[:, None, :], sin[rows].double()[:, None, :]
    got_k = kcd.cpu()
    for name, got, x in (("q", q_rot.cpu(), q), ("k", None, k)):
        ref, mag = rotary_ref64(x.double(), c64, s64, rot, inter)
        if name == "k":
            live = ((pos >= 0) & (pos < NMAX)).nonzero().flatten().tolist()
            seq = np.repeat(np.arange(B), COUNTS)
            got = torch.stack([got_k[int(bt[seq[t], int(pos[t]) // 64]), int(pos[t]) % 64] for t in live])
            ref, mag, x = ref[live], mag[live], x[live]
            assert len(live) == cu[-1] - 3
        err = (got.double() - ref).abs()
        bar = rotary_bar(ref, mag, dt)
        print(name, inter, table, "max err / bar %.3g" % float((err / bar).max()))
        assert bool((err <= bar).all()), (name, float((err - bar).max()))
        assert torch.equal(got[..., rot:].view(torch.int16), x[..., rot:].view(torch.int16)), "columns at or beyond rotary_dim"


@pytest.mark.parametrize("layout", ["contiguous", "paged64"])
def test_e4m3_on_the_ragged_batch(layout):
    """Power-of-two descales: the image is torch's CPU cast of y / d after the clamp, bit for bit (rotated K included).  General descales: the dequantised
    code is within half an e4m3 step of the float64 quotient, (2^-4 + 2^-20) |exact| + d 2^-10, as tests/test_kvappend_gpu.py holds the uniform call."""
    dev = dc.dev()
    H, Hkv, D, dt = 16, 2, 128, BF16
    B, cu = len(COUNTS), _cu(COUNTS)
    q, k, v = _tokens(cu[-1], H, Hkv, D, dt, 31)
    cos, sin = _tables(D, torch.float32)
    page, bt, cshape = 0, None, (B, NMAX, Hkv, D)
    if layout == "paged64":
        page = 64
        bt, total = _block_table(COUNTS, LENS, 64, 33, BAD_UNDER[64][0])
        cshape = (total, 64, Hkv, D)
    g = torch.Generator().manual_seed(34)
    cud, lens = torch.tensor(cu, dtype=torch.int32, device=dev), torch.tensor(LENS, dtype=torch.int32, device=dev)
    btd = None if bt is None else bt.to(dev)
    kd, vd = (2.0 ** -torch.randint(5, 8, (B, Hkv), generator=g).float() for _ in range(2))
    kc, vc = _pool(cshape, E4M3), _pool(cshape, E4M3, 5)
    kcd, vcd = kc.to(dev), vc.to(dev)
    kvcache_append_varlen(kcd, vcd, k.to(dev), v.to(dev), cud, lens, block_table=btd, rotary_cos=cos.to(dev), rotary_sin=sin.to(dev), rotary_interleaved=False,
                          k_descale=kd.to(dev), v_descale=vd.to(dev))
    torch.cuda.synchronize()
    want_k, want_v, _ = _expected(_bytes(kc), _bytes(vc), k, v, None, cu, LENS, page, bt, cos=cos, sin=sin, inter=False, fp8=True, kd=kd, vd=vd)
    _same(_bytes(kcd.cpu()), want_k, "k")
    _same(_bytes(vcd.cpu()), want_v, "v")
    # general descales
    kd, vd = (0.02 + 0.03 * torch.rand((B, Hkv), generator=g) for _ in range(2))
    kcd, vcd = kc.to(dev), vc.to(dev)
    kvcache_append_varlen(kcd, vcd, k.to(dev), v.to(dev), cud, lens, block_table=btd, rotary_cos=cos.to(dev), rotary_sin=sin.to(dev), rotary_interleaved=False,
                          k_descale=kd.to(dev), v_descale=vd.to(dev))
    torch.cuda.synchronize()
    seq = np.repeat(np.arange(B), COUNTS)
    pos = torch.tensor([LENS[s] - COUNTS[s] + i for s in range(B) for i in range(COUNTS[s])])
    live = [t for t in range(cu[-1]) if 0 <= int(pos[t]) < NMAX and (not page or 0 <= int(bt[seq[t], int(pos[t]) // 64]) < cshape[0])]
    assert len(live) == cu[-1] - 3 - (36 if page else 0)
    exact_k, _ = rotary_ref64(k.double(), cos[pos.clamp(0, NMAX - 1)].double()[:, None, :], sin[pos.clamp(0, NMAX - 1)].double()[:, None, :], D, False)
    for name, cache, exact, d in (("k", kcd.cpu(), exact_k, kd), ("v", vcd.cpu(), v.double(), vd)):
        got = torch.stack([cache.view(torch.uint8)[int(bt[seq[t], int(pos[t]) // 64]) if page else seq[t], int(pos[t]) % 64 if page else int(pos[t])] for t in live])
        dd = d[seq[live]].double()[:, :, None]
        ex = exact[live]
        assert float((ex / dd).abs().max()) < 448.0
        err = (got.view(E4M3).double() * dd - ex).abs()
        bar = (2.0 ** -4 + 2.0 ** -20) * ex.abs() + dd * 2.0 ** -10
        print(name, layout, "max err / bar %.3g" % float((err / bar).max()))
        assert bool((err <= bar).all()), (name, float((err - bar).max()))


def test_a_partly_filled_token_buffer():
    """cu[B] < total: the tail tokens write nothing, their q_out rows are q's bit for bit, and the images are those of the call on the truncated tensors."""
    dev = dc.dev()
    H, Hkv, D, dt, tail = 8, 2, 64, F16, 37
    B, cu = len(COUNTS), _cu(COUNTS)
    q, k, v = _tokens(cu[-1] + tail, H, Hkv, D, dt, 51)
    cos, sin = (t.to(dev) for t in _tables(D, torch.float32))
    bt, total = _block_table(COUNTS, LENS, 64, 52)
    cud, lens, btd = torch.tensor(cu, dtype=torch.int32, device=dev), torch.tensor(LENS, dtype=torch.int32, device=dev), bt.to(dev)
    ka, va, kb, vb = (_pool((total, 64, Hkv, D), dt, s).to(dev) for s in (0, 5, 0, 5))
    qa = kvcache_append_varlen(ka, va, k.to(dev), v.to(dev), cud, lens, block_table=btd, rotary_cos=cos, rotary_sin=sin, q=q.to(dev))
    qb = kvcache_append_varlen(kb, vb, k[:cu[-1]].to(dev), v[:cu[-1]].to(dev), cud, lens, block_table=btd, rotary_cos=cos, rotary_sin=sin, q=q[:cu[-1]].to(dev))
    torch.cuda.synchronize()
    _same(_bytes(ka), _bytes(kb), "k")
    _same(_bytes(va), _bytes(vb), "v")
    _same(qa[:cu[-1]].view(torch.int16), qb.view(torch.int16), "q_out of the owned tokens")
    _same(qa[cu[-1]:].cpu().view(torch.int16), q[cu[-1]:].view(torch.int16), "q_out of the tail")
    assert not torch.equal(qa[:cu[-1]].cpu(), q[:cu[-1]]) and not torch.equal(_bytes(ka).cpu(), _bytes(_pool((total, 64, Hkv, D), dt)))
    # ... and a buffer that starts late: tokens in front of cu[0] belong to no sequence either
    late = torch.tensor([c + 5 for c in cu], dtype=torch.int32, device=dev)
    kc2, vc2 = (_pool((total, 64, Hkv, D), dt, s).to(dev) for s in (0, 5))
    qc = kvcache_append_varlen(kc2, vc2, k[:cu[-1] + 5].to(dev).roll(5, 0), v[:cu[-1] + 5].to(dev).roll(5, 0), late, lens, block_table=btd, rotary_cos=cos,
                               rotary_sin=sin, q=q[:cu[-1] + 5].to(dev).roll(5, 0))
    torch.cuda.synchronize()
    _same(_bytes(kc2), _bytes(kb), "k, late start")
    _same(qc[5:].view(torch.int16), qb.view(torch.int16), "q_out, late start")
    _same(qc[:5].cpu().view(torch.int16), q[cu[-1]:cu[-1] + 5].view(torch.int16), "q_out in front of cu[0]")


@pytest.mark.parametrize("which", range(len(HOSTILE)))
def test_hostile_cu_seqlens_stay_inside_the_predicted_rows(which):
    """cu_seqlens that are no ascending offsets (the fixed arrays of tests/test_kvappend_varlen.py).  Caches and q_out are views inside one patterned
    allocation with margins on both sides; after the call every byte outside the rows the host side of the kernel's two index functions predicts —
    fa2_kvappend_varlen_token, then fa2_kvappend_slot — is unchanged.  Every predicted address lies inside the views (asserted before the launch)."""
    dev = dc.dev()
    cu = HOSTILE[which]
    B, total, H, Hkv, D, dt, cap = len(cu) - 1, 24, 4, 2, 64, F16, 64
    lens_t = (30, 40, 50, 64)
    q, k, v = _tokens(total, H, Hkv, D, dt, 70 + which)
    cos, sin = _tables(D, torch.float32, cap)
    margin = 1 << 16
    nk, nq = B * cap * Hkv * D * 2, total * H * D * 2
    big = _pattern(4 * margin + 2 * nk + nq, which).to(dev)
    at_k, at_v, at_q = margin, 2 * margin + nk, 3 * margin + 2 * nk
    kc, vc = (big[a:a + nk].view(dt).view(B, cap, Hkv, D) for a in (at_k, at_v))
    qo = big[at_q:at_q + nq].view(dt).view(total, H, D)
    before = big.cpu()
    # the prediction
    keep = torch.ones(before.numel(), dtype=torch.bool)
    keep[at_q:at_q + nq] = False                              # every q_out row is written: rotated, or copied through
    plain, writes = [], 0
    for t in range(total):
        tok = _fa2_lib.kvappend_varlen_token(cu, t)
        if tok is None:
            plain.append(t)
            continue
        s, i, n = tok
        assert 0 <= s < B and 0 <= i < n
        p = _fa2_lib.kvappend_slot(lens_t[s], cap, n, i)
        if p >= 0:
            assert p < cap
            for a in (at_k, at_v):
                keep[a + (s * cap + p) * Hkv * D * 2:a + (s * cap + p + 1) * Hkv * D * 2] = False
            writes += 1
    kd_, vd_, qd, cosd, sind = (x.to(dev) for x in (k, v, q, cos, sin))
    cud, lens = torch.tensor(cu, dtype=torch.int32, device=dev), torch.tensor(lens_t, dtype=torch.int32, device=dev)
    rc = dc.call("append_varlen", dtype=dc.code(dt), fmt=_fa2_lib.FA2_CACHE_16BIT, kn=kd_.data_ptr(), vn=vd_.data_ptr(), k=kc.data_ptr(), v=vc.data_ptr(),
                 cu=cud.data_ptr(), lens=lens.data_ptr(), bt=None, B=B, total=total, Hkv=Hkv, D=D, cap=cap, page=0, pages=0, kns=pc.s2(kd_), vns=pc.s2(vd_),
                 ks=dc.s3(kc), vs=dc.s3(vc), bts=0, q=qd.data_ptr(), qo=qo.data_ptr(), H=H, qs=pc.s2(qd), qos=pc.s2(qo), cos=cosd.data_ptr(), sin=sind.data_ptr(),
                 rdt=_fa2_lib.FA2_DTYPE_F32, rot=D, sro=cap, ros=cos.stride(0), inter=1, kd=None, vd=None, ds=None,
                 stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _fa2_lib.check(rc)
    torch.cuda.synchronize()
    after = big.cpu()
    _same(after[keep], before[keep], ("outside the predicted rows", cu))
    got_q = after[at_q:at_q + nq].view(dt).view(total, H, D)
    if plain:
        _same(got_q[plain].view(torch.int16), q[plain].view(torch.int16), "q rows of tokens without a sequence")
    print(cu, "tokens without a sequence:", len(plain), "written K / V rows:", writes)


# ---------------------------------------------------------------------------------------------------------------- fused prefill
PF_NQ = (0, 1, 3, 64, 65, 130, 0, 2)
PF_LENS = (17, 200, 3, 100, 129, 130, 0, 65)


def _prefill_case(H, Hkv, D, dt, dev):
    """History keys in the cache (NaN where the new tokens go and beyond), the new tokens, tables; and the float64-rotated inputs of the reference."""
    g = torch.Generator().manual_seed(1000 * H + D)
    cu = _cu(PF_NQ)
    q, k, v = _tokens(cu[-1], H, Hkv, D, dt, 77 + D)
    cos, sin = _tables(D, torch.float32, 256)
    hist_k = [torch.randn((n - c, Hkv, D), generator=g).to(dt) for n, c in zip(PF_LENS, PF_NQ)]
    hist_v = [torch.randn((n - c, Hkv, D), generator=g).to(dt) for n, c in zip(PF_LENS, PF_NQ)]
    nan = lambda c: torch.full((c, Hkv, D), float("nan"), dtype=dt)          # noqa: E731
    pre_k = [torch.cat([h, nan(c)]).to(dev) for h, c in zip(hist_k, PF_NQ)]
    pre_v = [torch.cat([h, nan(c)]).to(dev) for h, c in zip(hist_v, PF_NQ)]
    pos = torch.tensor([PF_LENS[s] - PF_NQ[s] + i for s in range(len(PF_NQ)) for i in range(PF_NQ[s])])
    c64, s64 = cos[pos].double()[:, None, :], sin[pos].double()[:, None, :]
    q64 = rotary_ref64(q.double(), c64, s64, D, False)[0].to(dt).to(dev)      # rotated in float64, rounded once to the I/O dtype: what the cache holds
    k64 = rotary_ref64(k.double(), c64, s64, D, False)[0].to(dt)
    ref_k = [torch.cat([h, k64[cu[s]:cu[s + 1]]]).to(dev) for s, h in enumerate(hist_k)]
    ref_v = [torch.cat([h, v[cu[s]:cu[s + 1]]]).to(dev) for s, h in enumerate(hist_v)]
    return cu, q, k, v, cos, sin, pre_k, pre_v, q64, ref_k, ref_v


@pytest.mark.parametrize("layout", ["contiguous", "paged64"])
@pytest.mark.parametrize("shape", [(8, 2, 64, BF16), (8, 8, 128, F16)], ids=["H8_Hkv2_D64_bf16", "H8_Hkv8_D128_f16"])
def test_fused_prefill_equals_append_then_prefill(shape, layout):
    """flash_attention_prefill(k=, v=, rotary_*) against kvcache_append_varlen followed by flash_attention_prefill on the rotated q: o, lse and both
    caches bit for bit; and o, lse against tests/prefill_calls.py's float64 reference on inputs rotated in float64 (rounded once to the I/O dtype, as
    an exact rotation would store them: where the f32 rotation rounds the other way — about one element in 2^13 — one input moves by one unit in the
    last place, a fraction of the bar's own slack)."""
    dev = dc.dev()
    H, Hkv, D, dt = shape
    cu, q, k, v, cos, sin, pre_k, pre_v, q64, ref_k, ref_v = _prefill_case(H, Hkv, D, dt, dev)
    B = len(PF_NQ)
    if layout == "paged64":
        kc, vc, bt = pc.paged_cache(pre_k, pre_v, 64, 4, 5)
    else:
        (kc, vc), bt = pc.contiguous_cache(pre_k, pre_v, 256), None
    cud, lens = torch.tensor(cu, dtype=torch.int32, device=dev), torch.tensor(PF_LENS, dtype=torch.int32, device=dev)
    qd, kn, vn, cosd, sind = (t.to(dev) for t in (q, k, v, cos, sin))
    ka, va, kb, vb = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    o, lse = flash_attention_prefill(qd, ka, va, cud, lens, bt, max_seqlen_q=max(PF_NQ), return_lse=True, k=kn, v=vn, rotary_cos=cosd, rotary_sin=sind,
                                     rotary_interleaved=False)
    q_rot = kvcache_append_varlen(kb, vb, kn, vn, cud, lens, bt, rotary_cos=cosd, rotary_sin=sind, rotary_interleaved=False, q=qd)
    o2, lse2 = flash_attention_prefill(q_rot, kb, vb, cud, lens, bt, max_seqlen_q=max(PF_NQ), return_lse=True)
    torch.cuda.synchronize()
    assert pc.bits_equal(ka, kb) and pc.bits_equal(va, vb) and not pc.bits_equal(ka, kc), "the caches"
    assert pc.bits_equal(o, o2) and pc.bits_equal(lse, lse2)
    assert not bool(torch.isnan(o.float()).any()), "every new token's K / V was written before it was read"
    ref = pc.reference(q64, cud, ref_k, ref_v, D ** -0.5)
    fails = pc.check_float64((shape[:3], layout), o, lse * pc.LOG2E, ref)
    assert not fails, fails
    # without tables: the append alone, q untouched
    o3 = flash_attention_prefill(q_rot, kc.clone(), vc.clone(), cud, lens, bt, max_seqlen_q=max(PF_NQ), k=kb_rows(kb, bt, cu, layout), v=vn)
    assert pc.bits_equal(o3, o)


def kb_rows(kb, bt, cu, layout):
    """the rotated new K rows read back from a cache the append wrote: [total, Hkv, D]"""
    rows = []
    for s, (n, c) in enumerate(zip(PF_LENS, PF_NQ)):
        for p in range(n - c, n):
            rows.append(kb[int(bt[s, p // 64]), p % 64] if layout == "paged64" else kb[s, p])
    return torch.stack(rows)


def test_graph_replay_of_a_ragged_serving_step():
    """increment-lengths + fused prefill captured once with a fixed 64-token buffer and max_seqlen_q = 64, replayed for three steps while cu_seqlens_q,
    cache_seqlens and the block table change in place: step 2 fills the buffer only partly, step 3 starts a new sequence in slot 1 on the old one's
    pages, recycled in another order and not cleared.  Each step's o (the owned rows) and the final cache image equal the eager calls' on a twin."""
    dev = dc.dev()
    H, Hkv, D, dt, page, per, B, T = 8, 2, 64, BF16, 64, 4, 3, 64
    g = torch.Generator().manual_seed(91)
    pool_k, pool_v = (torch.randn((B * per + 2, page, Hkv, D), generator=g).to(dt) for _ in range(2))
    order = torch.randperm(B * per + 2, generator=g)[:B * per].to(torch.int32).reshape(B, per)
    cos, sin = (t.to(dev) for t in _tables(D, torch.float32, 256))
    start = (5, 60, 0)
    steps = []
    for nq in ((20, 12, 32), (1, 30, 0), (5, 1, 58)):
        q, k, v = _tokens(T, H, Hkv, D, dt, 300 + nq[0])
        steps.append((torch.tensor(nq, dtype=torch.int32), torch.tensor(_cu(nq), dtype=torch.int32), q.to(dev), k.to(dev), v.to(dev)))

    def mutate(s, lens, bt):
        if s == 2:                                             # slot 1: a new sequence on the finished one's pages, in another order
            lens[1] = 0
            bt[1] = bt[1].flip(0)

    def step(q, k, v, cu, inc, lens, bt, kc, vc):
        lens.add_(inc)
        return flash_attention_prefill(q, kc, vc, cu, lens, bt, max_seqlen_q=T, k=k, v=v, rotary_cos=cos, rotary_sin=sin)

    tk, tv, tl, tb = pool_k.to(dev), pool_v.to(dev), torch.tensor(start, dtype=torch.int32, device=dev), order.to(dev)
    want = []
    for s, (nq, cu, q, k, v) in enumerate(steps):
        mutate(s, tl, tb)
        want.append(step(q, k, v, cu.to(dev), nq.to(dev), tl, tb, tk, tv).clone())
    ck, cv, lens, bt = pool_k.to(dev), pool_v.to(dev), torch.tensor(start, dtype=torch.int32, device=dev), order.to(dev)
    nq0, cu0, q0, k0, v0 = steps[0]
    qi, ki, vi, cui, inci = q0.clone(), k0.clone(), v0.clone(), cu0.to(dev), nq0.to(dev)
    sk, sv, sl = ck.clone(), cv.clone(), lens.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up outside the capture, on caches and lengths of its own
        step(qi, ki, vi, cui, inci, sl, bt, sk, sv)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            go = step(qi, ki, vi, cui, inci, lens, bt, ck, cv)
    torch.cuda.current_stream().wait_stream(side)
    for s, (nq, cu, q, k, v) in enumerate(steps):
        mutate(s, lens, bt)
        for dst, src in ((qi, q), (ki, k), (vi, v), (cui, cu.to(dev)), (inci, nq.to(dev))):
            dst.copy_(src)
        go.zero_()
        graph.replay()
        torch.cuda.synchronize()
        n = int(cu[-1])
        assert n == (64, 31, 64)[s]
        assert pc.bits_equal(go[:n], want[s][:n]), s
        assert not bool(torch.isnan(go[:n].float()).any())
    assert pc.bits_equal(ck, tk) and pc.bits_equal(cv, tv) and torch.equal(lens, tl) and torch.equal(bt, tb)
    assert not pc.bits_equal(ck, pool_k.to(dev)) and not pc.bits_equal(want[0][:31], want[1][:31])
