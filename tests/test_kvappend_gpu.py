"""KV-cache append with rotary embedding and e4m3 quantisation on the GPU: fa2_kvcache_append through kvcache_append and the k / v / rotary_* keywords of
flash_attention_decode.

The batch is tests/test_decode_gpu.py's nine lengths, here the lengths AFTER the append: with Nnew in {1, 3, 4} (the shapes' Nq) that gives tokens at
negative positions (lengths 0, 1, 2), appends that straddle a 64-key page (65, 129) and a page's last slot (64).  Caches start as a per-byte poison
pattern; after a call the WHOLE pool is compared byte for byte with the expected image (the pattern with the targeted rows replaced), so a write
outside the targets, into a spare page or behind an unused block-table entry fails the test, and so does a skipped token that wrote something.
Rotated values are held to float64 under the bar of tests/test_kvappend.py (one rounding of an f32 value); e4m3 codes to torch's CPU cast after the
clamp, which is round-to-nearest-even with +-448 for +-Inf and NaN codes for NaN.  No test feeds an out-of-range length or page id to the GPU: the CPU
test of the shared position function covers those branches."""
import functools

import numpy as np
import pytest
import torch

import decode_calls as dc
import decode_refs as dr
from rocwmma_fattn.FlashAttn import flash_attention_decode, kvcache_append
from kvappend_refs import rotary_bar, rotary_ref64

pytestmark = pytest.mark.gpu

F16, BF16, E4M3 = torch.float16, torch.bfloat16, torch.float8_e4m3fn
LENS = (1, 63, 64, 65, 127, 129, 1000, 0, 2)
NMAX = 1024
LOG2E = 1.4426950408889634
# (H, Hkv, Nq, D, dtype): the decode tests' list — 1, 4, 20, 48 and 64 rows per K / V head
SHAPES = [(8, 8, 1, 128, F16), (8, 2, 1, 64, BF16), (10, 2, 4, 128, BF16), (16, 1, 3, 64, F16), (16, 1, 4, 128, F16)]
IDS = ["H%d_Hkv%d_Nq%d_D%d_%s" % (s[0], s[1], s[2], s[3], "f16" if s[4] == F16 else "bf16") for s in SHAPES]


def _pattern(nbytes, salt=0):
    """a per-byte poison pattern without a short period"""
    i = torch.arange(nbytes, dtype=torch.int64)
    return ((i * 131 + (i >> 8) * 7 + (i >> 16) * 3 + 89 + salt) % 251).to(torch.uint8)


def _pool(shape, dt, salt=0):
    """a cache tensor of `shape` and dtype `dt` (16-bit or e4m3) whose bytes are the pattern"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
    return _pattern(n, salt).view(dt).reshape(shape)


def _bytes(t):
    """the bytes of a contiguous cache tensor, [..., D * element size]"""
    return t.contiguous().view(torch.uint8)


def _targets(lens, nnew, cap):
    """[(b, i, p)] of the tokens that are written"""
    return [(b, i, n - nnew + i) for b, n in enumerate(lens) for i in range(nnew) if 0 <= n - nnew + i < cap]


def _expected(image, rows, lens, nnew, page=0, bt=None):
    """image [B | pages, rows, Hkv, bytes] (uint8, cloned): rows [B, Nnew, Hkv, bytes] written at the targets"""
    out = image.clone()
    for (b, i, p) in _targets(lens, nnew, NMAX):
        if page:
            out[int(bt[b, p // page]), p % page] = rows[b, i]
        else:
            out[b, p] = rows[b, i]
    return out


def _new_tokens(B, nnew, H, Hkv, D, dt, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    q, k, v = (torch.randn((B, nnew, h, D), generator=g).to(dt) for h in (H, Hkv, Hkv))
    return q, k, v


LAYOUTS = ["contiguous", "paged64", "paged128", "strided"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_image(shape, layout):
    """No rotary, 16-bit cache: V rows and K rows equal the source bit for bit at their targets, every other byte of the pool is unchanged."""
    dev = dc.dev()
    H, Hkv, nnew, D, dt = shape
    B = len(LENS)
    _, k, v = _new_tokens(B, nnew, H, Hkv, D, dt, 11 + H)
    g = torch.Generator(device="cpu").manual_seed(nnew + D)
    page, bt = 0, None
    if layout.startswith("paged"):
        page = int(layout[5:])
        bt, total, _ = dc.block_table(LENS, NMAX // page, page, g)
        kc, vc = _pool((total, page, Hkv, D), dt), _pool((total, page, Hkv, D), dt, 5)
        kview, vview = kc.to(dev), vc.to(dev)
    elif layout == "strided":                                  # a padded Nmax stride and a padded head stride
        kc, vc = _pool((B, NMAX + 48, Hkv + 1, D), dt), _pool((B, NMAX + 48, Hkv + 1, D), dt, 5)
        kfull, vfull = kc.to(dev), vc.to(dev)
        kview, vview = kfull[:, :NMAX, :Hkv], vfull[:, :NMAX, :Hkv]
        assert not kview.is_contiguous()
    else:
        kc, vc = _pool((B, NMAX, Hkv, D), dt), _pool((B, NMAX, Hkv, D), dt, 5)
        kview, vview = kc.to(dev), vc.to(dev)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    kd, vd = k.to(dev), v.to(dev)
    if layout == "strided":                                    # the new tokens as views with a padded head stride, too
        wide = torch.zeros((B, nnew, Hkv + 2, D), dtype=dt, device=dev)
        wide[:, :, :Hkv] = kd
        kd = wide[:, :, :Hkv]
    assert kvcache_append(kview, vview, kd, vd, lens, block_table=None if bt is None else bt.to(dev)) is None
    torch.cuda.synchronize()
    got_k, got_v = (_bytes((kfull if layout == "strided" else kview).cpu()), _bytes((vfull if layout == "strided" else vview).cpu()))
    if layout == "strided":                                    # the rows go through [:, :NMAX, :Hkv] of the full pool
        want_k, want_v = _bytes(kc).clone(), _bytes(vc).clone()
        for (b, i, p) in _targets(LENS, nnew, NMAX):
            want_k[b, p, :Hkv] = _bytes(k)[b, i]
            want_v[b, p, :Hkv] = _bytes(v)[b, i]
    else:
        want_k, want_v = _expected(_bytes(kc), _bytes(k), LENS, nnew, page, bt), _expected(_bytes(vc), _bytes(v), LENS, nnew, page, bt)
    assert len(_targets(LENS, nnew, NMAX)) < B * nnew or nnew == 1, "some tokens sit at negative positions"
    for name, got, want in (("k", got_k, want_k), ("v", got_v, want_v)):
        assert torch.equal(got, want), (name, layout, (got != want).nonzero()[:4].tolist())
    assert not torch.equal(got_k, _bytes(kc)), "something was written"


def _tables(rot, dt, seqlen_ro=NMAX):
    """cos / sin [seqlen_ro, rot / 2] from base 10 000 in float64 (every position's row is distinct), cast to dt"""
    inv = 10000.0 ** (-torch.arange(0, rot, 2, dtype=torch.float64) / rot)
    ang = torch.arange(seqlen_ro, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().to(dt), ang.sin().to(dt)


def _check_rotated(got, x, cos, sin, pos, rot, inter, dt, tag):
    """got / x [n, heads, D] rows at positions pos [n] (clamped into the table): float64 rotation under the derived bar, the tail exact"""
    rows = torch.as_tensor(pos).clamp(0, cos.shape[0] - 1)
    ref, mag = rotary_ref64(x.double(), cos[rows].double()[:, None, :], sin[rows].double()[:, None, :], rot, inter)
    err = (got.double() - ref).abs()
    bar = rotary_bar(ref, mag, dt)
    assert bool((err <= bar).all()), (tag, float((err - bar).max()), float(err.max()))
    assert torch.equal(got[..., rot:].view(torch.int16), x[..., rot:].view(torch.int16)), (tag, "columns at or beyond rotary_dim")
    print(tag, "max err %.3g, max err / bar %.3g" % (float(err.max()), float((err / bar).max())))


@pytest.mark.parametrize("table", ["f32", "io"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rotary(shape, table):
    dev = dc.dev()
    H, Hkv, nnew, D, dt = shape
    B = len(LENS)
    q, k, v = _new_tokens(B, nnew, H, Hkv, D, dt, 23 + H)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    tg = _targets(LENS, nnew, NMAX)
    bi = (torch.tensor([t[0] for t in tg]), torch.tensor([t[1] for t in tg]))
    pk = [t[2] for t in tg]
    qpos = [n - nnew + i for n in LENS for i in range(nnew)]
    for rot in (32, D):
        cos, sin = _tables(rot, torch.float32 if table == "f32" else dt)
        for inter in (True, False):
            kc, vc = _pool((B, NMAX, Hkv, D), dt), _pool((B, NMAX, Hkv, D), dt, 5)
            kcd, vcd = kc.to(dev), vc.to(dev)
            q_rot = kvcache_append(kcd, vcd, k.to(dev), v.to(dev), lens, rotary_cos=cos.to(dev), rotary_sin=sin.to(dev), rotary_interleaved=inter, q=q.to(dev))
            torch.cuda.synchronize()
            tag = (shape[:4], table, rot, "gptj" if inter else "neox")
            got = kcd.cpu()
            _check_rotated(got[bi[0], torch.tensor(pk)], k[bi], cos, sin, pk, rot, inter, dt, tag + ("k",))
            _check_rotated(q_rot.cpu().reshape(B * nnew, H, D), q.reshape(B * nnew, H, D), cos, sin, qpos, rot, inter, dt, tag + ("q",))
            # V is never rotated, and nothing but the targets changed
            assert torch.equal(_bytes(vcd.cpu()), _expected(_bytes(vc), _bytes(v), LENS, nnew))
            mask = torch.ones((B, NMAX), dtype=torch.bool)
            mask[bi[0], torch.tensor(pk)] = False
            assert torch.equal(_bytes(got)[mask], _bytes(kc)[mask])


def test_head_dim_96_rotary_dim_32():
    """A head dim decode does not serve (the append alone does): D = 96 is 12 chunks of 8 columns, rotary_dim 32 leaves 8 pass-through chunks behind
    the rotated span; both pairings, paged."""
    dev = dc.dev()
    H, Hkv, nnew, D, dt, rot = 4, 2, 3, 96, F16, 32
    B = len(LENS)
    q, k, v = _new_tokens(B, nnew, H, Hkv, D, dt, 96)
    bt, total, _ = dc.block_table(LENS, NMAX // 64, 64, torch.Generator(device="cpu").manual_seed(96))
    cos, sin = _tables(rot, torch.float32)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    tg = _targets(LENS, nnew, NMAX)
    for inter in (True, False):
        kc, vc = _pool((total, 64, Hkv, D), dt), _pool((total, 64, Hkv, D), dt, 5)
        kcd, vcd = kc.to(dev), vc.to(dev)
        q_rot = kvcache_append(kcd, vcd, k.to(dev), v.to(dev), lens, block_table=bt.to(dev), rotary_cos=cos.to(dev), rotary_sin=sin.to(dev),
                               rotary_interleaved=inter, q=q.to(dev))
        torch.cuda.synchronize()
        got = kcd.cpu()
        rows = torch.stack([got[int(bt[b, p // 64]), p % 64] for (b, i, p) in tg])
        src = torch.stack([k[b, i] for (b, i, p) in tg])
        _check_rotated(rows, src, cos, sin, [t[2] for t in tg], rot, inter, dt, ("D96", inter, "k"))
        _check_rotated(q_rot.cpu().reshape(B * nnew, H, D), q.reshape(B * nnew, H, D), cos, sin, [n - nnew + i for n in LENS for i in range(nnew)], rot, inter, dt,
                       ("D96", inter, "q"))
        assert torch.equal(_bytes(vcd.cpu()), _expected(_bytes(vc), _bytes(v), LENS, nnew, 64, bt))
        want = _expected(_bytes(kc), _bytes(got.new_zeros(k.shape)), LENS, nnew, 64, bt)       # (targets zeroed on both sides: the rest is the pattern)
        assert torch.equal(_expected(_bytes(got), _bytes(got.new_zeros(k.shape)), LENS, nnew, 64, bt), want)


def test_a_130_token_append():
    """Nnew = 130, more than two pages of 64: a prefill chunk.  Lengths after the append put tokens at negative positions (100), at the start of the
    cache (130), across page edges (200, 1000) and at the cache's last slot (1024)."""
    dev = dc.dev()
    lens_t, nnew, H, Hkv, D, dt = (130, 200, 1000, 100, 1024), 130, 4, 2, 64, BF16
    B = len(lens_t)
    q, k, v = _new_tokens(B, nnew, H, Hkv, D, dt, 130)
    bt, total, _ = dc.block_table(lens_t, NMAX // 64, 64, torch.Generator(device="cpu").manual_seed(130))
    lens = torch.tensor(lens_t, dtype=torch.int32, device=dev)
    kc, vc = _pool((total, 64, Hkv, D), dt), _pool((total, 64, Hkv, D), dt, 5)
    kcd, vcd = kc.to(dev), vc.to(dev)
    kvcache_append(kcd, vcd, k.to(dev), v.to(dev), lens, block_table=bt.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(_bytes(kcd.cpu()), _expected(_bytes(kc), _bytes(k), lens_t, nnew, 64, bt))
    assert torch.equal(_bytes(vcd.cpu()), _expected(_bytes(vc), _bytes(v), lens_t, nnew, 64, bt))
    # rotated (GPT-NeoX pairing, tables in the I/O dtype), contiguous
    cos, sin = _tables(D, dt)
    kc2, vc2 = _pool((B, NMAX, Hkv, D), dt).to(dev), _pool((B, NMAX, Hkv, D), dt, 5).to(dev)
    q_rot = kvcache_append(kc2, vc2, k.to(dev), v.to(dev), lens, rotary_cos=cos.to(dev), rotary_sin=sin.to(dev), rotary_interleaved=False, q=q.to(dev))
    tg = _targets(lens_t, nnew, NMAX)
    assert len(tg) == B * nnew - 30
    got = kc2.cpu()
    rows = torch.stack([got[b, p] for (b, i, p) in tg])
    _check_rotated(rows, torch.stack([k[b, i] for (b, i, p) in tg]), cos, sin, [t[2] for t in tg], D, False, dt, ("N130", "k"))
    _check_rotated(q_rot.cpu().reshape(B * nnew, H, D), q.reshape(B * nnew, H, D), cos, sin, [n - nnew + i for n in lens_t for i in range(nnew)], D, False, dt,
                   ("N130", "q"))


def _quant_ref(x, d=None):
    """torch's CPU cast after the clamp: RNE, +-448 for +-Inf, NaN codes for NaN"""
    y = x.float() if d is None else x.float() / d
    return y.clamp(-448.0, 448.0).to(E4M3)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_e4m3_every_input_pattern(dt):
    """All 65 536 bit patterns of the I/O dtype as v (and as k), 512 rows of 128, descale 1 (None and an explicit tensor of ones)."""
    dev = dc.dev()
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dt).reshape(1, 512, 1, 128)
    lens = torch.tensor([512], dtype=torch.int32, device=dev)
    ones = torch.ones((1, 1), device=dev)
    for kd in (None, ones):
        kc, vc = _pool((1, 512, 1, 128), E4M3).to(dev), _pool((1, 512, 1, 128), E4M3, 5).to(dev)
        kvcache_append(kc, vc, x.to(dev), x.to(dev), lens, k_descale=kd, v_descale=kd)
        torch.cuda.synchronize()
        nan = torch.isnan(x.float())
        want = _quant_ref(x).float()
        assert int(nan.sum()) > 0 and torch.isfinite(want[~nan]).all() and float(want[~nan].abs().max()) == 448.0
        for got8 in (kc.cpu(), vc.cpu()):
            got = got8.float()
            assert torch.equal(got[~nan], want[~nan]), ((got != want) & ~nan).nonzero()[:4].tolist()          # +-0 compare equal
            assert bool(((got8.view(torch.uint8)[nan] & 0x7F) == 0x7F).all()), "NaN in gives a NaN code (0x7f or 0xff)"


@pytest.mark.parametrize("layout", ["contiguous", "paged64"])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[3]], ids=[IDS[1], IDS[2], IDS[3]])
def test_e4m3_power_of_two_descales_are_bit_exact(shape, layout):
    dev = dc.dev()
    H, Hkv, nnew, D, dt = shape
    B = len(LENS)
    _, k, v = _new_tokens(B, nnew, H, Hkv, D, dt, 31 + H)
    g = torch.Generator(device="cpu").manual_seed(7 + D)
    kd, vd = (2.0 ** -torch.randint(5, 8, (B, Hkv), generator=g).float() for _ in range(2))
    page, bt = 0, None
    if layout == "paged64":
        page = 64
        bt, total, _ = dc.block_table(LENS, NMAX // page, page, g)
    cshape = (total, page, Hkv, D) if page else (B, NMAX, Hkv, D)
    kc, vc = _pool(cshape, E4M3), _pool(cshape, E4M3, 5)
    kcd, vcd = kc.to(dev), vc.to(dev)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    kvcache_append(kcd, vcd, k.to(dev), v.to(dev), lens, block_table=None if bt is None else bt.to(dev), k_descale=kd.to(dev), v_descale=vd.to(dev))
    torch.cuda.synchronize()
    want_k = _expected(_bytes(kc), _bytes(_quant_ref(k, kd[:, None, :, None])), LENS, nnew, page, bt)
    want_v = _expected(_bytes(vc), _bytes(_quant_ref(v, vd[:, None, :, None])), LENS, nnew, page, bt)
    assert torch.equal(_bytes(kcd.cpu()), want_k) and torch.equal(_bytes(vcd.cpu()), want_v)


@pytest.mark.parametrize("inter", [True, False], ids=["gptj", "neox"])
def test_e4m3_general_descale_and_rotated_k(inter):
    """Descales that are no powers of two, K rotated: the dequantised error against float64 is at most half an e4m3 step of the exact value plus f32
    slack, (2^-4 + 2^-20) |exact|, plus half the smallest subnormal step times the descale, d * 2^-10.  (|exact / d| stays below 448: no clamp.)"""
    dev = dc.dev()
    H, Hkv, nnew, D, dt = SHAPES[2]
    B = len(LENS)
    q, k, v = _new_tokens(B, nnew, H, Hkv, D, dt, 57)
    g = torch.Generator(device="cpu").manual_seed(58)
    kd, vd = (0.02 + 0.03 * torch.rand((B, Hkv), generator=g) for _ in range(2))
    cos, sin = _tables(D, torch.float32)
    kcd, vcd = _pool((B, NMAX, Hkv, D), E4M3).to(dev), _pool((B, NMAX, Hkv, D), E4M3, 5).to(dev)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    kvcache_append(kcd, vcd, k.to(dev), v.to(dev), lens, rotary_cos=cos.to(dev), rotary_sin=sin.to(dev), rotary_interleaved=inter, k_descale=kd.to(dev),
                   v_descale=vd.to(dev), q=q.to(dev))
    torch.cuda.synchronize()
    tg = _targets(LENS, nnew, NMAX)
    rows = torch.tensor([t[2] for t in tg])
    bi = (torch.tensor([t[0] for t in tg]), torch.tensor([t[1] for t in tg]))
    exact_k, _ = rotary_ref64(k[bi].double(), cos[rows].double()[:, None, :], sin[rows].double()[:, None, :], D, inter)
    for name, cache, exact, d in (("k", kcd, exact_k, kd), ("v", vcd, v[bi].double(), vd)):
        dd = d[bi[0]].double()[:, :, None]
        assert float((exact / dd).abs().max()) < 448.0
        deq = cache.cpu().view(torch.uint8)[bi[0], rows].view(E4M3).double() * dd
        err = (deq - exact).abs()
        bar = (2.0 ** -4 + 2.0 ** -20) * exact.abs() + dd * 2.0 ** -10
        print(name, inter, "max err / bar %.3g" % float((err / bar).max()))
        assert bool((err <= bar).all()), (name, float((err - bar).max()))


# Seeds of the fused cases' data.  decode_refs.refs_fp8 checks ITS OWN precondition on the CPU before anything is compared with the GPU: the oracle within
# FLOOR of float64 on these inputs.  Sequences of one or two keys with |V| up to 4 sit at 0.6 .. 1.15 of that floor whatever the seed (P rounded to 16
# bits times V); the e4m3 salt is the first of 3 .. 8 whose three shapes keep 10 % of margin (0.59 / 0.72 / 0.86), found with CPU code alone.
FUSED_SALT = {"16": 0, "fp8": 6}


@functools.lru_cache(maxsize=None)
def _fused_case(H, Hkv, nnew, D, dt, fmt):
    """CPU tensors of one fused case: q, the new k / v, caches whose first len_b keys are valid history (the append overwrites the last Nnew of them) and
    whose other keys are NaN, the descales (e4m3: powers of two), tables."""
    B = len(LENS)
    g = torch.Generator(device="cpu").manual_seed(1000 * H + 100 * Hkv + 10 * nnew + D + FUSED_SALT[fmt])
    q, k, v = (torch.randn((B, nnew, h, D), generator=g).to(dt) for h in (H, Hkv, Hkv))
    xk, xv = (torch.randn((B, NMAX, Hkv, D), generator=g) for _ in range(2))
    if fmt == "fp8":
        kd, vd = (2.0 ** -torch.randint(5, 8, (B, Hkv), generator=g).float() for _ in range(2))
        kc, vc = _quant_ref(xk, kd[:, None, :, None]), _quant_ref(xv, vd[:, None, :, None])
        for b, n in enumerate(LENS):
            kc.view(torch.uint8)[b, n:] = 0x7F
            vc.view(torch.uint8)[b, n:] = 0x7F
    else:
        kd = vd = None
        kc, vc = xk.to(dt), xv.to(dt)
        for b, n in enumerate(LENS):
            kc[b, n:] = float("nan")
            vc[b, n:] = float("nan")
    cos, sin = _tables(D, torch.float32)
    return q, k, v, kc, vc, kd, vd, cos, sin


@pytest.mark.parametrize("fmt", ["16", "fp8"])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[3]], ids=[IDS[1], IDS[2], IDS[3]])
def test_fused_call_equals_append_then_decode(shape, fmt):
    dev = dc.dev()
    H, Hkv, nnew, D, dt = shape
    q, k, v, kc, vc, kd, vd, cos, sin = _fused_case(*shape, fmt)
    qd, kn, vn, cosd, sind = (t.to(dev) for t in (q, k, v, cos, sin))
    kdd, vdd = (None if t is None else t.to(dev) for t in (kd, vd))
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    refs = None
    for ns in (0, 1, 3):
        ka, va, kb, vb = kc.to(dev), vc.to(dev), kc.to(dev), vc.to(dev)
        o, lse = flash_attention_decode(qd, ka, va, lens, return_lse=True, num_splits=ns, k_descale=kdd, v_descale=vdd, k=kn, v=vn, rotary_cos=cosd,
                                        rotary_sin=sind, rotary_interleaved=False)
        q_rot = kvcache_append(kb, vb, kn, vn, lens, rotary_cos=cosd, rotary_sin=sind, rotary_interleaved=False, k_descale=kdd, v_descale=vdd, q=qd)
        o2, lse2 = flash_attention_decode(q_rot, kb, vb, lens, return_lse=True, num_splits=ns, k_descale=kdd, v_descale=vdd)
        torch.cuda.synchronize()
        assert torch.equal(_bytes(ka.cpu()), _bytes(kb.cpu())) and torch.equal(_bytes(va.cpu()), _bytes(vb.cpu())), "the caches"
        assert torch.equal(o.view(torch.int16), o2.view(torch.int16)) and torch.equal(lse.view(torch.int32), lse2.view(torch.int32)), (shape[:4], fmt, ns)
        assert not torch.equal(_bytes(ka.cpu()), _bytes(kc)), "the append wrote"
        if refs is None:                                       # the references: on the cache contents and the rotated q read back from the device
            args = (q_rot.cpu(), ka.cpu(), va.cpu())
            refs = dr.refs16(*args, LENS, dc.code(dt)) if fmt == "16" else dr.refs_fp8(*args, kd, vd, LENS, dc.code(dt))
        dr.check(o, lse * LOG2E, refs, LENS, dc.code(dt), (shape[:4], fmt, ns), verbose=True)


def test_graph_replay_of_the_fused_paged_call():
    """One captured serving step — lengths incremented in place, new k / v / q copied into the captured inputs — replayed for three steps: each equals
    the eager call on a twin cache."""
    dev = dc.dev()
    H, Hkv, D, dt, page = 8, 2, 128, F16, 64
    start = (5, 62, 63, 126, 0)
    B, per = len(start), 4
    g = torch.Generator(device="cpu").manual_seed(91)
    order = torch.randperm(B * per + 2, generator=g)[:B * per].to(torch.int32).reshape(B, per)
    pool_k, pool_v = (torch.randn((B * per + 2, page, Hkv, D), generator=g).to(dt) for _ in range(2))
    cos, sin = (t.to(dev) for t in _tables(D, torch.float32, 256))
    bt = order.to(dev)
    steps = [tuple(torch.randn((B, 1, h, D), generator=g).to(dt).to(dev) for h in (H, Hkv, Hkv)) for _ in range(3)]
    # eager, on a twin
    tk, tv, tl = pool_k.to(dev), pool_v.to(dev), torch.tensor(start, dtype=torch.int32, device=dev)
    want = []
    for (q, k, v) in steps:
        tl += 1
        o, lse = flash_attention_decode(q, tk, tv, tl, block_table=bt, return_lse=True, k=k, v=v, rotary_cos=cos, rotary_sin=sin)
        want.append((o.clone(), lse.clone()))
    ck, cv, lens = pool_k.to(dev), pool_v.to(dev), torch.tensor(start, dtype=torch.int32, device=dev)
    qi, ki, vi = (t.clone() for t in steps[0])
    scratch_k, scratch_v, scratch_l = ck.clone(), cv.clone(), lens + 1
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up outside the capture, on caches of its own
        flash_attention_decode(qi, scratch_k, scratch_v, scratch_l, block_table=bt, return_lse=True, k=ki, v=vi, rotary_cos=cos, rotary_sin=sin)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            go, gl = flash_attention_decode(qi, ck, cv, lens, block_table=bt, return_lse=True, k=ki, v=vi, rotary_cos=cos, rotary_sin=sin)
    torch.cuda.current_stream().wait_stream(side)
    for s, (q, k, v) in enumerate(steps):
        lens += 1
        qi.copy_(q)
        ki.copy_(k)
        vi.copy_(v)
        go.zero_()
        gl.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(go.view(torch.int16), want[s][0].view(torch.int16)) and torch.equal(gl, want[s][1]), s
    assert torch.equal(ck, tk) and torch.equal(cv, tv) and torch.equal(lens, tl)
    assert not torch.equal(want[0][0], want[1][0])
