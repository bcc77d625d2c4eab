"""The C calls of the five serving operators (flash_attention_decode, flash_attention_prefill, flash_attention_prefill_fp8, kvcache_append,
kvcache_append_varlen), without a device: every call a table of operator calls makes is recorded by decode_calls.recording_lib and compared, argument
for argument, with values this file computes from the tensors and puts in order through decode_abi.c_args — never with what the operator says.  A pointer
the operator allocates (lse, the rotated q, a contiguous copy) is the one value taken from the record: it must be set and must not be an input's.
The tables cover both cache layouts and formats, the descale combinations, decode's three entries, the prefill options and its pad path, the fused
calls (append first, attention second, on the rotated q, with the same descales) and the appends' copies; every fused call, given an argument only
the append refuses, raises before the first C call."""
import ctypes

import pytest
import torch

import decode_calls as dc
from rocwmma_fattn import FlashAttn, _fa2_lib

F16, BF16, E4M3 = torch.float16, torch.bfloat16, torch.float8_e4m3fn
C16, C8, F32 = _fa2_lib.FA2_CACHE_16BIT, _fa2_lib.FA2_CACHE_E4M3, _fa2_lib.FA2_DTYPE_F32
LAYOUTS = [(paged, cache) for paged in (False, True) for cache in (F16, E4M3)]
LAYOUT_IDS = ["%s-%s" % ("paged" if p else "contiguous", "e4m3" if c == E4M3 else "16bit") for p, c in LAYOUTS]
DESCALES = ("none", "k", "v", "both", "split")


# ---------------------------------------------------------------------------------------------------------------- what the tensors say
def ptr(t):
    return None if t is None else t.data_ptr()


def code(dt):
    return _fa2_lib.FA2_DTYPE_F16 if dt == F16 else _fa2_lib.FA2_DTYPE_BF16


def bnhd(t):
    """{batch | page, head, row} of a [B, N, heads, D] tensor"""
    return None if t is None else (t.stride(0), t.stride(2), t.stride(1))


def hr(t):
    """{head, row} of a packed [total, heads, D] tensor"""
    return None if t is None else (t.stride(1), t.stride(0))


class Fresh:
    """A pointer the operator allocated: set, and none of `others`' (the inputs it must not be)."""

    def __init__(self, *others):
        self.others = [ptr(t) for t in others]


def cache_kw(kc, vc, lens, bt=None, kd=None, vd=None, split=False):
    """The cache's part of every entry's arguments.  split: the descales came with different strides, so the call gets contiguous copies."""
    paged = bt is not None
    d0 = kd if kd is not None else vd
    kw = dict(fmt=C8 if kc.dtype == E4M3 else C16, k=ptr(kc), v=ptr(vc), lens=ptr(lens), bt=ptr(bt), Hkv=kc.shape[2], cap=bt.shape[1] if paged else kc.shape[1],
              page=kc.shape[1] if paged else 0, pages=kc.shape[0] if paged else 0, ks=bnhd(kc), vs=bnhd(vc), bts=bt.stride(0) if paged else 0, kd=ptr(kd), vd=ptr(vd),
              ds=None if d0 is None else tuple(d0.stride()))
    if split:
        assert kd.stride() != vd.stride() and not kd.is_contiguous() and not vd.is_contiguous()
        kw.update(kd=Fresh(kd, vd), vd=Fresh(kd, vd), ds=(kc.shape[2], 1))
    return kw


def check_call(call, entry, **want):
    """One recorded call is the named entry's, on c_args(entry, **want) -> its arguments by keyword"""
    name, got = call
    symbol, order = dc.ENTRIES[entry][:2]
    assert name == symbol
    expected = dc.c_args(entry, **want)
    assert len(got) == len(order)
    for n, g, w in zip(order, got, expected):
        g = tuple(g) if isinstance(g, ctypes.Array) else g
        if isinstance(w, Fresh):
            assert g not in (None, 0) and g not in w.others, (symbol, n, g)
        else:
            assert g == w and isinstance(g, float) == isinstance(w, float), (symbol, n, g, w)
    return dict(zip(order, got))


def scoremod_kw(wl=-1, softcap=0.0, slopes=None):
    return dict(wl=wl, cap_=float(softcap), sl=ptr(slopes), st=0 if slopes is None or slopes.dim() == 1 else slopes.stride(0))


def decode_want(q, o, cache, ns=0, q_ptr=None, **mods):
    """-> the entry flash_attention_decode(q, ...) -> o goes to, and its arguments (q_ptr: the q the kernel reads, when it is not the caller's)"""
    B, Nq, H, D = q.shape
    mod = scoremod_kw(**mods)
    entry = "window" if mod != scoremod_kw() else "fp8" if cache["fmt"] == C8 else "plain"
    return entry, dict(cache, **mod, dtype=code(q.dtype), q=ptr(q) if q_ptr is None else q_ptr, o=ptr(o), lse=Fresh(q, o), B=B, H=H, Nq=Nq, D=D,
                       qs=bnhd(q) if q_ptr is None else (Nq * H * D, D, H * D), os=(Nq * H * D, D, H * D), ls=(H * Nq, Nq), scale=D ** -0.5, ns=ns, ws=None, wsb=0,
                       stream=None)


def check_decode(calls, q, o, cache, ns=0, q_ptr=None, **mods):
    """The size query of the entry, then the entry"""
    entry, want = decode_want(q, o, cache, ns, q_ptr, **mods)
    (qname, qargs), call = calls
    sizes = tuple(want[n] for n in ("dtype", "B", "H", "Hkv", "Nq", "D", "cap", "page", "ns")) + ((want["wl"],) if entry == "window" else ())
    assert (qname, qargs) == (dc.ENTRIES[entry][2], sizes)
    return check_call(call, entry, **want)


def prefill_want(q, o, cu, cache, max_q, D=None, q_ptr=None, scale=None, **mods):
    """-> the entry and the arguments of flash_attention_prefill[_fp8](q, ...) -> o.  D: the head dim the kernel runs at (the pad path: not q's)"""
    total, H, Dq = q.shape
    D = Dq if D is None else D
    entry = "prefill_fp8" if cache["fmt"] == C8 else "prefill"
    return entry, dict(cache, **scoremod_kw(**mods), dtype=code(q.dtype), q=ptr(q) if q_ptr is None else q_ptr, o=ptr(o), lse=Fresh(q, o), cu=ptr(cu), B=cu.numel() - 1,
                       H=H, max_q=max_q, D=D, qs=hr(q) if q_ptr is None else (D, H * D), os=(D, H * D), lss=total, scale=Dq ** -0.5 if scale is None else scale,
                       stream=None)


def rotary_kw(k, cos=None, sin=None, inter=True, cos_ptr=None, sin_ptr=None, ros=None):
    """cos_ptr / sin_ptr / ros: what a table that had to be copied becomes"""
    if cos is None:
        return dict(cos=None, sin=None, rdt=0, rot=0, sro=0, ros=0, inter=1 if inter else 0)
    return dict(cos=ptr(cos) if cos_ptr is None else cos_ptr, sin=ptr(sin) if sin_ptr is None else sin_ptr, rdt=F32 if cos.dtype == torch.float32 else code(k.dtype),
                rot=2 * cos.shape[1], sro=cos.shape[0], ros=cos.stride(0) if ros is None else ros, inter=1 if inter else 0)


def append_want(k, v, cache, q=None, kn_ptr=None, **rot):
    """kvcache_append(k, v [B, Nnew, Hkv, D], q=q).  kn_ptr: k had to be copied"""
    B, N, Hkv, D = k.shape
    H = 0 if q is None else q.shape[2]
    return "append", dict(cache, **rotary_kw(k, **rot), dtype=code(k.dtype), kn=ptr(k) if kn_ptr is None else kn_ptr, vn=ptr(v), B=B, N=N, D=D,
                          kns=bnhd(k) if kn_ptr is None else (N * Hkv * D, D, Hkv * D), vns=bnhd(v), q=ptr(q), qo=None if q is None else Fresh(q, k, v), H=H,
                          Nq=0 if q is None else N, qs=bnhd(q), qos=None if q is None else (N * H * D, D, H * D), stream=None)


def append_varlen_want(k, v, cu, cache, q=None, kn_ptr=None, **rot):
    """kvcache_append_varlen(k, v [total, Hkv, D], cu, q=q)"""
    total, Hkv, D = k.shape
    H = 0 if q is None else q.shape[1]
    return "append_varlen", dict(cache, **rotary_kw(k, **rot), dtype=code(k.dtype), kn=ptr(k) if kn_ptr is None else kn_ptr, vn=ptr(v), cu=ptr(cu), B=cu.numel() - 1,
                                 total=total, D=D, kns=hr(k) if kn_ptr is None else (D, Hkv * D), vns=hr(v), q=ptr(q), qo=None if q is None else Fresh(q, k, v), H=H,
                                 qs=hr(q), qos=None if q is None else (D, H * D), stream=None)


# ---------------------------------------------------------------------------------------------------------------- the table's tensors
def caches(paged=True, cache=F16, dt=F16, D=64):
    """-> k_cache, v_cache (e4m3, or 16-bit in dt), cache_seqlens, block_table (None: contiguous) for two sequences"""
    kc = torch.zeros((6, 64, 2, D) if paged else (2, 128, 2, D), dtype=dt).to(E4M3 if cache == E4M3 else dt)
    return kc, kc.clone(), torch.tensor([70, 100], dtype=torch.int32), torch.tensor([[2, 3, 0], [4, 1, 5]], dtype=torch.int32) if paged else None


def packed(dt=F16, D=64, total=10):
    """-> q [total, 4, D], k, v [total, 2, D], cu_seqlens"""
    cu = torch.tensor([0, 4, total] if total else [0, 0, 0], dtype=torch.int32)
    return torch.zeros(total, 4, D, dtype=dt), torch.zeros(total, 2, D, dtype=dt), torch.zeros(total, 2, D, dtype=dt), cu


def uniform(dt=F16, D=64, N=1):
    """-> q [2, N, 4, D], k, v [2, N, 2, D]"""
    return torch.zeros(2, N, 4, D, dtype=dt), torch.zeros(2, N, 2, D, dtype=dt), torch.zeros(2, N, 2, D, dtype=dt)


def descales(which):
    """-> k_descale, v_descale [2, 2] and whether the call must copy them ("split": two strided views with different strides)"""
    if which == "split":
        return torch.ones(4, 2)[::2], torch.ones(2, 4)[:, ::2], True
    wide = torch.ones(2, 2, 3)
    return (wide[..., 0] if which in ("k", "both") else None), (wide[..., 1] if which in ("v", "both") else None), False


def tables(dt=torch.float32, rows=16, half=16):
    return torch.ones(rows, half, dtype=dt), torch.zeros(rows, half, dtype=dt)


@pytest.fixture
def rec(monkeypatch):
    return dc.recording_lib(monkeypatch)


def run(rec, f, *a, **kw):
    del rec.calls[:]
    out = f(*a, **kw)
    return out, list(rec.calls)


# ---------------------------------------------------------------------------------------------------------------- layout, format and descales
@pytest.mark.parametrize("paged,cache", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("dt", (F16, BF16), ids=("f16", "bf16"))
def test_decode_on_every_layout_and_format(rec, paged, cache, dt):
    q = uniform(dt)[0]
    kc, vc, lens, bt = caches(paged, cache, dt)
    o, calls = run(rec, FlashAttn.flash_attention_decode, q, kc, vc, lens, bt)
    check_decode(calls, q, o, cache_kw(kc, vc, lens, bt))
    assert o.shape == q.shape and o.dtype == dt


@pytest.mark.parametrize("paged,cache", LAYOUTS, ids=LAYOUT_IDS)
def test_prefill_on_every_layout_and_format(rec, paged, cache):
    q, _, _, cu = packed()
    kc, vc, lens, bt = caches(paged, cache)
    f = FlashAttn.flash_attention_prefill_fp8 if cache == E4M3 else FlashAttn.flash_attention_prefill
    o, calls = run(rec, f, q, kc, vc, cu, lens, bt, max_seqlen_q=6)
    (call,) = calls
    entry, want = prefill_want(q, o, cu, cache_kw(kc, vc, lens, bt), 6)
    assert entry == ("prefill_fp8" if cache == E4M3 else "prefill")
    check_call(call, entry, **want)
    assert o.shape == q.shape


@pytest.mark.parametrize("paged,cache", LAYOUTS, ids=LAYOUT_IDS)
def test_appends_on_every_layout_and_format(rec, paged, cache):
    kc, vc, lens, bt = caches(paged, cache)
    _, k, v = uniform(N=3)
    out, (call,) = run(rec, FlashAttn.kvcache_append, kc, vc, k, v, lens, bt)
    entry, want = append_want(k, v, cache_kw(kc, vc, lens, bt))
    check_call(call, entry, **want)
    assert out is None
    _, k, v, cu = packed()
    out, (call,) = run(rec, FlashAttn.kvcache_append_varlen, kc, vc, k, v, cu, lens, bt)
    entry, want = append_varlen_want(k, v, cu, cache_kw(kc, vc, lens, bt))
    check_call(call, entry, **want)
    assert out is None


@pytest.mark.parametrize("which", DESCALES)
@pytest.mark.parametrize("op", ("decode", "prefill_fp8", "append", "append_varlen"))
def test_descales_reach_every_e4m3_call(rec, op, which):
    """None, one, the other, both (strided alike: passed as they are, with their stride pair), both with different strides (contiguous copies)"""
    kc, vc, lens, bt = caches(True, E4M3)
    kd, vd, split = descales(which)
    cache = cache_kw(kc, vc, lens, bt, kd, vd, split)
    if not split and which != "none":
        assert cache["ds"] == (6, 3)
    if op == "decode":
        q = uniform()[0]
        o, calls = run(rec, FlashAttn.flash_attention_decode, q, kc, vc, lens, bt, k_descale=kd, v_descale=vd)
        got = check_decode(calls, q, o, cache)
    elif op == "prefill_fp8":
        q, _, _, cu = packed()
        o, (call,) = run(rec, FlashAttn.flash_attention_prefill_fp8, q, kc, vc, cu, lens, bt, max_seqlen_q=6, k_descale=kd, v_descale=vd)
        entry, want = prefill_want(q, o, cu, cache, 6)
        got = check_call(call, entry, **want)
    elif op == "append":
        _, k, v = uniform()
        _, (call,) = run(rec, FlashAttn.kvcache_append, kc, vc, k, v, lens, bt, k_descale=kd, v_descale=vd)
        entry, want = append_want(k, v, cache)
        got = check_call(call, entry, **want)
    else:
        _, k, v, cu = packed()
        _, (call,) = run(rec, FlashAttn.kvcache_append_varlen, kc, vc, k, v, cu, lens, bt, k_descale=kd, v_descale=vd)
        entry, want = append_varlen_want(k, v, cu, cache)
        got = check_call(call, entry, **want)
    if split:
        assert got["kd"] != got["vd"]


# ---------------------------------------------------------------------------------------------------------------- flash_attention_decode
@pytest.mark.parametrize("cache", (F16, E4M3), ids=("16bit", "e4m3"))
def test_decode_reaches_the_banded_entry_and_passes_num_splits(rec, cache):
    q = uniform(N=2)[0]
    kc, vc, lens, bt = caches(True, cache)
    ckw = cache_kw(kc, vc, lens, bt)
    f = FlashAttn.flash_attention_decode
    slopes_h, slopes_bh = torch.ones(4), torch.ones(2, 4)
    for kw, mods in ((dict(window=5), dict(wl=5)), (dict(window=(7, 0)), dict(wl=7)), (dict(softcap=30.0), dict(softcap=30.0)),
                     (dict(alibi_slopes=slopes_h), dict(slopes=slopes_h)), (dict(alibi_slopes=slopes_bh), dict(slopes=slopes_bh)),
                     (dict(window=3, softcap=2, alibi_slopes=slopes_bh), dict(wl=3, softcap=2.0, slopes=slopes_bh))):
        o, calls = run(rec, f, q, kc, vc, lens, bt, num_splits=3, **kw)
        got = check_decode(calls, q, o, ckw, ns=3, **mods)
        assert calls[1][0] == "fa2_fwd_decode_window" and got["fmt"] == ckw["fmt"]
    for ns in (0, 1, 16):
        o, calls = run(rec, f, q, kc, vc, lens, bt, num_splits=ns)
        check_decode(calls, q, o, ckw, ns=ns)
        assert calls[1][0] == ("fa2_fwd_decode_fp8" if cache == E4M3 else "fa2_fwd_decode")
    o, calls = run(rec, f, q, kc, vc, lens, bt, return_lse=True, scale=0.25)
    entry, want = decode_want(q, o[0], ckw)
    got = check_call(calls[1], entry, **dict(want, scale=0.25, lse=Fresh(q, *o)))
    assert o[1].shape == (2, 4, 2) and o[1].dtype == torch.float32
    # a q the kernel cannot address is copied; the caches never are
    wide = torch.zeros(2, 2, 4, 128, dtype=F16)
    o, calls = run(rec, f, wide[..., ::2], kc, vc, lens, bt)
    check_decode(calls, wide[..., ::2], o, ckw, q_ptr=Fresh(wide))


# ---------------------------------------------------------------------------------------------------------------- the prefill calls
@pytest.mark.parametrize("cache", (F16, E4M3), ids=("16bit", "e4m3"))
def test_prefill_options_reach_the_call(rec, cache):
    q, _, _, cu = packed()
    kc, vc, lens, bt = caches(True, cache)
    ckw = cache_kw(kc, vc, lens, bt)
    f = FlashAttn.flash_attention_prefill_fp8 if cache == E4M3 else FlashAttn.flash_attention_prefill
    slopes_h, slopes_bh = torch.ones(4), torch.ones(2, 4)
    for kw, mods in ((dict(), dict()), (dict(window=5), dict(wl=5)), (dict(window=(7, 0)), dict(wl=7)), (dict(softcap=30.0), dict(softcap=30.0)),
                     (dict(alibi_slopes=slopes_h), dict(slopes=slopes_h)), (dict(alibi_slopes=slopes_bh), dict(slopes=slopes_bh)),
                     (dict(window=3, softcap=2, alibi_slopes=slopes_bh, scale=0.5), dict(wl=3, softcap=2.0, slopes=slopes_bh, scale=0.5))):
        for max_q in (6, 300):
            o, (call,) = run(rec, f, q, kc, vc, cu, lens, bt, max_seqlen_q=max_q, **kw)
            entry, want = prefill_want(q, o, cu, ckw, max_q, **mods)
            check_call(call, entry, **want)
    (o, lse), (call,) = run(rec, f, q, kc, vc, cu, lens, bt, max_seqlen_q=6, return_lse=True)
    entry, want = prefill_want(q, o, cu, ckw, 6)
    check_call(call, entry, **dict(want, lse=Fresh(q, o, lse)))
    assert lse.shape == (4, 10) and lse.dtype == torch.float32
    # a stated maximum of 0: no call, o zero, lse -inf
    q1 = torch.ones_like(q)
    (o, lse), calls = run(rec, f, q1, kc, vc, cu, lens, bt, max_seqlen_q=0, return_lse=True)
    assert calls == [] and o.shape == q.shape and not o.any() and bool((lse == float("-inf")).all()) and lse.shape == (4, 10)
    # no query row: no call
    q0, _, _, cu0 = packed(total=0)
    (o, lse), calls = run(rec, f, q0, kc, vc, cu0, lens, bt, max_seqlen_q=6, return_lse=True)
    assert calls == [] and o.shape == (0, 4, 64) and lse.shape == (4, 0)
    # a q the kernel cannot address is copied; the caches never are
    wide = torch.zeros(10, 4, 128, dtype=F16)
    o, (call,) = run(rec, f, wide[..., ::2], kc, vc, cu, lens, bt, max_seqlen_q=6)
    entry, want = prefill_want(wide[..., ::2], o, cu, ckw, 6, q_ptr=Fresh(wide))
    check_call(call, entry, **want)


@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
def test_prefill_pads_head_dim_60_to_64_on_copies(rec, paged):
    q, _, _, cu = packed(D=60)
    kc, vc, lens, bt = caches(paged, D=60)
    o, (call,) = run(rec, FlashAttn.flash_attention_prefill, q, kc, vc, cu, lens, bt, max_seqlen_q=6)
    rows = kc.shape[1]
    padded = dict(cache_kw(kc, vc, lens, bt), k=Fresh(kc, vc, q), v=Fresh(kc, vc, q), ks=(rows * 2 * 64, 64, 2 * 64), vs=(rows * 2 * 64, 64, 2 * 64))
    entry, want = prefill_want(q, o, cu, padded, 6, D=64, q_ptr=Fresh(q, kc, vc))
    got = check_call(call, entry, **want)
    assert got["D"] == 64 and len({got["q"], got["k"], got["v"], got["o"]}) == 4
    assert o.shape == (10, 4, 60) and o.stride() == (4 * 64, 64, 1)


# ---------------------------------------------------------------------------------------------------------------- fused calls
def _dead(t):
    """the tensor on a device that is not the call's: what only the append's own device check refuses"""
    return torch.empty(t.shape, dtype=t.dtype, device="meta")


@pytest.mark.parametrize("rotary", (False, True), ids=("plain", "rotary"))
@pytest.mark.parametrize("paged,cache", LAYOUTS, ids=LAYOUT_IDS)
def test_fused_decode_appends_then_decodes(rec, paged, cache, rotary):
    q, k, v = uniform(N=2)
    kc, vc, lens, bt = caches(paged, cache)
    kd, vd, split = descales("split" if cache == E4M3 else "none")
    cos, sin = tables(half=32)
    rot = dict(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=False) if rotary else {}
    o, calls = run(rec, FlashAttn.flash_attention_decode, q, kc, vc, lens, bt, k=k, v=v, k_descale=kd, v_descale=vd, num_splits=2, **rot)
    assert [n for n, _ in calls] == ["fa2_kvcache_append", dc.ENTRIES["fp8" if cache == E4M3 else "plain"][2], dc.ENTRIES["fp8" if cache == E4M3 else "plain"][0]]
    ckw = cache_kw(kc, vc, lens, bt, kd, vd, split)
    entry, want = append_want(k, v, ckw, q=q if rotary else None, **(dict(cos=cos, sin=sin, inter=False) if rotary else {}))
    app = check_call(calls[0], entry, **want)
    dec = check_decode(calls[1:], q, o, ckw, ns=2, q_ptr=app["qo"] if rotary else None)
    assert dec["q"] == (app["qo"] if rotary else q.data_ptr()) and (app["q"], app["Nq"]) == ((q.data_ptr(), 2) if rotary else (None, 0))
    if cache == E4M3:
        assert (app["kd"], app["vd"], tuple(app["ds"])) == (dec["kd"], dec["vd"], tuple(dec["ds"])), "one pair of descales for both calls"
    else:
        assert (app["kd"], app["vd"], app["ds"]) == (None, None, None)
    # an argument only the append looks at: the call raises before the first C call
    for bad in ((dict(rot, rotary_sin=_dead(sin)),) if rotary else ()) + (dict(rot, v=_dead(v)),):
        del rec.calls[:]
        with pytest.raises(RuntimeError, match="must be on the ROCm device of the caches"):
            FlashAttn.flash_attention_decode(q, kc, vc, lens, bt, **dict(dict(k=k, v=v, k_descale=kd, v_descale=vd), **bad))
        assert rec.calls == []
    if rotary:
        with pytest.raises(ValueError, match="share one dtype"):
            FlashAttn.flash_attention_decode(q, kc, vc, lens, bt, k=k, v=v, k_descale=kd, v_descale=vd, rotary_cos=cos, rotary_sin=sin.half())
        assert rec.calls == []


@pytest.mark.parametrize("rotary", (False, True), ids=("plain", "rotary"))
@pytest.mark.parametrize("paged,cache", LAYOUTS, ids=LAYOUT_IDS)
def test_fused_prefill_appends_then_attends(rec, paged, cache, rotary):
    q, k, v, cu = packed()
    kc, vc, lens, bt = caches(paged, cache)
    kd, vd, split = descales("split" if cache == E4M3 else "none")
    cos, sin = tables(torch.float16)
    f = FlashAttn.flash_attention_prefill_fp8 if cache == E4M3 else FlashAttn.flash_attention_prefill
    base = dict(max_seqlen_q=6, k=k, v=v, window=9)
    if cache == E4M3:
        base.update(k_descale=kd, v_descale=vd)
    rot = dict(rotary_cos=cos, rotary_sin=sin) if rotary else {}
    o, calls = run(rec, f, q, kc, vc, cu, lens, bt, **base, **rot)
    assert [n for n, _ in calls] == ["fa2_kvcache_append_varlen", "fa2_fwd_prefill_fp8" if cache == E4M3 else "fa2_fwd_prefill"]
    ckw = cache_kw(kc, vc, lens, bt, kd, vd, split)
    entry, want = append_varlen_want(k, v, cu, ckw, q=q if rotary else None, **(dict(cos=cos, sin=sin) if rotary else {}))
    app = check_call(calls[0], entry, **want)
    entry, want = prefill_want(q, o, cu, ckw, 6, q_ptr=app["qo"] if rotary else None, wl=9)
    att = check_call(calls[1], entry, **want)
    assert att["q"] == (app["qo"] if rotary else q.data_ptr()) and app["q"] == (q.data_ptr() if rotary else None)
    if cache == E4M3:
        assert (app["kd"], app["vd"], tuple(app["ds"])) == (att["kd"], att["vd"], tuple(att["ds"])), "one pair of descales for both calls"
    for bad in ((dict(rot, rotary_sin=_dead(sin)),) if rotary else ()) + (dict(rot, v=_dead(v)),):
        del rec.calls[:]
        with pytest.raises(RuntimeError, match="must be on the ROCm device of the caches"):
            f(q, kc, vc, cu, lens, bt, **dict(base, **bad))
        assert rec.calls == []
    if rotary:
        with pytest.raises(ValueError, match="share one dtype"):
            f(q, kc, vc, cu, lens, bt, **dict(base, rotary_cos=cos, rotary_sin=sin.float()))
        assert rec.calls == []


# ---------------------------------------------------------------------------------------------------------------- the appends
def _table_cases():
    """(what the call is given, what reaches the C call): f32 and 16-bit tables, both pairings, tables that need the contiguous copy"""
    cos, sin = tables()
    yield dict(rotary_cos=cos, rotary_sin=sin), dict(cos=cos, sin=sin)
    yield dict(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=False), dict(cos=cos, sin=sin, inter=False)
    cos, sin = tables(torch.float16, rows=40, half=8)
    yield dict(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=True), dict(cos=cos, sin=sin)
    wide = torch.ones(16, 32)
    cos, sin = wide[:, ::2], wide[:, 1::2]                              # columns apart: both copied
    yield dict(rotary_cos=cos, rotary_sin=sin), dict(cos=cos, sin=sin, cos_ptr=Fresh(wide, sin), sin_ptr=Fresh(wide, sin), ros=16)
    cos, sin = torch.ones(16, 16), wide[:, :16]                         # two row strides: one stride for both, so sin is copied
    yield dict(rotary_cos=cos, rotary_sin=sin), dict(cos=cos, sin=sin, sin_ptr=Fresh(wide, cos), ros=16)
    cos, sin = wide[:, :16], wide[:, 16:]                               # strided alike, rows on 16-byte boundaries: passed as they are
    yield dict(rotary_cos=cos, rotary_sin=sin), dict(cos=cos, sin=sin, ros=32)


@pytest.mark.parametrize("with_q", (False, True), ids=("k", "k+q"))
@pytest.mark.parametrize("cache", (F16, E4M3), ids=("16bit", "e4m3"))
def test_appends_pass_the_tables_and_q(rec, cache, with_q):
    kc, vc, lens, bt = caches(True, cache)
    ckw = cache_kw(kc, vc, lens, bt)
    for given, reach in _table_cases():
        q, k, v = uniform(N=3)
        out, (call,) = run(rec, FlashAttn.kvcache_append, kc, vc, k, v, lens, bt, q=q if with_q else None, **given)
        entry, want = append_want(k, v, ckw, q=q if with_q else None, **reach)
        got = check_call(call, entry, **want)
        assert (got["Nq"], got["H"]) == ((3, 4) if with_q else (0, 0))
        assert (out is None) if not with_q else (out.data_ptr() == got["qo"] and out.shape == q.shape and out.dtype == q.dtype)
        q, k, v, cu = packed()
        out, (call,) = run(rec, FlashAttn.kvcache_append_varlen, kc, vc, k, v, cu, lens, bt, q=q if with_q else None, **given)
        entry, want = append_varlen_want(k, v, cu, ckw, q=q if with_q else None, **reach)
        got = check_call(call, entry, **want)
        assert (out is None) if not with_q else (out.data_ptr() == got["qo"] and out.shape == q.shape and out.dtype == q.dtype)


def test_appends_copy_new_tokens_they_cannot_address_and_skip_an_empty_buffer(rec):
    kc, vc, lens, bt = caches(True)
    ckw = cache_kw(kc, vc, lens, bt)
    wide = torch.zeros(2, 3, 2, 128, dtype=F16)
    v = uniform(N=3)[2]
    _, (call,) = run(rec, FlashAttn.kvcache_append, kc, vc, wide[..., ::2], v, lens, bt)
    entry, want = append_want(wide[..., ::2], v, ckw, kn_ptr=Fresh(wide, v))
    check_call(call, entry, **want)
    _, (call,) = run(rec, FlashAttn.kvcache_append, kc, vc, wide[..., :64], v, lens, bt)            # a view the kernel addresses: passed as it is
    entry, want = append_want(wide[..., :64], v, ckw)
    assert check_call(call, entry, **want)["kns"][2] == 256
    wide = torch.zeros(10, 2, 128, dtype=F16)
    q, _, v, cu = packed()
    _, (call,) = run(rec, FlashAttn.kvcache_append_varlen, kc, vc, wide[..., ::2], v, cu, lens, bt)
    entry, want = append_varlen_want(wide[..., ::2], v, cu, ckw, kn_ptr=Fresh(wide, v))
    check_call(call, entry, **want)
    _, (call,) = run(rec, FlashAttn.kvcache_append_varlen, kc, vc, wide[..., 64:], v, cu, lens, bt)
    entry, want = append_varlen_want(wide[..., 64:], v, cu, ckw)
    assert check_call(call, entry, **want)["kns"][1] == 256
    # total = 0 on the packed append: no call; with q and tables an empty q comes back
    cos, sin = tables()
    out, calls = run(rec, FlashAttn.kvcache_append_varlen, kc, vc, wide[:0, :, :64], v[:0], cu, lens, bt)
    assert out is None and calls == []
    out, calls = run(rec, FlashAttn.kvcache_append_varlen, kc, vc, wide[:0, :, :64], v[:0], cu, lens, bt, rotary_cos=cos, rotary_sin=sin, q=q[:0])
    assert out.shape == (0, 4, 64) and calls == []
