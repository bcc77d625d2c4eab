"""CPU tests of the packed (ragged) KV-cache append (include/fa2_gfx950.h: fa2_kvcache_append_varlen, fa2_kvappend_varlen_token; kvcache_append_varlen and
the k / v / rotary_* keywords of flash_attention_prefill): the symbols, the token -> sequence function the kernel and the host share — exhaustively on
well-formed offsets against a linear scan, and on hostile arrays against the one property the kernel's safety rests on — every validation code of the
new entry and the order they are checked in, the operator's argument checks, and the calls the operator makes, through a stand-in library.
Nothing here touches a device: every rejected call returns before the launch."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import decode_calls as dc
from conftest import ROOT
from rocwmma_fattn import FlashAttn, _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention_prefill, kvcache_append_varlen

HEADER = os.path.join(ROOT, "include", "fa2_gfx950.h")
SYMBOLS = ("fa2_kvcache_append_varlen", "fa2_kvappend_varlen_token")
OK, NULLP, SHAPE, HEAD_DIM, ALIGN, DTYPE, SCALE, GRID = 0, -1, -2, -3, -4, -5, -6, -7
F16, BF16, F32 = _fa2_lib.FA2_DTYPE_F16, _fa2_lib.FA2_DTYPE_BF16, _fa2_lib.FA2_DTYPE_F32
C16, C8 = _fa2_lib.FA2_CACHE_16BIT, _fa2_lib.FA2_CACHE_E4M3
E4M3 = torch.float8_e4m3fn
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def test_symbols_are_declared_exported_and_bound():
    lib = _fa2_lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _fa2_lib.SYMBOLS, name
        assert getattr(lib, name).argtypes == _fa2_lib.SYMBOLS[name][1]
    proto = re.search(r"\bfa2_kvcache_append_varlen\s*\((.*?)\);", text, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_fa2_lib.SYMBOLS["fa2_kvcache_append_varlen"][1]) == len(dc.ENTRIES["append_varlen"][1]) == 37
    assert _fa2_lib.SYMBOLS["fa2_kvcache_append_varlen"][1][10] is ctypes.c_int64, "total is a 64-bit count"
    assert len(_fa2_lib.SYMBOLS["fa2_kvappend_varlen_token"][1]) == 6
    import rocwmma_fattn
    assert "kvcache_append_varlen" in FlashAttn.__all__ and rocwmma_fattn.kvcache_append_varlen is kvcache_append_varlen


# ---------------------------------------------------------------------------------------------------------------- token -> sequence
class _Token:
    """fa2_kvappend_varlen_token with its three outputs kept: -> (seq, i, nnew)"""

    def __init__(self):
        self.f = _fa2_lib.load().fa2_kvappend_varlen_token
        self.s, self.i, self.n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self.refs = (ctypes.byref(self.s), ctypes.byref(self.i), ctypes.byref(self.n))

    def __call__(self, cu, B, t):
        assert self.f(cu, B, t, *self.refs) == OK
        return self.s.value, self.i.value, self.n.value


def test_token_exhaustively_against_a_linear_scan():
    """B = 1 .. 9, every cu made of per-sequence counts in {0, 1, 2, 5} — leading, trailing and consecutive zero-length sequences among them — every t in
    [-1, cu[B] + 1]: the owner a linear scan finds (the one sequence with cu[s] <= t < cu[s + 1]), or none."""
    tok = _Token()
    f, refs, s_, i_, n_ = tok.f, tok.refs, tok.s, tok.i, tok.n
    seen = 0
    for B in range(1, 10):
        for counts in itertools.product((0, 1, 2, 5), repeat=B):
            cu = [0]
            owner = []                                           # the linear scan: sequence s owns the next counts[s] tokens
            for s, c in enumerate(counts):
                owner += [(s, i, c) for i in range(c)]
                cu.append(cu[-1] + c)
            arr = (ctypes.c_int * (B + 1))(*cu)
            for t in range(cu[-1]):
                f(arr, B, t, *refs)
                if (s_.value, i_.value, n_.value) != owner[t]:
                    raise AssertionError((cu, t, (s_.value, i_.value, n_.value), owner[t]))
            for t in (-1, cu[-1], cu[-1] + 1):
                assert f(arr, B, t, *refs) == OK and (s_.value, i_.value, n_.value) == (-1, 0, 0), (cu, t)
            seen += 1
    assert seen == sum(4 ** b for b in range(1, 10))
    assert _fa2_lib.kvappend_varlen_token([0, 0, 3, 3, 4], 3) == (3, 0, 1) and _fa2_lib.kvappend_varlen_token([0, 0, 3, 3, 4], 4) is None
    assert _fa2_lib.kvappend_varlen_token([2, 5], 1) is None and _fa2_lib.kvappend_varlen_token([2, 5], 2) == (0, 0, 3)


HOSTILE = [      # fixed arrays the GPU test feeds to the kernel, too (tests/test_kvappend_varlen_gpu.py)
    [40, 30, 20, 10, 0],                       # decreasing
    [0, -5, 7, -2, 12],                        # negative entries between valid ones
    [-8, -3, 4, 9, 20],                        # a negative start
    [0, 6, INT_MAX, 9, 14],                    # INT_MAX in the middle
    [5, 5, 5, 5, 5],                           # all equal
    [0, 9, 3, 12, 400],                        # not ascending, an end far above total
    [INT_MIN, INT_MAX, INT_MIN, INT_MAX, 3],   # the extremes
    [3, 0, 8, 8, 2],
]


def _consistent(cu, t, got):
    s, i, n = got
    B = len(cu) - 1
    if s == -1:
        return (i, n) == (0, 0)
    return 0 <= s < B and cu[s] <= t < cu[s + 1] and i == t - cu[s] and n == cu[s + 1] - cu[s] and 0 <= i < n


def test_token_on_hostile_arrays():
    """Decreasing, negative, INT_MAX, all equal and 300 random int32 arrays: the answer is always "no sequence" or a consistent (seq, i, nnew) — never an
    index out of range.  (The function reads cu[0 .. B] alone whatever they hold: csrc/fa2_decode.hip.h has the argument.)"""
    tok = _Token()
    g = np.random.default_rng(20251)
    arrays = [list(a) for a in HOSTILE]
    for n in range(300):
        B = int(g.integers(1, 40))
        kind = n % 3
        if kind == 0:
            a = g.integers(INT_MIN, INT_MAX, B + 1, endpoint=True)
        elif kind == 1:
            a = g.integers(-20, 60, B + 1)
        else:                                                    # ascending with a few entries spoilt
            a = np.sort(g.integers(0, 200, B + 1))
            a[g.integers(0, B + 1, 2)] = g.integers(-300, 300, 2)
        arrays.append([int(x) for x in a])
    named = 0
    for cu in arrays:
        B = len(cu) - 1
        arr = (ctypes.c_int * (B + 1))(*cu)
        ts = {-1, 0, 1, INT_MAX, INT_MAX + 1, INT_MIN, 2 ** 40, -2 ** 40}
        for c in cu:
            ts.update((c - 1, c, c + 1))
        if max(abs(c) for c in cu) < 1000:
            ts.update(range(min(cu) - 1, max(cu) + 2))
        for t in sorted(ts):
            got = tok(arr, B, t)
            assert _consistent(cu, t, got), (cu, t, got)
            named += got[0] >= 0
    assert named > 1000, "the property was exercised on tokens that are owned"
    # a token an ascending array would give to a sequence is never given to another one
    assert tok((ctypes.c_int * 5)(0, 9, 3, 12, 400), 4, 10) in ((-1, 0, 0), (2, 7, 9))
    lib = _fa2_lib.load()
    one = ctypes.c_int()
    r = ctypes.byref(one)
    arr = (ctypes.c_int * 2)(0, 1)
    assert lib.fa2_kvappend_varlen_token(None, 1, 0, r, r, r) == NULLP and lib.fa2_kvappend_varlen_token(arr, 1, 0, None, r, r) == NULLP
    assert lib.fa2_kvappend_varlen_token(arr, 1, 0, r, None, r) == NULLP and lib.fa2_kvappend_varlen_token(arr, 1, 0, r, r, None) == NULLP
    assert lib.fa2_kvappend_varlen_token(arr, 0, 0, r, r, r) == SHAPE and lib.fa2_kvappend_varlen_token(arr, -1, 0, r, r, r) == SHAPE


# ---------------------------------------------------------------------------------------------------------------- the C-ABI's checks
P = dc.HOST                                  # 16-byte aligned host memory that no call here ever touches
S2, S3 = _fa2_lib.strides2, _fa2_lib.strides3
DEFAULTS = dict(dtype=F16, fmt=C16, kn=P, vn=P, k=P, v=P, cu=P, lens=P, bt=None, B=2, total=5, Hkv=2, D=128, cap=256, page=0, pages=0, kns=S2(128, 256),
                vns=S2(128, 256), ks=S3(256 * 256, 128, 256), vs=S3(256 * 256, 128, 256), bts=0, q=None, qo=None, H=0, qs=None, qos=None, cos=None, sin=None,
                rdt=F32, rot=0, sro=0, ros=0, inter=1, kd=None, vd=None, ds=None)
BIG = dict(total=2 ** 31)                    # the defect of the LAST class: a well-formed call that carries it got past every other check


def _call(**kw):
    """fa2_kvcache_append_varlen on host memory that is never touched: every call here returns before a launch."""
    return dc.host_call("append_varlen", DEFAULTS, **kw)


def _rotary(**kw):
    return dict(dict(cos=P, sin=P, rdt=F32, rot=64, sro=16, ros=32), **kw)


def _with_q(**kw):
    a = _rotary(q=P, qo=P, H=8, qs=S2(128, 1024), qos=S2(128, 1024))
    a.update(kw)
    return a


def test_every_error_code():
    p = P
    assert _call(**BIG) == GRID and _call(**_with_q(**BIG)) == GRID and _call(fmt=C8, kd=p, vd=p, ds=S2(2, 1), **BIG) == GRID
    assert _call(total=2 ** 31 - 1, Hkv=1 << 20, D=512) == GRID                                  # blockIdx.y
    for name in ("kn", "vn", "k", "v", "cu", "lens", "kns", "vns", "ks", "vs"):
        assert _call(**{name: None}) == NULLP, name
    assert _call(page=64, pages=4, bt=None) == NULLP
    for name in ("q", "qo", "qs", "qos"):
        assert _call(**_with_q(**{name: None})) == NULLP, name
    assert _call(**_rotary(cos=None)) == NULLP and _call(**_rotary(sin=None)) == NULLP
    assert _call(fmt=C8, kd=p, ds=None) == NULLP and _call(fmt=C8, vd=p, ds=None) == NULLP
    for kw in (dict(B=0), dict(Hkv=0), dict(total=-1), dict(D=0), dict(cap=0), dict(page=48, pages=4, bt=p), dict(page=-64, pages=4, bt=p),
               dict(page=64, pages=0, bt=p), dict(page=1 << 20, cap=1 << 12, pages=4, bt=p), _with_q(H=0), _with_q(H=7), _with_q(cos=None, sin=None),
               _rotary(sro=0), _rotary(ros=-32), dict(fmt=C8, kd=p, ds=S2(-2, 1)), dict(fmt=C8, vd=p, ds=S2(2, -1))):
        assert _call(**kw) == SHAPE, kw
    for kw in (dict(D=60), dict(D=520), dict(D=1024), dict(fmt=C8, D=72), _rotary(rot=0), _rotary(rot=8), _rotary(rot=24), _rotary(rot=144), _rotary(rot=-16)):
        assert _call(**kw) == HEAD_DIM, kw
    assert _call(D=72, kns=S2(72, 144), vns=S2(72, 144), **BIG) == GRID                           # a multiple of 8 serves a 16-bit cache
    for kw in (dict(kn=p + 8), dict(vn=p + 8), dict(k=p + 8), dict(v=p + 4), dict(cu=p + 2), dict(cu=p + 1), dict(lens=p + 2), dict(page=64, pages=4, bt=p + 2),
               dict(kns=S2(132, 256)), dict(vns=S2(128, 0)), dict(kns=S2(-128, 256)), dict(ks=S3(65536, 128, 260)), dict(vs=S3(-65536, 128, 256)),
               dict(page=64, pages=4, bt=p, bts=-4), dict(fmt=C8, ks=S3(65536 + 8, 128, 256)), dict(fmt=C8, vs=S3(65536, 136, 256)),
               dict(fmt=C8, kd=p + 2, ds=S2(2, 1)), dict(fmt=C8, vd=p + 1, ds=S2(2, 1)), _with_q(q=p + 8), _with_q(qo=p + 8), _with_q(qs=S2(132, 1024)),
               _with_q(qos=S2(128, -1024)), _rotary(cos=p + 8), _rotary(sin=p + 4), _rotary(ros=34), _rotary(rdt=F16, ros=36)):
        assert _call(**kw) == ALIGN, kw
    assert _call(**_rotary(ros=36, **BIG)) == GRID                                                  # f32 rows: multiples of 4 elements
    for kw in (dict(dtype=2), dict(dtype=-1), dict(fmt=2), dict(fmt=-1), _rotary(rdt=BF16), _rotary(rdt=3), dict(kd=p, ds=S2(2, 1)), dict(vd=p, ds=S2(2, 1))):
        assert _call(**kw) == DTYPE, kw
    assert _call(dtype=BF16, **_rotary(rdt=BF16, **BIG)) == GRID


def test_an_empty_token_buffer_is_success_without_a_launch():
    """total = 0 passes the checks and returns FA2_OK: the pointers are host memory, so a launch would not have."""
    assert _call(total=0) == OK and _call(**_with_q(total=0)) == OK and _call(fmt=C8, kd=P, ds=S2(2, 1), total=0) == OK
    assert _call(total=0, cu=None) == NULLP and _call(total=0, D=60) == HEAD_DIM and _call(total=0, dtype=9) == DTYPE      # ... the checks still run


def test_error_precedence():
    """null pointer, sizes, head dim / rotary_dim, alignment, dtype, grid — fa2_kvcache_append's order: a call with two defects reports the earlier."""
    defects = [(NULLP, dict(cu=None)), (SHAPE, dict(B=0)), (HEAD_DIM, dict(D=60)), (ALIGN, dict(lens=P + 2)), (DTYPE, dict(dtype=7)), (GRID, BIG)]
    for i, (code, kw) in enumerate(defects):
        assert _call(**kw) == code
        for (_, later) in defects[i + 1:]:
            assert _call(**dict(later, **kw)) == code, (kw, later)
    rot = [(NULLP, dict(sin=None)), (SHAPE, dict(sro=0)), (HEAD_DIM, dict(rot=24)), (ALIGN, dict(ros=34)), (DTYPE, dict(rdt=BF16))]
    for i, (code, kw) in enumerate(rot):
        assert _call(**_rotary(**kw)) == code
        for (_, later) in rot[i + 1:]:
            assert _call(**_rotary(**dict(later, **kw))) == code, (kw, later)


# ---------------------------------------------------------------------------------------------------------------- the operator
def _args(total=10, H=4, Hkv=2, D=64, dt=torch.float16, cache=torch.float16, page=64):
    q = torch.zeros(total, H, D, dtype=dt)
    kc = torch.zeros(6, page, Hkv, D, dtype=torch.float16).to(dt).to(cache)
    k, v = (torch.zeros(total, Hkv, D, dtype=dt) for _ in range(2))
    cu = torch.tensor([0, 4, total], dtype=torch.int32)
    lens = torch.tensor([70, 100], dtype=torch.int32)
    bt = torch.zeros(2, 3, dtype=torch.int32)
    return q, kc, kc.clone(), k, v, cu, lens, bt


def test_operator_argument_checks():
    """Raised before any device work: CPU tensors reach the checks."""
    q, kc, vc, k, v, cu, lens, bt = _args()
    cos, sin = torch.ones(16, 16), torch.zeros(16, 16)
    # prefill: rotary without k / v, one of k / v alone, a k of another length, an e4m3 cache
    with pytest.raises(ValueError, match="rotary without an append"):
        flash_attention_prefill(q, kc, vc, cu, lens, bt, rotary_cos=cos, rotary_sin=sin)
    with pytest.raises(ValueError, match="rotary without an append"):
        flash_attention_prefill(q, kc, vc, cu, lens, bt, rotary_sin=sin)
    with pytest.raises(ValueError, match="k and v together"):
        flash_attention_prefill(q, kc, vc, cu, lens, bt, k=k)
    with pytest.raises(ValueError, match="k and v together"):
        flash_attention_prefill(q, kc, vc, cu, lens, bt, v=v)
    with pytest.raises(ValueError, match=r"k.shape\[0\] == total_q"):
        flash_attention_prefill(q, kc, vc, cu, lens, bt, k=k[:9], v=v[:9])
    with pytest.raises(ValueError, match="k and v together"):
        flash_attention_prefill(q, kc, vc, cu, lens, bt, k=k.bfloat16(), v=v.bfloat16())
    with pytest.raises(ValueError, match="k and v together"):
        flash_attention_prefill(q, kc, vc, cu, lens, bt, k=k, v=v[:9], max_seqlen_q=6)
    with pytest.raises(ValueError, match="flash_attention_prefill.*16-bit caches only"):
        flash_attention_prefill(q, kc.to(E4M3), vc.to(E4M3), cu, lens, bt, k=k, v=v, rotary_cos=cos, rotary_sin=sin)
    for bad in (torch.ones(16, 12), torch.ones(16, 40)):
        with pytest.raises(ValueError, match="multiple of 16"):
            flash_attention_prefill(q, kc, vc, cu, lens, bt, k=k, v=v, rotary_cos=bad, rotary_sin=bad, max_seqlen_q=6)
    # the packed append itself
    with pytest.raises(ValueError, match="k / v \\[total, Hkv, D\\]"):
        kvcache_append_varlen(kc, vc, k[None], v[None], cu, lens, bt)
    with pytest.raises(ValueError, match="one shape and dtype"):
        kvcache_append_varlen(kc, vc, k, v[:, :1], cu, lens, bt)
    with pytest.raises(ValueError, match="inconsistent"):
        kvcache_append_varlen(kc, vc[..., :32], k, v, cu, lens, bt)
    with pytest.raises(ValueError, match="nothing to do"):
        kvcache_append_varlen(kc, vc, k, v, cu, lens, bt, q=q)
    with pytest.raises(ValueError, match="Hkv dividing H"):
        kvcache_append_varlen(kc, vc, k, v, cu, lens, bt, rotary_cos=cos, rotary_sin=sin, q=q[:, :3])
    with pytest.raises(ValueError, match="Hkv dividing H"):
        kvcache_append_varlen(kc, vc, k, v, cu, lens, bt, rotary_cos=cos, rotary_sin=sin, q=q[:9])
    with pytest.raises(ValueError, match="come together"):
        kvcache_append_varlen(kc, vc, k, v, cu, lens, bt, rotary_cos=cos)
    with pytest.raises(ValueError, match="share one dtype"):
        kvcache_append_varlen(kc, vc, k, v, cu, lens, bt, rotary_cos=cos, rotary_sin=sin.half())
    with pytest.raises(ValueError, match="cu_seqlens must be"):
        kvcache_append_varlen(kc, vc, k, v, cu.long(), lens, bt)
    with pytest.raises(ValueError, match="cu_seqlens must be"):
        kvcache_append_varlen(kc, vc, k, v, cu[:1], lens, bt)
    with pytest.raises(ValueError, match=r"cache_seqlens must be .* \[B\] = \[2\]"):
        kvcache_append_varlen(kc, vc, k, v, cu, torch.ones(3, dtype=torch.int32), bt)
    with pytest.raises(ValueError, match="block_table must be int32"):
        kvcache_append_varlen(kc, vc, k, v, cu, lens, bt[:1])
    with pytest.raises(ValueError, match="descale.*float8_e4m3fn caches"):
        kvcache_append_varlen(kc, vc, k, v, cu, lens, bt, k_descale=torch.ones(2, 2))
    with pytest.raises(ValueError, match=r"\[B, Hkv\] = \[2, 2\]"):
        kvcache_append_varlen(kc.to(E4M3), vc.to(E4M3), k, v, cu, lens, bt, k_descale=torch.ones(10, 2))
    q9, kc9, vc9, k9, v9 = _args(D=100)[:5]
    with pytest.raises(ValueError, match="multiples of 8"):
        kvcache_append_varlen(kc9, vc9, k9, v9, cu, lens, bt)
    q8, kc8, vc8, k8, v8 = _args(D=72, cache=E4M3)[:5]
    with pytest.raises(ValueError, match="multiples of 8"):
        kvcache_append_varlen(kc8, vc8, k8, v8, cu, lens, bt)
    with pytest.raises(ValueError, match="e5m2 and the fnuz formats"):
        kvcache_append_varlen(kc.to(torch.float8_e5m2), vc.to(torch.float8_e5m2), k, v, cu, lens, bt)
    # everything in order: only the device is missing
    with pytest.raises(RuntimeError, match="ROCm device"):
        kvcache_append_varlen(kc, vc, k, v, cu, lens, bt, rotary_cos=cos, rotary_sin=sin, q=q)
    with pytest.raises(RuntimeError, match="ROCm device"):
        flash_attention_prefill(q, kc, vc, cu, lens, bt, k=k, v=v, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=False, max_seqlen_q=6)


def _prefill_args_of_the_parent(q, kc, vc, cu, lens, bt, max_q, o_ptr, lse_ptr):
    """The one C call flash_attention_prefill made before it had the five keywords, argument for argument (o and lse are allocated by the call)."""
    total, H, D = q.shape
    hr = lambda t: (t.stride(1), t.stride(0))                   # noqa: E731
    bnhd = lambda t: (t.stride(0), t.stride(2), t.stride(1))    # noqa: E731
    return dc.c_args("prefill", dtype=F16, fmt=C16, q=q.data_ptr(), k=kc.data_ptr(), v=vc.data_ptr(), o=o_ptr, lse=lse_ptr, cu=cu.data_ptr(), lens=lens.data_ptr(),
                     bt=bt.data_ptr(), B=2, H=H, Hkv=kc.shape[2], max_q=max_q, D=D, cap=bt.shape[1], page=kc.shape[1], pages=kc.shape[0], qs=hr(q), ks=bnhd(kc),
                     vs=bnhd(vc), os=(D, H * D), lss=total, bts=bt.stride(0), scale=float(D ** -0.5), wl=-1, cap_=0.0, sl=None, st=0, stream=None)


def _plain(a):
    return tuple(tuple(x) if isinstance(x, ctypes.Array) else x for x in a)


def test_the_prefill_call_without_the_keywords_is_the_parents(monkeypatch):
    rec = dc.recording_lib(monkeypatch)
    q, kc, vc, k, v, cu, lens, bt = _args()
    o = flash_attention_prefill(q, kc, vc, cu, lens, bt, max_seqlen_q=6)
    assert [name for name, _ in rec.calls] == ["fa2_fwd_prefill"]
    a = rec.calls[0][1]
    lse_ptr = dc.arg("prefill", a, "lse")
    assert _plain(a) == _prefill_args_of_the_parent(q, kc, vc, cu, lens, bt, 6, o.data_ptr(), lse_ptr) and lse_ptr not in (None, 0)


def test_the_fused_prefill_appends_then_attends_on_the_rotated_q(monkeypatch):
    rec = dc.recording_lib(monkeypatch)
    q, kc, vc, k, v, cu, lens, bt = _args()
    cos, sin = torch.ones(16, 16), torch.zeros(16, 16)
    arg = lambda a, n: dc.arg("append_varlen", a, n)            # noqa: E731
    flash_attention_prefill(q, kc, vc, cu, lens, bt, max_seqlen_q=6, k=k, v=v)          # no rotary: q is not touched and not passed
    (n1, a1), (n2, a2) = rec.calls
    assert (n1, n2, len(a1)) == ("fa2_kvcache_append_varlen", "fa2_fwd_prefill", 37) and dc.arg("prefill", a2, "q") == q.data_ptr()
    assert [arg(a1, n) for n in ("q", "qo", "rot", "H")] == [None, None, 0, 0]
    assert [arg(a1, n) for n in ("kn", "vn", "k", "v", "cu", "lens", "bt", "B", "total", "Hkv", "D", "cap", "page", "pages")] == \
        [k.data_ptr(), v.data_ptr(), kc.data_ptr(), vc.data_ptr(), cu.data_ptr(), lens.data_ptr(), bt.data_ptr(), 2, 10, 2, 64, 3, 64, 6]
    assert tuple(arg(a1, "kns")) == (64, 128) and tuple(arg(a1, "ks")) == (64 * 2 * 64, 64, 128)
    del rec.calls[:]
    flash_attention_prefill(q, kc, vc, cu, lens, bt, max_seqlen_q=6, k=k, v=v, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=False)
    (n1, a1), (n2, a2) = rec.calls
    assert (n1, n2) == ("fa2_kvcache_append_varlen", "fa2_fwd_prefill")
    assert arg(a1, "q") == q.data_ptr() and arg(a1, "qo") not in (None, q.data_ptr()) and dc.arg("prefill", a2, "q") == arg(a1, "qo"), "prefill reads the rotated q"
    assert [arg(a1, n) for n in ("rot", "H", "sro", "ros", "inter", "rdt")] == [32, 4, 16, 16, 0, F32] and tuple(arg(a1, "qs")) == (64, 256)
    del rec.calls[:]
    assert kvcache_append_varlen(kc, vc, k, v, cu, lens, bt) is None and [n for n, _ in rec.calls] == ["fa2_kvcache_append_varlen"]
    del rec.calls[:]
    assert kvcache_append_varlen(kc, vc, k[:0], v[:0], cu, lens, bt) is None and rec.calls == [], "an empty token buffer: no call"
