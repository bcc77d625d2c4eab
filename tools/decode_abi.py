"""The C argument order of the serving entries, for the tests and the tools alike: fa2_fwd_decode, fa2_fwd_decode_fp8, fa2_fwd_decode_window,
fa2_fwd_decode_mla, fa2_kvcache_append, fa2_kvcache_append_varlen, fa2_kvcache_append_mla, fa2_kvcache_append_mla_varlen, fa2_fwd_prefill and
fa2_fwd_prefill_fp8 by keyword (ENTRIES, c_args: the only copy under tests/ and
tools/), what the tensors of a decode call say (tensor_kw) and the GPU call on NaN-filled outputs and workspace (decode_c).  tests/decode_calls.py hands
these on to the tests beside what only tests need; the tools import them here, so that a tool runs with nothing but itself, this file and the package."""
import ctypes

import torch

from rocwmma_fattn import _fa2_lib

F16, BF16, E4M3 = torch.float16, torch.bfloat16, torch.float8_e4m3fn


def code(dt):
    return _fa2_lib.FA2_DTYPE_F16 if dt == F16 else _fa2_lib.FA2_DTYPE_BF16


def s3(t):
    """{batch | page, head, row} element strides of a [B, N, heads, D] tensor."""
    return _fa2_lib.strides3(t.stride(0), t.stride(2), t.stride(1))


def s2(t):
    return _fa2_lib.strides2(t.stride(0), t.stride(1))


def nan_out(q):
    B, Nq, H, D = q.shape
    return (torch.full((B, Nq, H, D), float("nan"), dtype=q.dtype, device=q.device), torch.full((B, H, Nq), float("nan"), dtype=torch.float32, device=q.device))


def same_bits(a, b):
    """(o, lse) pairs: the O bits and the LSE values"""
    return torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------- the C argument order
_HEAD = ("q", "k", "v", "o", "lse", "lens", "bt", "B", "H", "Hkv", "Nq", "D", "cap", "page", "pages", "qs", "ks", "vs", "os", "ls", "bts", "scale")
_DESCALES = ("kd", "vd", "ds")
_TAIL = ("ns", "ws", "wsb", "stream")
_SCOREMOD = ("wl", "cap_", "sl", "st")
_PREFILL_HEAD = ("q", "k", "v", "o", "lse", "cu", "lens", "bt", "B", "H", "Hkv", "max_q", "D", "cap", "page", "pages", "qs", "ks", "vs", "os", "lss", "bts",
                 "scale")         # (qs, os: {head, row} pairs of packed tensors; lss: the one head stride of lse [H, total_q])
ENTRIES = {      # entry -> (symbol, its arguments by keyword, its workspace query)
    "plain": ("fa2_fwd_decode", ("dtype",) + _HEAD + _TAIL, "fa2_fwd_decode_workspace_bytes"),
    "fp8": ("fa2_fwd_decode_fp8", ("dtype",) + _HEAD + _DESCALES + _TAIL, "fa2_fwd_decode_fp8_workspace_bytes"),
    "window": ("fa2_fwd_decode_window", ("dtype", "fmt") + _HEAD + _DESCALES + _SCOREMOD + _TAIL, "fa2_fwd_decode_window_workspace_bytes"),
    "append": ("fa2_kvcache_append", ("dtype", "fmt", "kn", "vn", "k", "v", "lens", "bt", "B", "Hkv", "N", "D", "cap", "page", "pages", "kns", "vns", "ks", "vs", "bts",
                                      "q", "qo", "H", "Nq", "qs", "qos", "cos", "sin", "rdt", "rot", "sro", "ros", "inter") + _DESCALES + ("stream",), None),
    "append_varlen": ("fa2_kvcache_append_varlen", ("dtype", "fmt", "kn", "vn", "k", "v", "cu", "lens", "bt", "B", "total", "Hkv", "D", "cap", "page", "pages", "kns", "vns",
                                                    "ks", "vs", "bts", "q", "qo", "H", "qs", "qos", "cos", "sin", "rdt", "rot", "sro", "ros", "inter") + _DESCALES +
                      ("stream",), None),
    # decode on a latent (MLA) cache: k is the one latent tensor, D / Dv the 576 / 512 columns; no Hkv, no v, no vs
    "mla": ("fa2_fwd_decode_mla", ("dtype", "q", "k", "o", "lse", "lens", "bt", "B", "H", "Nq", "D", "Dv", "cap", "page", "pages", "qs", "ks", "os", "ls", "bts",
                                   "scale") + _TAIL, "fa2_fwd_decode_mla_workspace_bytes"),
    # ... and its append: kn / vn are kv_c / k_pe (kns / vns: their {batch, row} pairs; packed: one row stride each), k the one latent tensor
    "append_mla": ("fa2_kvcache_append_mla", ("dtype", "kn", "vn", "k", "lens", "bt", "B", "N", "D", "Dv", "cap", "page", "pages", "kns", "vns", "ks", "bts", "q", "qo",
                                              "H", "Nq", "qs", "qos", "cos", "sin", "rdt", "rot", "sro", "ros", "inter", "stream"), None),
    "append_mla_varlen": ("fa2_kvcache_append_mla_varlen", ("dtype", "kn", "vn", "k", "cu", "lens", "bt", "B", "total", "D", "Dv", "cap", "page", "pages", "kns", "vns",
                                                            "ks", "bts", "q", "qo", "H", "qs", "qos", "cos", "sin", "rdt", "rot", "sro", "ros", "inter", "stream"), None),
    "prefill": ("fa2_fwd_prefill", ("dtype", "fmt") + _PREFILL_HEAD + _SCOREMOD + ("stream",), None),
    "prefill_fp8": ("fa2_fwd_prefill_fp8", ("dtype",) + _PREFILL_HEAD + _DESCALES + _SCOREMOD + ("stream",), None),
}
_ABSENT = dict(kd=None, vd=None, ds=None, wl=-1, cap_=0.0, sl=None, st=0)      # what an entry without the argument computes with
_FORMAT = {"plain": _fa2_lib.FA2_CACHE_16BIT, "fp8": _fa2_lib.FA2_CACHE_E4M3, "prefill_fp8": _fa2_lib.FA2_CACHE_E4M3}   # ... and the cache format it serves


def c_args(entry, **kw):
    """The argument tuple of the named entry from keyword values.  A keyword the entry does not take must hold the value the entry computes with."""
    order = ENTRIES[entry][1]
    for n in set(kw) - set(order):
        assert kw[n] == (_FORMAT[entry] if n == "fmt" else _ABSENT[n]), "%s does not take %s = %r" % (ENTRIES[entry][0], n, kw[n])
    return tuple(kw[n] for n in order)


def arg(entry, args, name):
    """the named argument out of a tuple in the entry's order"""
    return args[ENTRIES[entry][1].index(name)]


def call(entry, **kw):
    """the entry of the loaded library on c_args(entry, **kw) -> its return code"""
    return getattr(_fa2_lib.load(), ENTRIES[entry][0])(*c_args(entry, **kw))


def _ptr(t):
    return None if t is None else t.data_ptr()


def tensor_kw(q, k, v, o, lse, lens, block_table=None, kd=None, vd=None, scale=None):
    """What the tensors of a decode call say: pointers, sizes, strides, the cache format, the default scale.  A block table makes k / v a pool."""
    B, Nq, H, D = q.shape
    cap, page, pages = (k.shape[1], 0, 0) if block_table is None else (block_table.shape[1], k.shape[1], k.shape[0])
    d0 = kd if kd is not None else vd
    assert kd is None or vd is None or kd.stride() == vd.stride()
    return dict(dtype=code(q.dtype), fmt=_fa2_lib.FA2_CACHE_E4M3 if k.dtype == E4M3 else _fa2_lib.FA2_CACHE_16BIT, q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(),
                o=o.data_ptr(), lse=lse.data_ptr(), lens=lens.data_ptr(), bt=_ptr(block_table), B=B, H=H, Hkv=k.shape[2], Nq=Nq, D=D, cap=cap, page=page, pages=pages,
                qs=s3(q), ks=s3(k), vs=s3(v), os=s3(o), ls=s2(lse), bts=0 if block_table is None else block_table.stride(0), scale=D ** -0.5 if scale is None else scale,
                kd=_ptr(kd), vd=_ptr(vd), ds=None if d0 is None else s2(d0))


def decode_c(entry, q, k, v, lens, num_splits, window_left=-1, softcap=0.0, slopes=None, *, block_table=None, kd=None, vd=None, o=None, lse=None, scale=None,
             check=True):
    """The named decode entry with NaN-filled outputs and a NaN-filled workspace sized by the entry's own query: every element the contract names must be
    written, nothing unwritten read.  -> (o, lse); check=False: (return code, o, lse) instead of raising."""
    no, nl = nan_out(q)
    o, lse = no if o is None else o, nl if lse is None else lse
    kw = tensor_kw(q, k, v, o, lse, lens, block_table, kd, vd, scale)
    sizes = [kw[n] for n in ("dtype", "B", "H", "Hkv", "Nq", "D", "cap", "page")] + [num_splits] + ([window_left] if entry == "window" else [])
    need = getattr(_fa2_lib.load(), ENTRIES[entry][2])(*sizes)
    ws = torch.full((max(need, 16) // 4,), float("nan"), dtype=torch.float32, device=q.device)
    rc = call(entry, **kw, wl=window_left, cap_=softcap, sl=_ptr(slopes), st=0 if slopes is None or slopes.dim() == 1 else slopes.stride(0), ns=num_splits,
              ws=ws.data_ptr() if need else None, wsb=need, stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if check:
        _fa2_lib.check(rc)
    torch.cuda.synchronize()
    return (o, lse) if check else (rc, o, lse)
