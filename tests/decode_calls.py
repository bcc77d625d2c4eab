"""The one call layer of the decode and append tests: the C argument order and the GPU call on NaN-filled outputs and workspace (tools/decode_abi.py, which
the tools share: ENTRIES, c_args, decode_c and the small helpers, handed on here under their names), the CPU call on host memory that is never
touched (host_call), the paged-pool builder and the stand-in library of the operator tests.  A plain module, like decode_refs.py: no fixtures, and
nothing here touches a device until a caller asks for one."""
import contextlib
import ctypes
import os
import sys

import pytest
import torch

from conftest import ROOT
from rocwmma_fattn import FlashAttn, _fa2_lib

if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.append(os.path.join(ROOT, "tools"))
from decode_abi import E4M3, ENTRIES, arg, c_args, call, code, decode_c, nan_out, s2, s3, same_bits, tensor_kw  # noqa: E402,F401

NAN_BYTE = 0x7F                      # an e4m3 NaN code


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------------- CPU: calls that are refused
_HOST = ctypes.create_string_buffer(4096 + 16)
HOST = (ctypes.addressof(_HOST) + 15) & ~15          # 16-byte aligned host memory that no call here ever touches


def host_call(entry, defaults, **kw):
    """The named entry on `defaults` (a file's own well-formed call on HOST) with `kw` laid over them: refused before the launch -> the return code."""
    return call(entry, **dict(defaults, stream=None, **kw))


# ---------------------------------------------------------------------------------------------------------------- paged pools
def block_table(lens, per, page, g, spare=3, keep=None):
    """Shuffled physical pages for the used logical pages of each sequence, `spare` pages more, and entries that name one of the spare pages (a valid
    id) wherever a sequence has no page or keep(b, j) is False (a page the server freed).  -> table [B, per], pool size, [(b, j, page id)] in use"""
    used = [-(-n // page) for n in lens]
    total = sum(used) + spare
    order = torch.randperm(total, generator=g).tolist()
    bt = torch.full((len(lens), per), order[-1], dtype=torch.int32)
    placed, nxt = [], 0
    for b, u in enumerate(used):
        for j in range(u):
            if keep is None or keep(b, j):
                bt[b, j] = order[nxt]
                placed.append((b, j, order[nxt]))
            nxt += 1
    assert keep is None or len(placed) < sum(used), "keep freed nothing"
    return bt, total, placed


def paged(k, v, lens, page, g, spare=3, keep=None):
    """The [B, Nmax, Hkv, D] caches (16-bit or e4m3) scattered into pages in shuffled physical order.  Spare pages, pages no sequence uses and freed pages
    hold NaN (e4m3: 0x7f bytes), and the block-table entries without a page point at such a page.  -> pool K, pool V, block table"""
    raw = (lambda t: t.view(torch.uint8)) if k.dtype == E4M3 else (lambda t: t)
    bt, total, placed = block_table(lens, k.shape[1] // page, page, g, spare, keep)
    pools = []
    for t in (k, v):
        pool = torch.full((total, page) + tuple(t.shape[2:]), NAN_BYTE if t.dtype == E4M3 else float("nan"), dtype=raw(t).dtype)
        for b, j, pid in placed:
            pool[pid] = raw(t)[b, j * page:(j + 1) * page]
        pools.append(pool.view(t.dtype))
    return pools[0], pools[1], bt


# ---------------------------------------------------------------------------------------------------------------- the operator without a device
class _Recording:
    """Stands in for the loaded library: every call answers 0 and is kept as (symbol, arguments)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append((name, a))
            return 0
        return f


def recording_lib(monkeypatch):
    """CPU tensors claim a ROCm device and the operator's device plumbing is stubbed, so that a call reaches the library — which is the recorder."""
    rec = _Recording()
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(_fa2_lib, "load", lambda: rec)
    monkeypatch.setattr(FlashAttn, "_raw_stream", lambda dev: None)
    monkeypatch.setattr(FlashAttn, "_current_device", lambda: 0)
    monkeypatch.setattr(FlashAttn, "_workspace_unused", lambda dev, stream: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    return rec
