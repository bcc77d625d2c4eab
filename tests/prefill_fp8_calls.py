"""The fp8 side of the prefill tests (tests/test_prefill_fp8.py, test_prefill_fp8_gpu.py, test_prefill_fp8_far_gpu.py): fa2_fwd_prefill_fp8 through ctypes,
keys and values quantised to e4m3 under per (sequence, K / V head) descales, their exact dequantised values for the 16-bit twin and the float64 reference,
and the conversion of prefill_calls' NaN-filled 16-bit caches into e4m3 caches whose every dead slot holds the NaN code 0x7f.  The call layer and the
cache builders are prefill_calls', imported.  A plain module: nothing here touches a device until asked."""
import torch

import prefill_calls as pc
from rocwmma_fattn import _fa2_lib

E4M3 = torch.float8_e4m3fn
NAN_BYTE = 0x7F                                      # an e4m3 NaN code: what a 16-bit NaN converts to
POW2 = tuple(2.0 ** e for e in range(-3, 4))         # 1/8 .. 8: every finite e4m3 value times one of these is a f16 and a bf16 value


def prefill_fp8_c(q, kc, vc, cu, lens, bt, max_q, scale, kd=None, vd=None, window_left=-1, softcap=0.0, slopes=None, out=None, check=True):
    """fa2_fwd_prefill_fp8 on NaN-filled o / lse (or `out`) -> o [total_q, H, D], lse f32 [H, total_q] in log2 units.  kc / vc: e4m3 (strides = bytes)."""
    o, lse = out if out is not None else pc.nan_out(q)
    d0 = kd if kd is not None else vd
    rc = pc.decode_abi.call("prefill_fp8", **pc.prefill_kw(q, kc, vc, o, lse, cu, lens, bt, max_q, scale, window_left, softcap, slopes), kd=pc.ptr(kd), vd=pc.ptr(vd),
                            ds=None if d0 is None else _fa2_lib.strides2(d0.stride(0), d0.stride(1)))
    if check:
        _fa2_lib.check(rc)
        return o, lse
    return rc


def pow2_descales(B, Hkv, seed, device):
    """float32 [B, Hkv] drawn from POW2."""
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(POW2)[torch.randint(0, len(POW2), (B, Hkv), generator=g)].to(device)


def general_descales(B, Hkv, seed, device):
    """float32 [B, Hkv], different per sequence and head, between 0.37 and 2.9 (both occur)."""
    g = torch.Generator().manual_seed(seed)
    d = 0.37 + (2.9 - 0.37) * torch.rand((B, Hkv), generator=g)
    d.view(-1)[0], d.view(-1)[-1] = 0.37, 2.9
    return d.to(device)


def quantise(seqs, descale):
    """Per-sequence [len_s, Hkv, D] values under descale [B, Hkv] (None: ones) -> the e4m3 codes (x / descale).to(e4m3), as exact 16-bit tensors of the
    sequences' dtype (every e4m3 value is a f16 and a bf16 value)."""
    out = []
    for s, x in enumerate(seqs):
        d = descale[s].float()[None, :, None] if descale is not None else 1.0
        out.append((x.float() / d).to(E4M3).float().to(x.dtype))
    return out


def dequant(codes, descale):
    """The true keys / values float(code) * descale[s, hkv], float32 (exact: a 4-bit significand times a 24-bit one)."""
    return [c.float() * (descale[s].float()[None, :, None] if descale is not None else 1.0) for s, c in enumerate(codes)]


def to_e4m3(cache16):
    """A NaN-filled 16-bit cache that holds e4m3 values -> the e4m3 cache: exact, and every NaN becomes the code 0x7f."""
    c8 = cache16.to(E4M3)
    raw = c8.view(torch.uint8)
    assert bool(((raw == NAN_BYTE) == torch.isnan(cache16)).all()) and torch.equal(c8.float().nan_to_num(nan=0.0), cache16.float().nan_to_num(nan=0.0))
    return c8


def as_dtype(true, dtype):
    """The true values as the 16-bit twin's keys: exact when the descales are powers of two in POW2 (asserted)."""
    out = [t.to(dtype) for t in true]
    assert all(torch.equal(a.float(), t) for a, t in zip(out, true)), "the dequantised values are not exact in %s" % dtype
    return out


def make_case(lens, nqs, H, Hkv, D, dtype, seed, device, descales="pow2", prefix=True):
    """prefill_calls.make_inputs' N(0, 1) draw, quantised: q, cu, the descales kd / vd [B, Hkv] ("pow2", "general" or None), the codes kc / vc (lists of
    exact 16-bit tensors) and the true values kt / vt (float32 lists).  prefix: the first 192 keys of sequence 1 hold sequence 0's CODES (a shared
    physical page; the true values differ by the descales' ratio)."""
    q, cu, ks, vs = pc.make_inputs(lens, nqs, H, Hkv, D, dtype, seed, device)
    B = len(lens)
    if descales is None:
        kd = vd = None
    else:
        make = pow2_descales if descales == "pow2" else general_descales
        kd, vd = make(B, Hkv, seed + 100, device), make(B, Hkv, seed + 200, device).flip(0)
    kc, vc = quantise(ks, kd), quantise(vs, vd)
    if prefix and B > 1 and lens[0] >= 192 and lens[1] >= 192:
        kc[1][:192], vc[1][:192] = kc[0][:192], vc[0][:192]
    return dict(q=q, cu=cu, kd=kd, vd=vd, kc=kc, vc=vc, kt=dequant(kc, kd), vt=dequant(vc, vd), lens=tuple(lens), nqs=tuple(nqs))
