"""The float64 rotary reference and its error bar, shared by tests/test_kvappend.py (the host side, fa2_rotary_eval) and tests/test_kvappend_gpu.py (the
kernel).  Plain CPU code: nothing here touches a device."""
import torch


def rotary_ref64(x, cos, sin, rot, inter):
    """float64 rotation of rows x [..., D] by table rows cos / sin [..., rot / 2] (float64 in, float64 out) -> (y, |x1| + |x2| per column)."""
    y, mag = x.clone(), torch.zeros_like(x)
    half = rot // 2
    i1 = torch.arange(half) * 2 if inter else torch.arange(half)
    i2 = i1 + 1 if inter else i1 + half
    x1, x2 = x[..., i1], x[..., i2]
    y[..., i1] = x1 * cos - x2 * sin
    y[..., i2] = x1 * sin + x2 * cos
    mag[..., i1] = mag[..., i2] = x1.abs() + x2.abs()
    return y, mag


E4M3 = torch.float8_e4m3fn


def rotary_f32(x, cos, sin, rot, inter):
    """The append's own arithmetic (csrc/fa2_rotary.h) on rows x [..., D] of 16-bit values and table rows cos / sin [..., rot / 2] (f32 or 16-bit, upcast
    exactly): y1 = fma(x1, c, -(x2 s)), y2 = fma(x1, s, x2 c) -> f32 [..., D], the columns at or beyond rot unchanged.  The products x2 s and x2 c are
    rounded to f32; x1 c and x1 s are exact in float64 (at most 11 + 24 bits), so the float64 sum rounded to f32 is the fma's result (but for a double
    rounding that needs a float64 sum an f32 half step away from exact: never seen; tests/test_fuzz_decode.py holds this to fa2_rotary_eval's bits)."""
    xf, c, s = x.float(), cos.float(), sin.float()
    half = rot // 2
    i1 = torch.arange(half) * 2 if inter else torch.arange(half)
    i2 = i1 + 1 if inter else i1 + half
    x1, x2 = xf[..., i1], xf[..., i2]
    y = xf.clone()
    y[..., i1] = (x1.double() * c.double() - (x2 * s).double()).float()
    y[..., i2] = (x1.double() * s.double() + (x2 * c).double()).float()
    return y


def quantise(y, d=None):
    """rne_e4m3(clamp(y / descale, +-448)) of f32 y [B, n, heads, D] with d [B, heads] or None (1.0): torch's CPU division and cast, both round to nearest even"""
    y = y if d is None else y / d.float()[:, None, :, None]
    return y.clamp(-448.0, 448.0).to(E4M3)


def targets(lens, nnew, capacity_keys):
    """[(b, i, p)] of the new tokens that are written: p = len - Nnew + i inside [0, capacity_keys)"""
    return [(b, i, int(n) - nnew + i) for b, n in enumerate(lens) for i in range(nnew) if 0 <= int(n) - nnew + i < capacity_keys]


def append_rows(k, v, lens, q=None, cos=None, sin=None, inter=True, fp8=False, kd=None, vd=None):
    """What fa2_kvcache_append stores for new tokens k / v [B, Nnew, Hkv, D] (16-bit) under the lengths AFTER the append: (K rows, V rows, rotated q or
    None) in the cache format.  Token i of sequence b is rotated by table row clamp(len_b - Nnew + i, 0, seqlen_ro - 1) (q row i too, whether or not the
    token is written); 16-bit cache: one rounding of the f32 value (V, and K without tables: the source bits); e4m3: quantise() of the f32 value."""
    nnew, dt = k.shape[1], k.dtype
    yk, q_rot = k.float(), None
    if cos is not None:
        rot = 2 * cos.shape[1]
        pos = (torch.as_tensor(list(lens), dtype=torch.int64)[:, None] - nnew + torch.arange(nnew)[None, :]).clamp(0, cos.shape[0] - 1)
        c, s = cos[pos][:, :, None, :], sin[pos][:, :, None, :]
        yk = rotary_f32(k, c, s, rot, inter)
        if q is not None:
            q_rot = rotary_f32(q, c, s, rot, inter).to(dt)
    if fp8:
        return quantise(yk, kd), quantise(v.float(), vd), q_rot
    return yk.to(dt), v.clone(), q_rot


def rotary_bar(ref, mag, dt):
    """One rounding of an f32 value to the destination (relative 2^-11 fp16, 2^-8 bf16), the f32 arithmetic (two roundings of 2^-24 on terms of
    magnitude at most |x1| + |x2|, with slack: 2^-22), and the subnormal floor of the destination (half a step: 2^-25 fp16, 2^-134 bf16)."""
    rel, floor = (2.0 ** -11, 2.0 ** -25) if dt == torch.float16 else (2.0 ** -8, 2.0 ** -134)
    return rel * ref.abs() + 2.0 ** -22 * mag + floor
