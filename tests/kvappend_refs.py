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


def rotary_bar(ref, mag, dt):
    """One rounding of an f32 value to the destination (relative 2^-11 fp16, 2^-8 bf16), the f32 arithmetic (two roundings of 2^-24 on terms of
    magnitude at most |x1| + |x2|, with slack: 2^-22), and the subnormal floor of the destination (half a step: 2^-25 fp16, 2^-134 bf16)."""
    rel, floor = (2.0 ** -11, 2.0 ** -25) if dt == torch.float16 else (2.0 ** -8, 2.0 ** -134)
    return rel * ref.abs() + 2.0 ** -22 * mag + floor
