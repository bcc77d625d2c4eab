"""CPU tests of the score modifiers (logit soft-capping, ALiBi slopes): the shared arithmetic of csrc/fa2_scoremod.h through the library's host function
fa2_scoremod_eval against float64, the validation order of the four entry points, and the operator's argument errors.  Nothing here touches a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import flash_attention, flash_attention_varlen

ERR_SOFTCAP = -10


def evaluate(x, softcap, slope=0.0, pos=0, j=0):
    s, f = ctypes.c_float(), ctypes.c_float()
    assert _fa2_lib.load().fa2_scoremod_eval(x, softcap, slope, pos, j, ctypes.byref(s), ctypes.byref(f)) == 0
    return s.value, f.value


def ulp_of(x):
    return float(np.spacing(np.float32(x)))


@pytest.mark.parametrize("softcap", [0.5, 30.0, 50.0])
def test_softcap_against_float64(softcap):
    """s = softcap * tanh(x / softcap) over x / softcap in +-[1e-6, 1e3].  Bound on |s - s64|: 6 ulps of softcap.  The form 1 - 2 / (1 + e^2y) has an
    ABSOLUTE error in t of at most ~3 * 2^-24 wherever it is not saturated (the quotient 2 / (1 + e) is at most 2 and carries the roundings of the sum
    and of the division, half an ulp each, i.e. 2 * 2^-24 absolute; the final subtraction another 2^-24 at most), plus 0.45 * 2^-24 for each of the two
    roundings of the argument (x * (1 / softcap), then * 2 log2 e; y (1 - tanh^2 y) <= 0.45), plus 2^-24 for exp2f itself at e ~ 1: about 5 * 2^-24 in t.
    softcap in [2^k, 2^(k+1)) has an ulp of 2^(k-23), so softcap * 5 * 2^-24 is below 5 ulps of softcap, and the product's own rounding adds half of one.
    Measured maximum: 1.40 / 2.86 / 2.49 ulps at softcap 0.5 / 30 / 50 (printed below)."""
    cap32 = float(np.float32(softcap))
    ys = np.concatenate([np.logspace(-6, 3, 4001), -np.logspace(-6, 3, 4001)])
    worst = 0.0
    for y in ys:
        x = float(np.float32(y * cap32))
        s, f = evaluate(x, cap32)
        assert math.isfinite(s) and math.isfinite(f), (x, s, f)
        t64 = math.tanh(x / cap32)
        worst = max(worst, abs(s - cap32 * t64) / ulp_of(cap32))
        t32 = float(np.tanh(np.float32(x) / np.float32(cap32)))
        if abs(t32) == 1.0:                                 # float32 tanh is saturated (from |y| ~ 9.01 on): so is the library's, exactly, with a zero derivative factor
            assert s == math.copysign(cap32, x) and f == 0.0, (x, s, f)
        assert 0.0 <= f <= 1.0
        assert abs(f - (1.0 - t64 * t64)) <= 8 * 2.0 ** -24, (x, f)
    print("softcap %g: max |s - s64| = %.2f ulps of softcap (bound 6)" % (softcap, worst))
    assert worst <= 6.0


@pytest.mark.parametrize("softcap", [0.5, 30.0, 1e4, 1e6])
def test_softcap_is_relative_near_zero(softcap):
    """Below |x / softcap| = 1/8 the tanh is the odd series: |s - s64| is a few ulps of s ITSELF, not of softcap, so that a large softcap leaves the
    scores alone (the 1 - 2 / (1 + e^2y) form alone was 1e-3 off in every score at softcap = 1e4: tools/fuzz_lse.py's first runs).  Bound: 0.5 ulp for
    x * (1 / softcap) twice (the reciprocal, the product), 1.5 for the series' Horner steps and truncation (62 y^8 / 2835 <= 1.4e-9), 0.5 each for
    y * poly and softcap * t: 4 ulps of s.  The derivative factor stays within 8 * 2^-24 of 1 - tanh^2."""
    cap32 = float(np.float32(softcap))
    worst = 0.0
    for y in np.concatenate([np.logspace(-8, math.log10(0.1249), 2001), -np.logspace(-8, math.log10(0.1249), 2001)]):
        x = float(np.float32(y * cap32))
        s, f = evaluate(x, cap32)
        t64 = math.tanh(x / cap32)
        worst = max(worst, abs(s - cap32 * t64) / ulp_of(cap32 * t64))
        assert abs(f - (1.0 - t64 * t64)) <= 8 * 2.0 ** -24, (x, f)
    print("softcap %g: max |s - s64| = %.2f ulps of s below |y| = 1/8 (bound 4)" % (softcap, worst))
    assert worst <= 4.0


def test_softcap_is_safe_at_the_ends_of_float32():
    for x in (3.0e38, -3.0e38, 1e30, -1e30, 0.0, 1e-45, -1e-45):
        for cap in (1e-3, 1.0, 50.0):
            s, f = evaluate(x, cap)
            assert math.isfinite(s) and math.isfinite(f)
            if abs(x) >= 1e30:
                assert s == math.copysign(float(np.float32(cap)), x) and f == 0.0
    assert evaluate(0.0, 30.0) == (0.0, 1.0)
    # the smallest softcap the library takes is the smallest normal float: its reciprocal is finite, so x = 0 stays 0 (no 0 * inf)
    tiny = float(np.float32(2.0 ** -126))
    for x in (0.0, 1e-45, 1.0, -3.0e38):
        s, f = evaluate(x, tiny)
        assert math.isfinite(s) and math.isfinite(f) and abs(s) <= tiny


def test_softcap_off_is_the_identity():
    for x in (-7.25, 0.0, 3.0e38, 1e-30):
        s, f = evaluate(x, 0.0)
        assert s == float(np.float32(x)) and f == 1.0


def test_alibi_term_on_both_sides_of_the_key():
    slope = float(np.float32(2.0 ** -3))
    for pos, j in ((10, 3), (3, 10), (5, 5), (0, 4000), (4000, 0), (2 ** 24 + 8, 0)):
        s, f = evaluate(1.5, 0.0, slope, pos, j)
        assert s == 1.5 - slope * abs(pos - j) and f == 1.0, (pos, j, s)
    # with a cap: the bias is added to the capped score, the factor is the cap's alone
    s0, f0 = evaluate(12.0, 30.0)
    s1, f1 = evaluate(12.0, 30.0, slope, 7, 19)
    assert s1 == float(np.float32(s0) - np.float32(slope * 12)) and f1 == f0
    # a slope of 0 changes nothing
    assert evaluate(12.0, 30.0, 0.0, 7, 19) == (s0, f0)


def test_eval_validation():
    lib = _fa2_lib.load()
    s, f = ctypes.c_float(), ctypes.c_float()
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), 1e-39, 1e-45, float(np.float32(2.0 ** -126)) * 0.99):      # (positive subnormals: 1 / softcap would be inf)
        assert lib.fa2_scoremod_eval(1.0, bad, 0.0, 0, 0, ctypes.byref(s), ctypes.byref(f)) == ERR_SOFTCAP
    assert lib.fa2_scoremod_eval(1.0, 1.0, 0.0, 0, 0, None, ctypes.byref(f)) == -1
    assert "softcap" in _fa2_lib.error_string(ERR_SOFTCAP)


def test_entry_point_validation_without_a_gpu():
    """FA2_ERR_SOFTCAP comes first through all four entry points, then the slope stride and the slope pointer's alignment; with good values the existing
    checks answer as they do for the windowed / packed calls."""
    lib = _fa2_lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    s3, l2, s2 = _fa2_lib.strides3(2 * 16 * 64, 16 * 64, 64), _fa2_lib.strides2(32, 16), _fa2_lib.strides2(64, 128)

    def fwd(q=p, D=64, cap=30.0, sl=p, st=0, flags=0, left=-1, smod=True):
        args = (0, q, p, p, p, p, 1, 2, 2, 16, 16, D, s3, s3, s3, s3, l2, 0.125, flags, left, -1, 0, None)
        return lib.fa2_fwd_scoremod(*args, cap, sl, st) if smod else lib.fa2_fwd_window(*args)

    def bwd(q=p, D=64, cap=30.0, sl=p, st=0, flags=0, left=-1, smod=True):
        args = (0, q, p, p, p, p, p, p, p, p, p, 1, 2, 16, 16, D, s3, s3, s3, s3, s3, s3, s3, s3, l2, 0.125, flags, left, -1, 0, None)
        return lib.fa2_bwd_scoremod(*args, cap, sl, st) if smod else lib.fa2_bwd_window(*args)

    def vfwd(q=p, D=64, cap=30.0, sl=p, st=0, flags=0, left=-1, cu=p, smod=True):
        args = (0, q, p, p, p, p, 2, 2, 2, 16, 16, D, cu, cu, s2, s2, s2, s2, 32, 0.125, flags, left, -1, None)
        return lib.fa2_fwd_varlen_scoremod(*args, cap, sl, st) if smod else lib.fa2_fwd_varlen(*args)

    def vbwd(q=p, D=64, cap=30.0, sl=p, st=0, flags=0, left=-1, cu=p, smod=True):
        args = (0, q, p, p, p, p, p, p, p, p, p, 2, 2, 16, 16, D, cu, cu, s2, s2, s2, s2, s2, s2, s2, s2, 32, 0.125, flags, left, -1, None)
        return lib.fa2_bwd_varlen_scoremod(*args, cap, sl, st) if smod else lib.fa2_bwd_varlen(*args)

    for f in (fwd, bwd, vfwd, vbwd):
        for bad in (-1.0, -1e-6, float("nan"), float("inf"), float("-inf"), 1e-39):
            assert f(cap=bad) == ERR_SOFTCAP, (f.__name__, bad)
            assert f(cap=bad, q=None) == ERR_SOFTCAP and f(cap=bad, D=44) == ERR_SOFTCAP        # reported before anything else is looked at
            assert f(cap=bad, sl=p + 2) == ERR_SOFTCAP and f(cap=bad, st=-1) == ERR_SOFTCAP
        assert f(st=-1) == -2 and f(st=-1, q=None) == -2 and f(st=-1, sl=p + 2) == -2            # FA2_ERR_BAD_SHAPE: a negative stride
        for off in (1, 2, 3):
            assert f(sl=p + off) == -4 and f(sl=p + off, q=None) == -4                          # FA2_ERR_ALIGNMENT: f32 slopes on a 4-byte boundary
        assert f(sl=p + 4, q=None) == -1                                                         # (4-byte aligned is enough)
        # with good values: the windowed / packed call's answers, for the cap alone, the slopes alone, both, and neither
        for kw in (dict(), dict(sl=None), dict(cap=0.0), dict(cap=0.0, sl=None), dict(st=2)):
            for defect in (dict(q=None), dict(D=44), dict(D=520), dict(left=-2), dict(flags=8)):
                assert f(**kw, **defect) == f(smod=False, **defect), (f.__name__, kw, defect)
        assert f(q=None) == -1 and f(D=44) == -3 and f(left=-2) == -2 and f(flags=8) == -2
    assert vfwd(cu=None) == -1 and vbwd(cu=None) == -1
    assert fwd(flags=4) == -2 and bwd(flags=4) == -2                                             # FA2_FLAG_BOTTOM_RIGHT belongs to the packed entry points


def test_operator_argument_errors_come_before_any_device_work():
    q = torch.zeros(2, 4, 16, 64, dtype=torch.float16)
    qp = torch.zeros(32, 4, 64, dtype=torch.float16)
    cu = torch.tensor([0, 16, 32], dtype=torch.int32)
    ok = torch.ones(4)
    for bad in (-1.0, float("nan"), float("inf"), "x", None, True, 1e-39):
        with pytest.raises(ValueError, match="softcap"):
            flash_attention(q, q, q, softcap=bad)
        with pytest.raises(ValueError, match="softcap"):
            flash_attention_varlen(qp, qp, qp, cu, cu, 16, 16, softcap=bad)
    wrong = [torch.ones(3), torch.ones(2, 3), torch.ones(3, 4), torch.ones(1, 2, 4), torch.ones(4, dtype=torch.float64), torch.ones(4, dtype=torch.float16),
             torch.ones(4, device="meta"), [0.5, 0.5, 0.5, 0.5], 0.5]
    for bad in wrong:
        with pytest.raises(ValueError, match="alibi_slopes"):
            flash_attention(q, q, q, alibi_slopes=bad)
        with pytest.raises(ValueError, match="alibi_slopes"):
            flash_attention(q.transpose(1, 2), q.transpose(1, 2), q.transpose(1, 2), BNHD_fmt=True, alibi_slopes=bad)
        with pytest.raises(ValueError, match="alibi_slopes"):
            flash_attention_varlen(qp, qp, qp, cu, cu, 16, 16, alibi_slopes=bad)
    for kw in (dict(softcap=30.0), dict(alibi_slopes=ok), dict(softcap=30.0, alibi_slopes=torch.ones(2, 4))):
        with pytest.raises(ValueError, match="mask"):
            flash_attention(q, q, q, mask=torch.ones(16, 16, dtype=torch.bool), **kw)
        with pytest.raises(ValueError, match="dropout"):
            flash_attention(q, q, q, dropout_p=0.1, dropout_seed=1, **kw)
        with pytest.raises(ValueError, match="dropout"):
            flash_attention_varlen(qp, qp, qp, cu, cu, 16, 16, dropout_p=0.1, dropout_seed=1, **kw)
        # good arguments on CPU tensors: refused as by the other paths of the operator
        with pytest.raises(RuntimeError, match="ROCm device"):
            flash_attention(q, q, q, **kw)
        with pytest.raises(RuntimeError, match="ROCm device"):
            flash_attention_varlen(qp, qp, qp, cu, cu, 16, 16, **kw)
    # a non-contiguous slope tensor is a good argument (made contiguous once, by the parser: that tensor is the one the launches read)
    from rocwmma_fattn.FlashAttn import _parse_scoremod, _scoremod_args
    strided = torch.arange(8, dtype=torch.float32)[::2]
    cap, sl = _parse_scoremod(30.0, strided, q, 4, 2)
    assert sl.is_contiguous() and torch.equal(sl, strided) and _scoremod_args((cap, sl)) == (30.0, sl.data_ptr(), 0)
    expanded = torch.ones(4).expand(2, 4)
    cap, sl = _parse_scoremod(0.0, expanded, q, 4, 2)
    assert sl.is_contiguous() and _scoremod_args((cap, sl)) == (0.0, sl.data_ptr(), 4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        flash_attention(q, q, q, alibi_slopes=expanded)
    # dropout_p == 0 together with the keywords is no conflict
    with pytest.raises(RuntimeError, match="ROCm device"):
        flash_attention(q, q, q, softcap=30.0, dropout_p=0.0)
