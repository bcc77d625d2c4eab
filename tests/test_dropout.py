"""CPU tests of attention dropout's mask contract (csrc/fa2_dropout.h, include/fa2_gfx950.h): the generator against the Random123 known answers, the
documented counter mapping restated in Python against the library's host function bit for bit, the statistics of the mask, and argument validation.
Nothing here touches a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from rocwmma_fattn import _fa2_lib
from rocwmma_fattn.FlashAttn import dropout_keep_mask, flash_attention, flash_attention_varlen

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox_py(ctr, key):
    """Philox4x32-10, written from the paper (Salmon et al., SC'11), independent of the library's code."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [c0, c1, c2, c3]


def philox_lib(ctr, key):
    out = (ctypes.c_uint32 * 4)()
    assert _fa2_lib.load().fa2_philox4x32_10((ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), out) == 0
    return list(out)


def threshold(p):
    pe = ctypes.c_float()
    t = _fa2_lib.load().fa2_dropout_threshold(p, ctypes.byref(pe))
    assert t >= 0
    return t, pe.value


def keep_py(seed, t, H, b, h, i, j):
    """The mapping as the header words it: ctr = {call(j), i, b * H + h, 0}, key = {seed lo, seed hi}, slice(j) picks the 16 bits."""
    call = (j >> 5) * 4 + ((j >> 2) & 1) * 2 + ((j >> 4) & 1)
    sl = ((j >> 3) & 1) * 4 + (j & 3)
    out = philox_py([call, i, b * H + h, 0], [seed & MASK32, seed >> 32])
    return ((out[sl >> 1] >> (16 * (sl & 1))) & 0xFFFF) >= t


def keep_lib(seed, p, H, b, h, i0, i1, j0, j1):
    m = np.empty((i1 - i0, j1 - j0), dtype=np.uint8)
    rc = _fa2_lib.load().fa2_dropout_keep_mask(seed, p, H, b, h, i0, i1, j0, j1, m.ctypes.data)
    assert rc == 0, rc
    return m.astype(bool)


KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([MASK32] * 4, [MASK32] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert philox_py(ctr, key) == want            # the independent implementation reproduces the Random123 vectors ...
    assert philox_lib(ctr, key) == want           # ... and so does the library


def test_philox_matches_python_on_random_inputs():
    g = np.random.default_rng(5)
    for _ in range(200):
        ctr = [int(x) for x in g.integers(0, 2 ** 32, 4)]
        key = [int(x) for x in g.integers(0, 2 ** 32, 2)]
        assert philox_lib(ctr, key) == philox_py(ctr, key)


@pytest.mark.parametrize("seed", [0, 1, 0x12345678, 2 ** 32, 0x9E3779B97F4A7C15, 2 ** 63 - 1, 2 ** 64 - 1])
def test_documented_mapping_equals_the_host_mask(seed):
    H, p = 5, 0.3
    t, _ = threshold(p)
    for (b, h, i0, i1, j0, j1) in ((0, 0, 0, 9, 0, 70), (3, 4, 65530, 65541, 65500, 65600), (1, 2, 2 ** 20 + 3, 2 ** 20 + 6, 2 ** 24 - 40, 2 ** 24 + 30)):
        got = keep_lib(seed, p, H, b, h, i0, i1, j0, j1)
        want = np.array([[keep_py(seed, t, H, b, h, i, j) for j in range(j0, j1)] for i in range(i0, i1)])
        assert np.array_equal(got, want), (seed, b, h, i0, j0)


def test_sub_rectangles_are_slices_and_the_mask_depends_on_b_h_seed():
    seed, p, H = 2 ** 40 + 17, 0.5, 3
    full = keep_lib(seed, p, H, 1, 2, 0, 150, 0, 210)
    for (i0, i1, j0, j1) in ((0, 150, 0, 210), (7, 8, 0, 210), (33, 97, 5, 6), (64, 150, 31, 129), (149, 150, 209, 210)):
        assert np.array_equal(keep_lib(seed, p, H, 1, 2, i0, i1, j0, j1), full[i0:i1, j0:j1])
    assert not np.array_equal(full, keep_lib(seed, p, H, 0, 2, 0, 150, 0, 210))
    assert not np.array_equal(full, keep_lib(seed, p, H, 1, 1, 0, 150, 0, 210))
    assert not np.array_equal(full, keep_lib(seed + 1, p, H, 1, 2, 0, 150, 0, 210))
    assert not np.array_equal(full, keep_lib(seed + 2 ** 32, p, H, 1, 2, 0, 150, 0, 210))        # the high key word counts
    # (b, h) enters as b * H + h only
    assert np.array_equal(keep_lib(seed, p, 3, 1, 2, 0, 40, 0, 40), keep_lib(seed, p, 5, 1, 0, 0, 40, 0, 40))
    # the wrapper: [B, H, Nq, Nkv] bool on the CPU
    m = dropout_keep_mask(seed, p, 2, H, 150, 210)
    assert m.dtype == torch.bool and m.shape == (2, H, 150, 210) and not m.is_cuda
    assert np.array_equal(m[1, 2].numpy(), full)
    assert dropout_keep_mask(seed, 0.0, 1, 1, 8, 8).all()


@pytest.mark.parametrize("p", [0.001, 0.1, 0.5, 0.9])
def test_threshold_and_statistics(p):
    t, p_eff = threshold(p)
    assert t == int(round(p * 65536)) and p_eff == t / 65536.0 and abs(p_eff - p) <= 2.0 ** -17
    rows, keys = 640, 1024                       # 655360 >= 2^19 elements
    n = rows * keys
    a = keep_lib(0xC0FFEE1234567, p, 4, 1, 3, 0, rows, 0, keys).astype(np.float64)
    b = keep_lib(0xC0FFEE1234568, p, 4, 1, 3, 0, rows, 0, keys).astype(np.float64)
    q = 1.0 - p_eff
    sigma = math.sqrt(q * (1 - q) / n)
    print("p %.4g: keep rate %.6f (want %.6f, sigma %.2g)" % (p, a.mean(), q, sigma))
    assert abs(a.mean() - q) <= 5 * sigma
    za = (a - a.mean()) / a.std()
    for name, c in (("keys", (za[:, 1:] * za[:, :-1]).mean()), ("rows", (za[1:, :] * za[:-1, :]).mean())):
        print("  lag-1 correlation along %s %.3g (bar %.3g)" % (name, c, 5 / math.sqrt(n)))
        assert abs(c) <= 5 / math.sqrt(n), (name, c)
    agree, want = (a == b).mean(), q * q + (1 - q) * (1 - q)
    print("  agreement between two seeds %.6f (want %.6f)" % (agree, want))
    assert abs(agree - want) <= 5 * math.sqrt(want * (1 - want) / n)


def test_threshold_edges():
    assert threshold(0.0) == (0, 0.0)
    t, pe = threshold(0.001)
    assert t == 66 and pe > 0                    # a 16-bit threshold: p = 0.001 does not become 0
    t, pe = threshold(float(np.nextafter(np.float32(1.0), np.float32(0.0))))
    assert t == 65535 and pe < 1.0               # (p that rounds to 65536 is clamped: 1 / (1 - p_eff) stays finite)
    lib = _fa2_lib.load()
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert lib.fa2_dropout_threshold(bad, None) == -9
        assert lib.fa2_dropout_keep_mask(1, bad, 1, 0, 0, 0, 1, 0, 1, ctypes.create_string_buffer(1)) == -9
    assert lib.fa2_dropout_keep_mask(1, 0.5, 1, 0, 0, 0, 1, 0, 1, None) == -1
    assert lib.fa2_dropout_keep_mask(1, 0.5, 2, 0, 2, 0, 1, 0, 1, ctypes.create_string_buffer(1)) == -2
    assert lib.fa2_dropout_keep_mask(1, 0.5, 2, 0, 0, 4, 4, 0, 1, ctypes.create_string_buffer(1)) == -2
    assert lib.fa2_philox4x32_10(None, None, None) == -1
    assert "dropout_p" in _fa2_lib.error_string(-9)


def test_entry_point_validation_without_a_gpu():
    """FA2_ERR_DROPOUT comes first through all four entry points; with a good p the existing checks answer as they do for the windowed / packed calls."""
    lib = _fa2_lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    s3, l2, s2 = _fa2_lib.strides3(2 * 16 * 64, 16 * 64, 64), _fa2_lib.strides2(32, 16), _fa2_lib.strides2(64, 128)

    def fwd(q=p, D=64, pd=0.1, flags=0, left=-1):
        return lib.fa2_fwd_dropout(0, q, p, p, p, p, 1, 2, 2, 16, 16, D, s3, s3, s3, s3, l2, 0.125, flags, left, -1, 0, None, pd, 7)

    def bwd(q=p, D=64, pd=0.1, flags=0, left=-1):
        return lib.fa2_bwd_dropout(0, q, p, p, p, p, p, p, p, p, p, 1, 2, 16, 16, D, s3, s3, s3, s3, s3, s3, s3, s3, l2, 0.125, flags, left, -1, 0, None, pd, 7)

    def vfwd(q=p, D=64, pd=0.1, flags=0, left=-1, cu=p):
        return lib.fa2_fwd_varlen_dropout(0, q, p, p, p, p, 2, 2, 2, 16, 16, D, cu, cu, s2, s2, s2, s2, 32, 0.125, flags, left, -1, None, pd, 7)

    def vbwd(q=p, D=64, pd=0.1, flags=0, left=-1, cu=p):
        return lib.fa2_bwd_varlen_dropout(0, q, p, p, p, p, p, p, p, p, p, 2, 2, 16, 16, D, cu, cu, s2, s2, s2, s2, s2, s2, s2, s2, 32, 0.125, flags, left, -1,
                                          None, pd, 7)

    for f in (fwd, bwd, vfwd, vbwd):
        for bad in (-1e-6, 1.0, 2.0, float("nan")):
            assert f(pd=bad) == -9, (f.__name__, bad)
            assert f(pd=bad, q=None) == -9 and f(pd=bad, D=44) == -9          # reported before anything else is looked at
        assert f(q=None) == -1, f.__name__                                    # FA2_ERR_NULL_POINTER, as today
        assert f(D=44) == -3 and f(D=520) == -3                               # FA2_ERR_HEAD_DIM
        assert f(left=-2) == -2 and f(flags=8) == -2                          # FA2_ERR_BAD_SHAPE
        assert f(q=None, pd=0.0) == -1                                        # p == 0 is legal: the next check answers
    assert vfwd(cu=None) == -1 and vbwd(cu=None) == -1
    assert fwd(flags=4) == -2 and bwd(flags=4) == -2                          # FA2_FLAG_BOTTOM_RIGHT belongs to the packed entry points


def test_operator_argument_errors_come_before_any_device_work():
    q = torch.zeros(1, 2, 16, 64, dtype=torch.float16)
    cu = torch.tensor([0, 16], dtype=torch.int32)
    for bad in (-0.1, 1.0, float("nan"), "x", None, True):
        with pytest.raises(ValueError, match="dropout_p"):
            flash_attention(q, q, q, dropout_p=bad)
        with pytest.raises(ValueError, match="dropout_p"):
            flash_attention_varlen(q[0].transpose(0, 1), q[0].transpose(0, 1), q[0].transpose(0, 1), cu, cu, 16, 16, dropout_p=bad)
    with pytest.raises(ValueError, match="dropout_seed"):
        flash_attention(q, q, q, dropout_p=0.1, dropout_seed=-1)
    with pytest.raises(ValueError, match="dropout_seed"):
        flash_attention(q, q, q, dropout_p=0.1, dropout_seed=2 ** 64)
    with pytest.raises(ValueError, match="mask"):
        flash_attention(q, q, q, mask=torch.ones(16, 16, dtype=torch.bool), dropout_p=0.1)
    # CPU tensors are refused as by the other paths of the operator
    with pytest.raises(RuntimeError, match="ROCm device"):
        flash_attention(q, q, q, dropout_p=0.1, dropout_seed=3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        flash_attention_varlen(q[0].transpose(0, 1), q[0].transpose(0, 1), q[0].transpose(0, 1), cu, cu, 16, 16, dropout_p=0.1, dropout_seed=3)
    with pytest.raises(ValueError, match="dropout_p"):
        dropout_keep_mask(1, 1.0, 1, 1, 4, 4)


def test_default_seed_comes_from_the_cpu_generator():
    from rocwmma_fattn.FlashAttn import _parse_dropout
    torch.manual_seed(1234)
    a = _parse_dropout(0.25, None)
    b = _parse_dropout(0.25, None)
    torch.manual_seed(1234)
    assert _parse_dropout(0.25, None) == a and a != b and 0 <= a[1] < 2 ** 63 and a[0] == 0.25
    assert _parse_dropout(0.0, None) is None and _parse_dropout(0, 5) is None
