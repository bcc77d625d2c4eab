// fa2_scoremod.h — the score modifiers (logit soft-capping and ALiBi slopes) of the FA2_SMOD kernels (scoremod_hip.cpp, varlen_scoremod_hip.cpp), shared by
// the three passes and the host (fa2_scoremod_eval, include/fa2_gfx950.h), so that the arithmetic exists once and can be tested on the CPU.
//
// Contract.  For query row i at key position pos (= i + q_offset; packed calls: i + the sequence's offset) and key j:
//     x  = (q_i . k_j) * scale                          f32: the MFMA product scaled in f32
//     s  = softcap > 0 ? softcap * tanh(x / softcap) : x
//     s -= slope[b, h] * |pos - j|                       h = the QUERY head, b = the batch (packed calls: the sequence); slope 0 = no ALiBi
// and the band's masks come LAST (tanh(-inf) = -1: capping a masked score would un-mask it).  The softmax, the LSE and P are those of s.
// Backward: dX = dS * (1 - tanh^2(x / softcap)) — smod_score returns that factor beside s; the ALiBi term is a constant of the call.
//
// tanh.  |y| >= 1/8: t = 1 - 2 / (1 + 2^(2 log2(e) y)): the exponential overflows to +inf or underflows to 0 for |y| beyond ~44, where the quotient is
// exactly 0 or 2 and t exactly +1 or -1 — finite for every finite y (the textbook (e - 1) / (e + 1) gives inf / inf there), and 1 - t^2 is exactly 0 in
// saturation.  That form cancels near 0: its error in t is a few 2^-24 ABSOLUTE, i.e. a few ulps of `softcap` in s whatever x is — at softcap = 1e4 that
// was 1e-3 in every score and in the LSE (found by tools/fuzz_lse.py).  So |y| < 1/8 takes the odd series y (1 - y^2/3 + 2 y^4/15 - 17 y^6/315), whose
// truncation (62 y^9 / 2835) is below 1.4e-9 relative there: the error of t is a few ulps of t itself, and s -> x as softcap grows.
// The division x / softcap is a multiplication by 1 / softcap, rounded on the host once per call.
// The distance |pos - j| enters as a float: exact below 2^24, rounded to nearest above.
// Slopes of either sign are served: nothing in the passes relies on s <= x (the dK / dV passes mask the rows >= Nq of a ragged last Q tile themselves).
#pragma once
#include <stdint.h>
#if !defined(__HIP_DEVICE_COMPILE__)
#include <math.h>
#endif

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FA2_SMOD_HD __host__ __device__
#else
#define FA2_SMOD_HD
#endif

namespace fa2 {

constexpr float kSmodLog2e = 1.4426950408889634f;

// What a score-modifier call adds to the parameter block of its kernels: one further kernel argument (FwdParams / BwdParams keep their layout).
struct ScoreMod {
    float softcap = 0.f;             // 0: no capping
    float inv_softcap = 0.f;         // 1 / softcap (0 when off: tanh(0) = 0 stays finite and is not used)
    float scale = 0.f;               // forward: |scale| (a negative scale is folded into Q's sign as elsewhere); the backward passes read BwdParams::scale
    const float* slopes = nullptr;   // f32 [.., H] in device memory; nullptr: no ALiBi
    int64_t stride = 0;              // elements between the slope vectors of two batches / sequences (0: one vector for all)
};
FA2_SMOD_HD inline ScoreMod make_scoremod(float softcap, float scale, const float* slopes, int64_t stride) {
    ScoreMod m;
    m.softcap = softcap;
    m.inv_softcap = softcap > 0.f ? 1.0f / softcap : 0.f;
    m.scale = scale < 0.f ? -scale : scale;
    m.slopes = slopes;
    m.stride = stride;
    return m;
}
// 0 (off) or a finite NORMAL positive number: NaN and inf are refused, and so is a positive value below the smallest normal float,
// because its reciprocal is +inf (0 * inf = NaN at x = 0) — 1 / 1.17549435e-38 is still finite
// (decided on the bits: the library is compiled with -fno-honor-nans, under which a floating-point comparison may not be relied on to refuse a NaN)
FA2_SMOD_HD inline bool softcap_ok(float softcap) {
    uint32_t bits;
    __builtin_memcpy(&bits, &softcap, 4);
    volatile uint32_t opaque = bits;          // (... nor the bit tests below, which the optimiser would turn back into such a comparison)
    const uint32_t u = opaque, ex = (u >> 23) & 0xffu;
    return (u << 1) == 0u || ((u >> 31) == 0u && ex >= 1u && ex <= 254u);
}

FA2_SMOD_HD inline float smod_exp2(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_exp2f(x);
#else
    return exp2f(x);
#endif
}
FA2_SMOD_HD inline float smod_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}
// tanh(y), exactly +-1 in saturation, finite for every finite y, a few ulps of the result near 0 (both forms computed, one selected: no branch)
FA2_SMOD_HD inline float smod_tanh(float y) {
    const float e = smod_exp2(y * 2.8853900817779268f);               // 2^(2 log2(e) y) = e^(2 y): +inf / 0 far out
    const float far = __builtin_fmaf(-2.0f, smod_rcp(1.0f + e), 1.0f);
    const float y2 = y * y;
    const float near = y * __builtin_fmaf(y2, __builtin_fmaf(y2, __builtin_fmaf(y2, -0.053968254f, 0.13333334f), -0.33333334f), 1.0f);
    return __builtin_fabsf(y) < 0.125f ? near : far;
}
// softcap * tanh(x / softcap) (the caller knows softcap > 0)
FA2_SMOD_HD inline float smod_cap(float x, float softcap, float inv_softcap, float* t) {
    *t = smod_tanh(x * inv_softcap);
    return softcap * *t;
}
// s - slope * dist
FA2_SMOD_HD inline float smod_alibi(float s, float slope, float dist) { return __builtin_fmaf(-slope, dist, s); }
// The whole transform without a branch (the backward passes: both modifiers always computed, a switched-off one selected away or multiplied by 0):
// x -> s, *dfac = ds / dx = 1 - tanh^2 (1 when softcap is off)
FA2_SMOD_HD inline float smod_score(float x, float softcap, float inv_softcap, float slope, float dist, float* dfac) {
    float t;
    const float capped = smod_cap(x, softcap, inv_softcap, &t);
    const bool on = softcap > 0.f;
    *dfac = on ? __builtin_fmaf(-t, t, 1.0f) : 1.0f;
    return smod_alibi(on ? capped : x, slope, dist);
}

}  // namespace fa2
