// fa2_rotary.h — the rotary-embedding arithmetic of the KV-cache append (fa2_kvcache_append; csrc/fa2_kvappend.hip.h), shared by the kernel and the host
// (fa2_rotary_eval, include/fa2_gfx950.h), so that the arithmetic exists once and can be tested on the CPU.
//
// Contract.  A row x of D columns, a table row (cos[j], sin[j]), j < rotary_dim / 2.  Pair j is the columns (2j, 2j + 1) when interleaved (GPT-J), else
// (j, j + rotary_dim / 2) (GPT-NeoX).  In f32:
//     y1 = x1 * c - x2 * s        = fma(x1, c, -(x2 * s))
//     y2 = x1 * s + x2 * c        = fma(x1, s,   x2 * c)
// each rounded ONCE to the destination format (RNE to the I/O dtype; an e4m3 destination divides the f32 value by the descale first).  The two products
// x2 * s and x2 * c are rounded to f32 and the fma adds the other product unrounded — written as an explicit fma so that the host and the device, whose
// compilers contract differently, form the same bits.  Columns at or beyond rotary_dim are not touched by this file: the callers copy them bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FA2_ROT_HD __host__ __device__
#else
#define FA2_ROT_HD
#endif

namespace fa2 {

FA2_ROT_HD inline void rotary_pair(float x1, float x2, float c, float s, float* y1, float* y2) {
    *y1 = __builtin_fmaf(x1, c, -(x2 * s));
    *y2 = __builtin_fmaf(x1, s, x2 * c);
}

// The column of pair j's two members, and the table row of a position: the row index is clamped into [0, seqlen_ro - 1] before it becomes an address
// (a table that is too short gives a wrong answer, not a fault).
FA2_ROT_HD inline int rotary_col1(int j, int rotary_dim, bool interleaved) { (void)rotary_dim; return interleaved ? 2 * j : j; }
FA2_ROT_HD inline int rotary_col2(int j, int rotary_dim, bool interleaved) { return interleaved ? 2 * j + 1 : j + rotary_dim / 2; }
FA2_ROT_HD inline int64_t rotary_table_row(int64_t pos, int64_t seqlen_ro) { return pos < 0 ? 0 : pos >= seqlen_ro ? seqlen_ro - 1 : pos; }

// 16-bit <-> f32 on bit patterns (the host has no _Float16 arithmetic to lean on; the kernel uses the hardware conversions, which round the same way: RNE,
// subnormals kept).
FA2_ROT_HD inline float rot_bits_f32(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
FA2_ROT_HD inline uint32_t rot_f32_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

FA2_ROT_HD inline float rot_f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, ex = (h >> 10) & 31u, man = h & 0x3ffu;
    if (ex == 0) {                                           // zero / subnormal: man * 2^-24, exact in f32
        const float v = (float)man * 5.9604644775390625e-8f;
        return rot_bits_f32(sign | rot_f32_bits(v));
    }
    if (ex == 31) return rot_bits_f32(sign | 0x7f800000u | (man << 13));
    return rot_bits_f32(sign | ((ex + 112u) << 23) | (man << 13));
}
FA2_ROT_HD inline float rot_bf16_to_f32(uint16_t h) { return rot_bits_f32((uint32_t)h << 16); }

FA2_ROT_HD inline uint16_t rot_f32_to_f16(float f) {
    uint32_t x = rot_f32_bits(f);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    x &= 0x7fffffffu;
    if (x > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (x >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);                     // |f| >= 65536 (and +-inf)
    if (x < 0x38800000u) {                                                       // |f| < 2^-14: a subnormal f16, a multiple of 2^-24
        if (x < 0x33000000u) return sign;                                        // |f| < 2^-25 rounds to zero (2^-25 itself ties to even: zero, below)
        // integer rounding of |f| * 2^24 (RNE): the value has at most 24 significant bits below 2^10
        const uint32_t ex = x >> 23, man = (x & 0x7fffffu) | 0x800000u;          // |f| = man * 2^(ex - 150)
        const uint32_t shift = 126u - ex;                                        // |f| * 2^24 = man >> shift, shift in 14 .. 24
        const uint32_t q = man >> shift, rem = man & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        return (uint16_t)(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
    }
    x += 0xfffu + ((x >> 13) & 1u);                                              // RNE at bit 13; a carry moves into the exponent
    const uint32_t h = (x - 0x38000000u) >> 13;
    return (uint16_t)(sign | (h >= 0x7c00u ? 0x7c00u : h));
}
FA2_ROT_HD inline uint16_t rot_f32_to_bf16(float f) {
    uint32_t x = rot_f32_bits(f);
    if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((x >> 16) | 0x40u);
    x += 0x7fffu + ((x >> 16) & 1u);
    return (uint16_t)(x >> 16);
}
FA2_ROT_HD inline float rot_io_to_f32(uint16_t h, bool bf16) { return bf16 ? rot_bf16_to_f32(h) : rot_f16_to_f32(h); }
FA2_ROT_HD inline uint16_t rot_f32_to_io(float f, bool bf16) { return bf16 ? rot_f32_to_bf16(f) : rot_f32_to_f16(f); }

}  // namespace fa2
