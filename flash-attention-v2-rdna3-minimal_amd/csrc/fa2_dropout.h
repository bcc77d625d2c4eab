// fa2_dropout.h — the keep mask of attention dropout, shared by the host (fa2_dropout_keep_mask, include/fa2_gfx950.h) and the three passes of the
// FA2_DROP kernels (dropout_hip.cpp, varlen_dropout_hip.cpp), so that it can be tested on the CPU and read back from the device bit for bit.
//
// Contract.  Whether the probability at (b, h, i, j) — batch (packed calls: sequence) b, QUERY head h, query row i, key j, the latter two counted inside
// the sequence — is kept is a pure function of (seed, b * H + h, i, j) and the threshold t.  Nothing else enters: not the tile size, the rows option, the
// head dim, the dtype, the memory layout, grouped or expanded k / v, or the pass that asks.
//
// Generator.  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants), key = the 64-bit seed:
//     key = { seed & 0xffffffff, seed >> 32 }
// Threshold.  t = round(p * 65536), clamped to [0, 65535]; an element is DROPPED when its 16 bits are < t, so p_eff = t / 65536 and the kept
// probabilities are scaled by 1 / (1 - p_eff) = 65536 / (65536 - t).  (p so close to 1 that it rounds to 65536 is clamped to 65535 / 65536.)
//
// Counter mapping.  One Philox call yields 128 bits = eight 16-bit slices = eight keys of one row:
//     ctr = { call(j), i, b * H + h, 0 }          call(j)  = (j >> 5) * 4 + ((j >> 2) & 1) * 2 + ((j >> 4) & 1)
//     bits16(j) = (out[slice >> 1] >> (16 * (slice & 1))) & 0xffff,      slice(j) = ((j >> 3) & 1) * 4 + (j & 3)
// i.e. inside a 32-key block, with j % 32 = 8 g + 4 u + e (g = 0..3, u = 0..1, e = 0..3), a call is (block, u, g >> 1) and covers the keys
// {8 g + 4 u + e : g in {2 (g >> 1), 2 (g >> 1) + 1}, e = 0..3}; slice = 4 (g & 1) + e.  This is the register order in which a lane of the S^T tile of
// mfma_f32_32x32x16 holds the keys of its row (u = lane / 32; registers 8 (g >> 1) ... 8 (g >> 1) + 7 of the 32-key accumulator): two calls per lane
// per 32 keys cover the lane's 16 scores, no bits are thrown away, and output word w of a call lines up with the packed pair of 16-bit probabilities
// (registers 2 w, 2 w + 1) the P.V product consumes — the forward masks packed dwords.  The dQ pass has the same lane layout.  In the dK / dV passes a
// lane owns one key and 32 rows of a tile; there a lane computes the four calls of ONE row over the wave's 32 keys and the 32 x 32 bit matrix of a
// half-wave is transposed with 32 ballots (drop_keylane_bits), so those passes also make four calls per lane and 32 scores.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FA2_DROP_HD __host__ __device__
#else
#define FA2_DROP_HD
#endif

namespace fa2 {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;      // multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;      // key increments (Weyl sequence)

// Philox4x32-10: out = philox(ctr, key)
FA2_DROP_HD inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// p in [0, 1) (the caller validates) -> t; *p_eff = t / 65536
FA2_DROP_HD inline uint32_t dropout_threshold(float p, float* p_eff) {
    int t = (int)(p * 65536.0f + 0.5f);
    t = t < 0 ? 0 : t > 65535 ? 65535 : t;
    if (p_eff) *p_eff = (float)t / 65536.0f;
    return (uint32_t)t;
}
// factor of the kept probabilities, 1 / (1 - p_eff)
FA2_DROP_HD inline float dropout_rescale(uint32_t t) { return 65536.0f / (float)(65536u - t); }

FA2_DROP_HD inline uint32_t dropout_call(uint32_t j) { return (j >> 5) * 4u + ((j >> 2) & 1u) * 2u + ((j >> 4) & 1u); }
FA2_DROP_HD inline uint32_t dropout_slice(uint32_t j) { return ((j >> 3) & 1u) * 4u + (j & 3u); }

// the element (bh = b * H + h, row i, key j): kept?
FA2_DROP_HD inline bool dropout_keep(uint64_t seed, uint32_t t, uint32_t bh, uint32_t i, uint32_t j) {
    uint32_t o[4];
    philox4x32_10(dropout_call(j), i, bh, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
    const uint32_t s = dropout_slice(j);
    return ((o[s >> 1] >> (16u * (s & 1u))) & 0xffffu) >= t;
}

// The seed and the threshold of a dropout call travel in fields of FwdParams / BwdParams that the windowed and packed kernels never read (the KV-split
// bookkeeping and the bias kind): the parameter blocks keep their layout, and every other kernel its kernarg segment.
template <typename P>
FA2_DROP_HD inline void set_dropout(P& p, uint64_t seed, uint32_t t) { p.full_items = (int)(uint32_t)seed; p.split_items = (int)(uint32_t)(seed >> 32); p.bias_kind = (int)t; }

#if defined(__HIPCC__)
struct DropCtx {
    uint32_t k0, k1, t, t_hi, bh;     // key words, threshold, threshold << 16, b * H + h
    float rs;                         // 1 / (1 - p_eff)
};
template <typename P>
__device__ __forceinline__ DropCtx drop_ctx(const P& p, int b, int h) {
    DropCtx d;
    d.k0 = (uint32_t)p.full_items; d.k1 = (uint32_t)p.split_items; d.t = (uint32_t)p.bias_kind; d.t_hi = d.t << 16;
    d.bh = (uint32_t)b * (uint32_t)p.H + (uint32_t)h;
    d.rs = dropout_rescale(d.t);
    return d;
}

// Lane = query row (the forward and the dQ pass): the Philox words of the lane's 32 scores of the 64-key tile at kv0 (a multiple of 64).
// Call c = 2 * half + gp: o[c][w] covers the accumulator registers 8 gp + 2 w (low 16 bits) and 8 gp + 2 w + 1 (high 16 bits) of 32-key half `half`.
__device__ __forceinline__ void drop_rowlane_call(const DropCtx& d, uint32_t row, uint32_t kv0, uint32_t hi, int c, uint32_t (&o)[4]) {
    philox4x32_10(((kv0 >> 5) + (uint32_t)(c >> 1)) * 4u + hi * 2u + (uint32_t)(c & 1), row, d.bh, 0u, d.k0, d.k1, o);
}
__device__ __forceinline__ void drop_rowlane_words(const DropCtx& d, uint32_t row, uint32_t kv0, uint32_t hi, uint32_t (&o)[4][4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) drop_rowlane_call(d, row, kv0, hi, c, o[c]);
}
// AND-mask of a packed pair of 16-bit probabilities from its Philox word
__device__ __forceinline__ uint32_t drop_pair_mask(const DropCtx& d, uint32_t w) {
    return ((w & 0xffffu) >= d.t ? 0xffffu : 0u) | (w >= d.t_hi ? 0xffff0000u : 0u);
}
__device__ __forceinline__ bool drop_keep_lo(const DropCtx& d, uint32_t w) { return (w & 0xffffu) >= d.t; }
__device__ __forceinline__ bool drop_keep_hi(const DropCtx& d, uint32_t w) { return w >= d.t_hi; }

// Lane = key (the dK / dV passes): the lane holds, of the 64-row Q tile at q0t, the rows q0t + (r & 3) + 8 (r >> 2) + 4 hi + 32 s (r = 0..15 registers of
// accumulator s = 0, 1) against its one key kvw0 + l31 (kvw0 a multiple of 32).  Returns the keep bits of those 32 scores, bit 16 s + r.
// Lane (x = l31, hi) computes row x of its half-wave against the wave's 32 keys (four calls), bit k of its word W = keep(row, kvw0 + k); ballot k then holds
// bit k of every lane, whose half `hi` is what the lane with l31 == k wants.  Every lane of the wave must be active.
__device__ __forceinline__ uint32_t drop_keylane_bits(const DropCtx& d, uint32_t q0t, uint32_t kvw0, uint32_t l31, uint32_t hi) {
    const uint32_t row = q0t + (l31 & 3u) + 8u * ((l31 & 15u) >> 2) + 4u * hi + 32u * (l31 >> 4);
    uint32_t W = 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {                      // call c = 2 u + gp of the 32-key block
        uint32_t o[4];
        philox4x32_10((kvw0 >> 5) * 4u + (uint32_t)c, row, d.bh, 0u, d.k0, d.k1, o);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int key = 8 * (2 * (c & 1) + (s >> 2)) + 4 * (c >> 1) + (s & 3);
            const bool keep = (s & 1) ? drop_keep_hi(d, o[s >> 1]) : drop_keep_lo(d, o[s >> 1]);
            W |= keep ? (1u << key) : 0u;
        }
    }
    uint32_t m_lo = 0u, m_hi = 0u;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const uint64_t m = __builtin_amdgcn_ballot_w64((W & (1u << k)) != 0u);
        if (l31 == (uint32_t)k) { m_lo = (uint32_t)m; m_hi = (uint32_t)(m >> 32); }
    }
    return hi ? m_hi : m_lo;
}
#endif

}  // namespace fa2
