// fa2_kvappend_mla_fp8.hip.h — the QUANTISING append for an e4m3 latent (MLA) KV cache of 656-byte rows (fa2_kvcache_append_mla_fp8,
// fa2_kvcache_append_mla_varlen_fp8; include/fa2_gfx950.h has the contract, DESIGN.md section 33 the reasons): the write side of fa2_fwd_decode_mla_fp8.
// One launch turns the new tokens' kv_c rows (512 columns) and k_pe rows (64 columns) into cache rows of 512 e4m3 codes, four f32 scales and 64 rotary
// columns in the I/O dtype at the key position only the device knows, and — when q is given — writes q with its trailing 64 columns rotated to q_out.
//
// The grid is fa2_kvappend_mla.hip.h's: blockIdx.x is the (sequence, token) group (the packed call: the packed token), so everything that decides
// "skip" is uniform over the workgroup; blockIdx.y * blockDim.x + threadIdx.x = T is the lane's index among the group's R * 36 units, R = 1 + H.
//   T >= 36   the q rows: the 16-bit kernel's units, lanes and code (kvappend_mla_row is CALLED, not copied), so q_out has its bits.
//   T <  64   the first wave of slice 0 — whole, whatever the workgroup size (64, 128 or 256 lanes) — quantises the latent row.  Lane l loads chunk l of
//             kv_c (16 bytes; the wave one kilobyte, coalesced), unpacks its 8 values and takes their max |x|.  The 16 lanes of a scale group of 128
//             columns are one DPP row: four steps (quad_perm xor 1, quad_perm xor 2, row_half_mirror, row_mirror) leave the group's amax in every
//             lane of the row — no LDS, no barrier.  Each lane forms scale = amax / 448 (an all-zero group: 1.0f), divides, clamps and converts its 8
//             values (append_quant8, fa2_kvappend.hip.h: the correctly rounded division, v_cvt_pk_fp8_f32) and stores 8 code bytes: 512 contiguous
//             bytes per wave.  Four v_readlane fetch the scales of lanes 0, 16, 32, 48 and lane 0 stores them as 16 bytes at byte 512.  Every
//             cross-lane operation sits outside the per-lane branches.
//   T 32..35  of that wave also move the rotary tail: unit u's two chunks of k_pe (mla_append_chunks: both members of a GPT-NeoX pair in one lane) go
//             through the 16-bit kernel's arithmetic (append_table, append_unpack8, rotary_pair, append_pack8) to bytes 528 .. 655; without tables bit
//             for bit.  (These lanes are below 36: they have no q unit.)
//
// mla_fp8_append_row is the row's address arithmetic, host and device: the kernels and the host walk of tools/kvappend_mla_fp8_sanitize.cpp call it.
// Safety is fa2_kvappend_mla.hip.h's: kvappend_slot gives the key position or "skip", a page id outside [0, num_pages) skips too
// (mla_append_cache_row, here with strides in BYTES), the table row is clamped, nothing is clamped onto a live row, all addressing is in 64 bits.
//
// A NaN in kv_c: v_max_f32 drops it, so the group's scale is that of its other elements and their codes are what they would be without it; the NaN
// itself divides to a NaN, falls through the clamp (this unit honours NaNs) and converts to a NaN code.  +-Inf makes the scale Inf: the group's finite
// elements become zeros and the Inf a NaN code.
#pragma once
#include <stdint.h>

#include "fa2_kvappend_mla.hip.h"    // KvAppendMlaParams, mla_append_chunks, mla_append_cache_row; the q rows' kvappend_mla_row

namespace fa2 {

// KvAppendMlaParams with kv_cache the BYTE cache and ks its strides in bytes; everything else keeps its meaning (the q rows are read through it as it is)
struct MlaFp8AppendRow {
    const uint16_t *c, *pe;         // the token's kv_c row (512 columns) and k_pe row (64 columns)
    char* dst;                      // the cache row: 656 bytes
    bool rotate;                    // the tail is rotated by table row offset tr
    int64_t tr;
};

// The latent row of one token.  (b, i, nnew), (sb, sr) and owned are mla_append_unit's.  -> false: no row is written (a token no sequence owns, a
// position outside the cache, a page id outside the pool); nothing of *w is valid then.
FA2_DEC_HD inline bool mla_fp8_append_row(const KvAppendMlaParams& p, int b, int i, int nnew, int64_t sb, int64_t sr, bool owned, MlaFp8AppendRow* w) {
    if (!owned) return false;
    const int64_t len = p.lens[b];
    const int64_t slot = kvappend_slot(len, p.capacity_keys, nnew, i);
    if (slot < 0) return false;
    const int64_t ofs = mla_append_cache_row(slot, b, p.bt, p.bts, p.page_size, p.num_pages, p.ks);
    if (ofs < 0) return false;
    w->dst = static_cast<char*>(p.kv_cache) + ofs;
    w->c = static_cast<const uint16_t*>(p.kv_c) + sb * p.cs[0] + sr * p.cs[1];
    w->pe = static_cast<const uint16_t*>(p.k_pe) + sb * p.ps[0] + sr * p.ps[1];
    w->rotate = p.cos != nullptr;
    w->tr = w->rotate ? rotary_table_row(len - nnew + i, p.seqlen_ro) * p.ros : 0;
    return true;
}

// Tail unit u (32 .. 35) of the row: the columns of k_pe its two chunks start at, the bytes of the cache row they land on, its first table entry
FA2_DEC_HD inline void mla_fp8_append_tail(int u, bool halves, int* col_a, int* col_b, int* byte_a, int* byte_b, int* j0) {
    int ca, cb;
    mla_append_chunks(u, halves, &ca, &cb);
    *col_a = 8 * (ca - kMlaTailChunk);
    *col_b = 8 * (cb - kMlaTailChunk);
    *byte_a = kMlaFp8RopeOff + 2 * *col_a;
    *byte_b = kMlaFp8RopeOff + 2 * *col_b;
    *j0 = 8 * (u - kMlaTailUnit);
}

#if defined(__HIPCC__)

// max over the 16 lanes of a DPP row, left in every lane of the row.  v >= 0 (or NaN-free by construction: v_max_f32 has dropped the NaNs)
__device__ __forceinline__ float mla_fp8_row_max(float v) {
    constexpr int kXor1 = 0xB1, kXor2 = 0x4E, kHalfMirror = 0x141, kMirror = 0x140;      // quad_perm:[1,0,3,2], quad_perm:[2,3,0,1], row_half_mirror, row_mirror
#define FA2_DPP_MAX(ctrl)                                                                                      \
    v = __builtin_fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, false)))
    FA2_DPP_MAX(kXor1);
    FA2_DPP_MAX(kXor2);
    FA2_DPP_MAX(kHalfMirror);
    FA2_DPP_MAX(kMirror);
#undef FA2_DPP_MAX
    return v;
}

// The latent row, by the first wave of slice 0 (all 64 lanes active: the caller's condition is uniform over the wave).  lane = threadIdx.x < 64.
template <bool BF16>
__device__ __forceinline__ void kvappend_mla_fp8_latent(const KvAppendMlaParams& p, const MlaFp8AppendRow& w, int lane) {
    float x[8];
    append_unpack8<BF16>(*reinterpret_cast<const u32x4*>(w.c + 8 * lane), x);
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) m = __builtin_fmaxf(m, __builtin_fabsf(x[k]));
    const float amax = mla_fp8_row_max(m);
    const float scale = amax > 0.0f ? amax / 448.0f : 1.0f;
    *reinterpret_cast<u32x2*>(w.dst + 8 * lane) = append_quant8(x, scale);
    const int sb = __builtin_bit_cast(int, scale);
    const u32x4 scales = {(uint32_t)__builtin_amdgcn_readlane(sb, 0), (uint32_t)__builtin_amdgcn_readlane(sb, 16), (uint32_t)__builtin_amdgcn_readlane(sb, 32),
                          (uint32_t)__builtin_amdgcn_readlane(sb, 48)};
    if (lane == 0) *reinterpret_cast<u32x4*>(w.dst + kMlaFp8ScaleOff) = scales;

    if (lane < kMlaTailUnit || lane >= kMlaUnits) return;       // the rotary tail: units 32 .. 35, nothing across lanes from here on
    int col_a, col_b, byte_a, byte_b, j0;
    mla_fp8_append_tail(lane, w.rotate && !p.interleaved, &col_a, &col_b, &byte_a, &byte_b, &j0);
    const u32x4 wa = *reinterpret_cast<const u32x4*>(w.pe + col_a);
    const u32x4 wb = *reinterpret_cast<const u32x4*>(w.pe + col_b);
    if (!w.rotate) {                                             // bit for bit
        *reinterpret_cast<u32x4*>(w.dst + byte_a) = wa;
        *reinterpret_cast<u32x4*>(w.dst + byte_b) = wb;
        return;
    }
    float xa[8], xb[8], c[8], s[8];
    append_table<BF16, 8>(p.cos, w.tr, j0, p.tab16 != 0, c);
    append_table<BF16, 8>(p.sin, w.tr, j0, p.tab16 != 0, s);
    append_unpack8<BF16>(wa, xa);
    append_unpack8<BF16>(wb, xb);
    if (!p.interleaved) {
#pragma unroll
        for (int e = 0; e < 8; ++e) rotary_pair(xa[e], xb[e], c[e], s[e], &xa[e], &xb[e]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            rotary_pair(xa[2 * k], xa[2 * k + 1], c[k], s[k], &xa[2 * k], &xa[2 * k + 1]);
            rotary_pair(xb[2 * k], xb[2 * k + 1], c[4 + k], s[4 + k], &xb[2 * k], &xb[2 * k + 1]);
        }
    }
    *reinterpret_cast<u32x4*>(w.dst + byte_a) = append_pack8<BF16>(xa);
    *reinterpret_cast<u32x4*>(w.dst + byte_b) = append_pack8<BF16>(xb);
}

// One token: what both kernels run
template <bool BF16>
__device__ __forceinline__ void kvappend_mla_fp8_token(const KvAppendMlaParams& p, int b, int i, int nnew, int64_t sb, int64_t sr, bool owned) {
    if (blockIdx.y == 0 && threadIdx.x < 64) {                   // one whole wave: blockDim.x is 64, 128 or 256
        MlaFp8AppendRow w;
        if (mla_fp8_append_row(p, b, i, nnew, sb, sr, owned, &w)) kvappend_mla_fp8_latent<BF16>(p, w, threadIdx.x);      // (uniform over the workgroup)
    }
    // the q rows: units 36 .. R * 36 - 1 of the 16-bit kernel, in its lanes, by its code.  Units 0 .. 35 are its latent row: never entered here, so
    // the byte cache and its byte strides are never read as a 16-bit cache's.
    if (blockIdx.y * blockDim.x + threadIdx.x >= kMlaUnits) kvappend_mla_row<BF16>(p, b, i, nnew, sb, sr, owned);
}

template <bool BF16>
__global__ __launch_bounds__(kAppendThreads) void kvappend_mla_fp8_kernel(const KvAppendMlaParams p) {
    const int tok = blockIdx.x;
    const int b = tok / p.Nnew, i = tok - b * p.Nnew;
    kvappend_mla_fp8_token<BF16>(p, b, i, p.Nnew, b, i, true);
}

template <bool BF16>
__global__ __launch_bounds__(kAppendThreads) void kvappend_mla_varlen_fp8_kernel(const KvAppendMlaParams p) {
    const int t = blockIdx.x;
    int s, i, nnew;
    const bool owned = kvappend_varlen_token(p.cu, p.B, t, &s, &i, &nnew);
    kvappend_mla_fp8_token<BF16>(p, owned ? s : 0, owned ? i : 0, owned ? nnew : 1, 0, t, owned);
}

#endif  // __HIPCC__

}  // namespace fa2

#if defined(__HIPCC__)
namespace fa2 {
// kvappend_mla_fp8_hip.cpp: the 16-bit launcher's grid and workgroup
FA2_LAUNCHER(launch_kvappend_mla_fp8, (const KvAppendMlaParams& p, int64_t groups, bool packed, hipStream_t stream), (p, groups, packed, stream))
}  // namespace fa2
#endif
