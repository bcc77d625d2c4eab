// fa2_kvappend_mla_index_fp8.hip.h — the QUANTISING append for the e4m3 index-key cache of the lightning indexer (fa2_kvcache_append_mla_index_fp8 and
// its packed form; include/fa2_gfx950.h has the contract, DESIGN.md section 35 the reasons): the write side of fa2_mla_indexer_logits_fp8.  One launch
// turns the new tokens' index keys (128 columns, fp16 / bf16) into 128 e4m3 codes and one float32 scale each, at the key position only the device knows.
//
//   work split   sixteen lanes — one DPP row — take a token, four tokens a wave, kIdxAppendTokens a workgroup; token T = 16 blockIdx.x + threadIdx.x / 16.
//                Lane c of the row loads columns 8 c .. 8 c + 7 (16 bytes; the row 256 contiguous bytes), takes their max |x|, and four DPP steps
//                (mla_fp8_row_max, section 33's) leave the token's amax in every lane of the row: no LDS, no barrier.
//   scale        amax / 448 in f32 (an all-zero row: 1.0f); with scale_pow2 the smallest power of two at or above it, from the exponent bits
//                (idx_fp8_pow2_bits: DeepSeek's ue8m0 choice).  code = e4m3(clamp(x / scale, +-448)) by append_quant8: the correctly rounded division.
//   stores       8 code bytes per lane as two dwords (a row of the 132-byte form is only 4-byte aligned), the scale by lane 0 of the row: vector
//                stores, plain C++.
//   skips        a token beyond the group count, a packed token no sequence owns, a position outside the cache (kvappend_slot) and a page id outside
//                the pool (mla_append_cache_row) load nothing and store nothing; nothing is clamped onto a live row.  Every cross-lane operation sits
//                outside the per-token branches.
// A NaN in k_idx: v_max_f32 drops it from the amax, it divides to a NaN, falls through the clamp (this unit honours NaNs) and becomes a NaN code.
#pragma once
#include <stdint.h>

#include "fa2_kvappend_mla_fp8.hip.h"      // mla_fp8_row_max, mla_append_cache_row, append_unpack8, append_quant8, kvappend_slot, kvappend_varlen_token

namespace fa2 {

constexpr int kIdxAppendThreads = 256;
constexpr int kIdxAppendTokens = kIdxAppendThreads / 16;

struct KvAppendMlaIndexParams {
    const void* x;              // k_idx [B, Nnew, 128] (packed: [total, 128]), the I/O dtype
    uint8_t* k;                 // the cache's codes
    float* ksc;                 // ... and scales
    const int* lens;            // cache_seqlens [B], device: the lengths AFTER the append
    const int* bt;              // block_table (paged) or null
    const int* cu;              // the packed call's cu_seqlens [B + 1], device; null: the uniform call
    int B, Nnew;                // (Nnew: the uniform call's)
    int page_size, num_pages, pow2;
    int64_t tokens;             // B * Nnew, or the packed call's total
    int64_t capacity_keys;
    int64_t xs[2];              // k_idx element strides {batch, row} (the packed call: {0, row})
    int64_t ks[3], ss[3];       // codes BYTE strides and scales ELEMENT strides {batch | page, -, row} (mla_append_cache_row's form)
    int64_t bts;
};

// The smallest power of two >= s for a positive normal s, from the bits (a denormal s gives 2^-126, Inf stays Inf); host and device
FA2_DEC_HD inline uint32_t idx_fp8_pow2_bits(uint32_t s_bits) { return (s_bits + 0x7fffffu) & 0x7f800000u; }

#if defined(__HIPCC__)

template <bool BF16>
__global__ __launch_bounds__(kIdxAppendThreads) void kvappend_mla_index_fp8_kernel(const KvAppendMlaIndexParams p) {
    const int c = threadIdx.x & 15;
    const int64_t t = (int64_t)blockIdx.x * kIdxAppendTokens + (threadIdx.x >> 4);
    int b = 0, i = 0, nnew = 1;
    int64_t sb = 0, sr = t;
    bool live = t < p.tokens;
    if (live) {
        if (p.cu) {
            live = kvappend_varlen_token(p.cu, p.B, t, &b, &i, &nnew);
        } else {
            b = (int)(t / p.Nnew); i = (int)(t - (int64_t)b * p.Nnew); nnew = p.Nnew;
            sb = b; sr = i;
        }
    }
    int64_t kofs = -1, sofs = -1;
    if (live) {
        const int64_t slot = kvappend_slot(p.lens[b], p.capacity_keys, nnew, i);
        if (slot >= 0) {
            kofs = mla_append_cache_row(slot, b, p.bt, p.bts, p.page_size, p.num_pages, p.ks);
            sofs = mla_append_cache_row(slot, b, p.bt, p.bts, p.page_size, p.num_pages, p.ss);
        }
    }
    live = live && kofs >= 0 && sofs >= 0;
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) append_unpack8<BF16>(*reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(p.x) + sb * p.xs[0] + sr * p.xs[1] + 8 * c), x);
    float m = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) m = __builtin_fmaxf(m, __builtin_fabsf(x[e]));
    const float amax = mla_fp8_row_max(m);                      // (all lanes: outside the branches)
    float scale = amax > 0.0f ? amax / 448.0f : 1.0f;
    if (p.pow2) scale = __builtin_bit_cast(float, idx_fp8_pow2_bits(__builtin_bit_cast(uint32_t, scale)));
    const u32x2 code = append_quant8(x, scale);
    if (!live) return;
    uint32_t* const dst = reinterpret_cast<uint32_t*>(p.k + kofs + 8 * c);
    dst[0] = code[0];
    dst[1] = code[1];
    if (c == 0) p.ksc[sofs] = scale;
}

#endif  // __HIPCC__

}  // namespace fa2

#if defined(__HIPCC__)
namespace fa2 {
// mla_indexer_fp8_hip.cpp: ceil(tokens / 16) workgroups of 256 lanes
FA2_HIDDEN int launch_kvappend_mla_index_fp8(bool bf16, const KvAppendMlaIndexParams& p, hipStream_t stream);
}  // namespace fa2
#endif
