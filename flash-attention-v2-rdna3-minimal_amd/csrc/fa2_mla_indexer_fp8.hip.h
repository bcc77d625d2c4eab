// fa2_mla_indexer_fp8.hip.h — the lightning indexer's logits over an E4M3 index-key cache (fa2_mla_indexer_logits_fp8; include/fa2_gfx950.h has the
// contract, DESIGN.md section 35 the reasons): DeepGEMM's fp8_paged_mqa_logits on gfx950, the FP8 operands going to the matrix pipe as they are.
// A token's index key is 128 OCP e4m3 codes and ONE float32 scale; codes and scales are addressed separately (byte strides / element strides), so the
// library's rows of 132 bytes and vLLM's blocks (a page's codes, then its scales) are two views of this one kernel.  With pos = len_b - Nq + i:
//
//   logits[b, i, s] = k_scale[b, s] * sum over heads h of  w'[b, i, h] * max(0, q8[b, i, h, :] . k8[b, s, :])      0 <= s <= pos
//   logits[b, i, s] = -inf                                                                                         pos < s < capacity
//
// The work split, the unconditional loads of row min(key, pos) through pos's page, the select before the store, the store of key ukey + lane and the
// one summation order are csrc/fa2_mla_indexer.hip.h's (no LDS, no barrier).  What differs:
//
//   one MFMA     an index row is 128 columns: ONE v_mfma_f32_16x16x128_f8f6f4 (cbsz = blgp = 0: e4m3 x e4m3) per (16 heads x 16 keys), where the
//                16-bit kernel issues four 16x16x32.  Rows, columns and accumulators map as there: A row = lane % 16 (a head), B column = lane % 16 (a
//                key), a lane's four accumulators are heads 4 (lane / 16) + j of key lane % 16.
//   columns      the reduction runs over all 128 columns, so which 32 of them a lane group g = lane / 16 holds is free as long as Q and K agree.  Here
//                group g holds columns 16 g .. 16 g + 15 and 64 + 16 g .. 64 + 16 g + 15, in this order in its 8 operand registers: each of a tile's
//                two load instructions then reads 64 CONTIGUOUS bytes of each of its 16 rows (the four groups side by side) — whole rows' halves,
//                whatever the pitch — where 32 contiguous columns per group would read four separate 16-byte pieces per row and instruction.
//   alignment    a row of the 132-byte form is only 4-byte aligned: the 16-byte loads go through a vector type of alignment 4 (global_load_dwordx4
//                needs no more than a dword boundary).
//   Q            8 registers per head block (32 at H_idx 64, half the 16-bit kernel's).  q_idx in e4m3 is loaded as it is (the caller folded the q
//                scales into the weights); q_idx in 16 bits is quantised in the prologue per (token, head): the head's 128 columns sit in the lanes
//                l, l ^ 16, l ^ 32, l ^ 48, so amax is two cross-lane maxima; s = amax / 448 (an all-zero head: 1), code = e4m3(clamp(x / s, +-448))
//                by append_quant8 (the correctly rounded division), w' = w * s.  mla_indexer_q_to_fp8 (FlashAttn.py) is this arithmetic in torch.
//   K            8 registers per 16-key tile, 32 per unit.  BOTH units of a wave are loaded before the first MFMA: 16 loads of 1 KiB, the 16 KiB per
//                wave the 16-bit kernel has in flight, in half its registers (section 35 has the table: the halved footprint buys waves per SIMD).
//   key scale    one float32 per lane and unit, coalesced: lane l reads the scale of key min(ukey + l, pos), the key whose logit it stores, and
//                multiplies once, after the two cross-row adds.  A NaN or negative scale gives what the formula gives.
//
// Safety is the 16-bit kernel's: len clamped into [0, capacity_keys], page ids into the pool, a row index at most pos < len, so dead rows, dead scales
// and dead pages are never addressed and the block-table entries of pages beyond pos never read.
#pragma once
#include <stdint.h>

#include "fa2_mla_indexer.hip.h"     // the work split's constants, mla_indexer_chunks, mla_indexer_heads_ok
#include "fa2_kvappend.hip.h"        // append_unpack8, append_quant8

namespace fa2 {

enum { kIdxQE4M3 = 0, kIdxQF16 = 1, kIdxQBF16 = 2 };      // the q form a kernel is instantiated for

struct MlaIndexerFp8Params {
    const void* q;              // q_idx [B, Nq, H, 128]: e4m3 codes or the 16-bit dtype
    const uint8_t* k;           // the codes: 128 bytes per token
    const float* ksc;           // the scales: one per token
    const float* w;             // weights [B, Nq, H] f32, the head dim contiguous
    float* logits;              // [B, Nq, capacity_keys] f32, the key dim contiguous
    const int* lens;            // cache_seqlens [B], device
    const int* bt;              // block_table (paged) or null
    int B, H, Nq;
    int page_size, num_pages;   // page_size 0 = contiguous cache
    int64_t capacity_keys;
    int64_t qs[3];              // q element strides {batch, head, row}
    int64_t ks[2], ss[2];       // codes BYTE strides and scales ELEMENT strides {batch | page, row}
    int64_t ws[2], ls[2], bts;
};

#if defined(__HIPCC__)

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));      // sixteen bytes on a dword boundary

// the 32 code bytes of lane group g: columns 16 g .. and 64 + 16 g .. of a row of 128 codes
__device__ __forceinline__ i32x8 idx_fp8_operand(const uint8_t* row, int g) {
    const u32x4_a4 lo = *reinterpret_cast<const u32x4_a4*>(row + 16 * g), hi = *reinterpret_cast<const u32x4_a4*>(row + 64 + 16 * g);
    return (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// ... of a 16-bit head whose 32 columns of this group were loaded as `raw`, quantised with the head's own scale; *s = that scale in every lane that
// holds a part of the head
template <bool BF16>
__device__ __forceinline__ i32x8 idx_fp8_quant_q(const u32x4 (&raw)[4], float* s) {
    float x[4][8];
    float m = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        append_unpack8<BF16>(raw[c], x[c]);
#pragma unroll
        for (int e = 0; e < 8; ++e) m = __builtin_fmaxf(m, __builtin_fabsf(x[c][e]));
    }
    m = __builtin_fmaxf(m, __shfl_xor(m, 16, 64));
    m = __builtin_fmaxf(m, __shfl_xor(m, 32, 64));
    *s = m > 0.f ? m / 448.0f : 1.0f;
    i32x8 r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const u32x2 code = append_quant8(x[c], *s);
        r[2 * c] = (int)code[0];
        r[2 * c + 1] = (int)code[1];
    }
    return r;
}

template <int QF, int HB>
__global__ __launch_bounds__(kIdxWaves * 64) void mla_indexer_logits_fp8_kernel(const MlaIndexerFp8Params p) {
    const float ninf = -__builtin_inff();
    const int i = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, kr = lane & 15;
    const int cap = (int)p.capacity_keys;
    const int len = decode_clamp_len(p.lens[b], p.capacity_keys);
    const int pos = len - p.Nq + i;
    const int c0 = blockIdx.x * kIdxChunk;
    float* const out = p.logits + b * p.ls[0] + i * p.ls[1];
    if (c0 > pos) {                                                       // the chunk holds no key of this row: -inf, and nothing is loaded
        for (int s = c0 + tid; s < c0 + kIdxChunk && s < cap; s += kIdxWaves * 64) out[s] = ninf;
        return;
    }
    i32x8 qf[HB];
    float wt[HB][4];
    const int64_t qrow = b * p.qs[0] + i * p.qs[2] + kr * p.qs[1];
    const float* const wrow = p.w + b * p.ws[0] + i * p.ws[1] + 4 * g;    // (4-byte aligned rows: four scalar loads per head block)
    if constexpr (QF == kIdxQE4M3) {
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) {
            qf[hb] = idx_fp8_operand(static_cast<const uint8_t*>(p.q) + qrow + hb * 16 * p.qs[1], g);
#pragma unroll
            for (int j = 0; j < 4; ++j) wt[hb][j] = wrow[hb * 16 + j];
        }
    } else {
        // every load first (16 registers per head block, dead once it is quantised), then one head block at a time: the f32 image of a block is 32
        // registers, and the fence keeps the compiler from unpacking all of them at once (244 VGPRs at H_idx 64 without it)
        u32x4 raw[HB][4];
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) {
            const uint16_t* const qh = static_cast<const uint16_t*>(p.q) + qrow + hb * 16 * p.qs[1] + 16 * g;
#pragma unroll
            for (int c = 0; c < 4; ++c) raw[hb][c] = *reinterpret_cast<const u32x4*>(qh + 64 * (c >> 1) + 8 * (c & 1));
#pragma unroll
            for (int j = 0; j < 4; ++j) wt[hb][j] = wrow[hb * 16 + j];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) {
            float s;
            qf[hb] = idx_fp8_quant_q<QF == kIdxQBF16>(raw[hb], &s);
#pragma unroll
            for (int j = 0; j < 4; ++j) wt[hb][j] *= __shfl(s, 4 * g + j, 64);      // head 4 g + j of the block: lane 4 g + j holds its scale
            asm volatile("" : "+v"(qf[hb]));                      // the codes exist HERE: the compiler would sink the divisions below the K loads
            __builtin_amdgcn_sched_barrier(0);                    // (the last one also keeps the K loads below the prologue's peak)
        }
    }
    const int page_keys = mla_page_keys(p.page_size, p.capacity_keys);
    i32x8 kf[kIdxUnitsPerWave][4];
    float ksc[kIdxUnitsPerWave];
#pragma unroll
    for (int uu = 0; uu < kIdxUnitsPerWave; ++uu) {                       // every load of the wave's units, before the first MFMA
        // a unit at or beyond the capacity (the last chunk) reads what a unit beyond pos reads — row pos — and stores nothing
        const int ukey = c0 + (uu * kIdxWaves + w) * kIdxUnit;           // wave-uniform
        const int anchor = ukey < pos ? ukey : pos;
        const int slot = anchor / page_keys, page0 = slot * page_keys;
        const int64_t base = p.page_size ? (int64_t)prefill_clamp_page(p.bt[b * p.bts + slot], p.num_pages) : (int64_t)b;
        const uint8_t* const kp = p.k + base * p.ks[0];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int key = ukey + t * kIdxTile + kr;
            kf[uu][t] = idx_fp8_operand(kp + (int64_t)((key < pos ? key : pos) - page0) * p.ks[1], g);
        }
        const int mykey = ukey + lane;
        ksc[uu] = p.ksc[base * p.ss[0] + (int64_t)((mykey < pos ? mykey : pos) - page0) * p.ss[1]];
    }
#pragma unroll
    for (int uu = 0; uu < kIdxUnitsPerWave; ++uu) {
        const int ukey = c0 + (uu * kIdxWaves + w) * kIdxUnit;
        if (ukey >= cap) break;
        float mine = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float sum = 0.f;
#pragma unroll
            for (int hb = 0; hb < HB; ++hb) {
                const f32x4 acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(qf[hb], kf[uu][t], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0, 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) sum = __builtin_fmaf(wt[hb][j], __builtin_fmaxf(acc[j], 0.f), sum);
            }
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            mine = g == t ? sum : mine;
        }
        const int s = ukey + lane;
        if (s < cap) out[s] = s <= pos ? mine * ksc[uu] : ninf;
    }
}

#endif  // __HIPCC__

}  // namespace fa2

#if defined(__HIPCC__)
#include "fa2_launch.h"
namespace fa2 {
// mla_indexer_fp8_hip.cpp: the kernel above for a q form and H / 16 head blocks on a grid of (chunks, Nq, B) workgroups
FA2_HIDDEN int launch_mla_indexer_logits_fp8(int q_form, const MlaIndexerFp8Params& p, hipStream_t stream);
}  // namespace fa2
#endif
