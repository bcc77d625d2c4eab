// fa2_mla_indexer.hip.h — the lightning indexer's logits for sparse MLA decode (fa2_mla_indexer_logits; include/fa2_gfx950.h has the contract, DESIGN.md
// section 34 the reasons): what names the lists fa2_fwd_decode_mla_sparse consumes.  Per sequence b and new token i of Nq, pos = len_b - Nq + i:
//
//   logits[b, i, s] = sum over heads h of  w[b, i, h] * max(0, q_idx[b, i, h, :] . k_idx[b, s, :])      0 <= s <= pos
//   logits[b, i, s] = -inf                                                                               pos < s < capacity
//
// The index-key cache holds ONE row of 128 columns per token, shared by all indexer heads; it is a contiguous cache or a pool of pages under the block
// table of the latent cache.  The kernel is a stream over that cache with no LDS and no barrier:
//
//   work split   one workgroup of four independent waves per (chunk of kIdxChunk consecutive key positions, token i, sequence b).  A wave takes the
//                chunk's units of 64 keys in turn (unit w, w + 4, ..); a unit is four 16-key tiles.  A chunk wholly beyond pos stores -inf and loads
//                nothing — no Q, no block-table entry.
//   Q            each wave holds the token's whole [H_idx, 128] Q as MFMA A fragments for the sweep: HB = H_idx / 16 head blocks x 4 k-steps x 4
//                registers (64 at H_idx 64), and its lane's 4 HB weights.
//   K            B = K^T: lane l loads the 16 bytes (key l % 16 of the tile, columns 32 kstep + 8 (l / 16) ..) straight from memory into the operand
//                registers; the 16 loads of a unit are issued together (4 KiB per wave in flight).  Every load is unconditional: the row a lane asks
//                for is min(its key, pos), so a lane whose key lies beyond pos re-reads a live row of the same page and a unit beyond pos re-reads row
//                pos (csrc/fa2_decode_mla_sparse.hip.h's lesson: a load predicated per lane makes the compiler wait for every load in flight).  What
//                such a lane computes is replaced by -inf before the store, by a select on the position.
//   heads on M   v_mfma_f32_16x16x32 with A = Q (16 heads x 32 columns), B = K^T (32 columns x 16 keys): a lane's four accumulators are four heads of
//                ONE key, so the ReLU, the weight and the sum over the lane's 4 HB (head block, j) values are in-lane max / fma in one fixed order;
//                two cross-row adds (lane ^ 16, lane ^ 32) finish the key.  HB x 4 MFMAs per 16 keys.
//   stores       the four tiles of a unit leave every lane the logits of keys l % 16 of each tile; lane l keeps tile l / 16, so the wave stores 64
//                consecutive float32 with one instruction.
//
// One summation order for every key: a row's bits depend on its own q, w and key row alone — not on the batch, the chunk or the layout (paged equals
// contiguous bit for bit).
// Safety (the lengths and the block table are device data nobody validated): len is clamped into [0, capacity_keys] (decode_clamp_len), page ids into
// the pool (prefill_clamp_page); a row index is at most pos < len, so a contiguous capacity that is no multiple of the tile is never read past its end,
// and only pages that hold a key at or below pos are addressed — the block-table entries of all others are never read.
#pragma once
#include <stdint.h>

#include "fa2_decode_mla.hip.h"      // decode_clamp_len, mla_page_keys, prefill_clamp_page, decode_mfma, the vector types

namespace fa2 {

constexpr int kIdxD = 128;                  // the index head dim: four k-steps of 32
constexpr int kIdxTile = 16;                // keys per MFMA tile
constexpr int kIdxUnit = 64;                // keys per store: divides every page size, so a unit never straddles a page
constexpr int kIdxWaves = 4;
constexpr int kIdxUnitsPerWave = 2;
constexpr int kIdxChunk = kIdxWaves * kIdxUnitsPerWave * kIdxUnit;      // 512 keys per workgroup
constexpr int kIdxMaxHeads = 64;

struct MlaIndexerParams {
    const void *q, *k;          // q_idx [B, Nq, H, 128], k_idx_cache [B, Nmax, 128] or [num_pages, page_size, 128]
    const float* w;             // weights [B, Nq, H] f32, the head dim contiguous
    float* logits;              // [B, Nq, capacity_keys] f32, the key dim contiguous
    const int* lens;            // cache_seqlens [B], device
    const int* bt;              // block_table (paged) or null
    int B, H, Nq;
    int page_size, num_pages;   // page_size 0 = contiguous cache
    int64_t capacity_keys;      // Nmax, or max_pages * page_size
    int64_t qs[3], ks[2], ws[2], ls[2], bts;      // element strides: q {batch, head, row}, k {batch | page, row}, w and logits {batch, row}
};

FA2_DEC_HD inline int mla_indexer_chunks(int64_t capacity_keys) { return (int)((capacity_keys + kIdxChunk - 1) / kIdxChunk); }
FA2_DEC_HD inline bool mla_indexer_heads_ok(int H) { return H >= 16 && H <= kIdxMaxHeads && H % 16 == 0; }

#if defined(__HIPCC__)

template <bool BF16, int HB>
__global__ __launch_bounds__(kIdxWaves * 64) void mla_indexer_logits_kernel(const MlaIndexerParams p) {
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
    const uint16_t* const qrow = static_cast<const uint16_t*>(p.q) + b * p.qs[0] + i * p.qs[2];
    u32x4 qf[HB][4];
    float wt[HB][4];
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
        const uint16_t* const qh = qrow + (hb * 16 + kr) * p.qs[1] + 8 * g;
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) qf[hb][kc] = *reinterpret_cast<const u32x4*>(qh + 32 * kc);
        const float* const wh = p.w + b * p.ws[0] + i * p.ws[1] + hb * 16 + 4 * g;      // (4-byte aligned rows: four scalar loads)
#pragma unroll
        for (int j = 0; j < 4; ++j) wt[hb][j] = wh[j];
    }
    const int page_keys = mla_page_keys(p.page_size, p.capacity_keys);
    const uint16_t* const kbase = static_cast<const uint16_t*>(p.k);
#pragma unroll
    for (int uu = 0; uu < kIdxUnitsPerWave; ++uu) {
        const int ukey = c0 + (uu * kIdxWaves + w) * kIdxUnit;           // wave-uniform
        if (ukey >= cap) break;
        // the page every row of this unit is read from: the unit's own, or — a unit beyond pos — the page of row pos
        const int anchor = ukey < pos ? ukey : pos;
        const int slot = anchor / page_keys, page0 = slot * page_keys;
        int64_t base = b * p.ks[0];
        if (p.page_size) base = (int64_t)prefill_clamp_page(p.bt[b * p.bts + slot], p.num_pages) * p.ks[0];
        const uint16_t* const kp = kbase + base + 8 * g;
        u32x4 kf[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int key = ukey + t * kIdxTile + kr;
            const uint16_t* const kt = kp + (int64_t)((key < pos ? key : pos) - page0) * p.ks[1];
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) kf[t][kc] = *reinterpret_cast<const u32x4*>(kt + 32 * kc);
        }
        float mine = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float sum = 0.f;
#pragma unroll
            for (int hb = 0; hb < HB; ++hb) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kc = 0; kc < 4; ++kc) acc = decode_mfma<BF16>(qf[hb][kc], kf[t][kc], acc);
#pragma unroll
                for (int j = 0; j < 4; ++j) sum = __builtin_fmaf(wt[hb][j], __builtin_fmaxf(acc[j], 0.f), sum);
            }
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            mine = g == t ? sum : mine;
        }
        const int s = ukey + lane;
        if (s < cap) out[s] = s <= pos ? mine : ninf;
    }
}

#endif  // __HIPCC__

}  // namespace fa2

#if defined(__HIPCC__)
#include "fa2_launch.h"
namespace fa2 {
// mla_indexer_hip.cpp: the kernel above for H / 16 head blocks on a grid of (chunks, Nq, B) workgroups
FA2_LAUNCHER(launch_mla_indexer_logits, (const MlaIndexerParams& p, hipStream_t stream), (p, stream))
}  // namespace fa2
#endif
