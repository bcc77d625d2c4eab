// fa2_mla_indexer_prefill_fp8.hip.h — the lightning indexer's logits for PACKED query tokens over an E4M3 index-key cache
// (fa2_mla_indexer_logits_varlen_fp8; include/fa2_gfx950.h has the contract, DESIGN.md section 36 the reasons): the prefill side of
// csrc/fa2_mla_indexer_fp8.hip.h.  Packed token t belongs to the sequence s that kvappend_varlen_token names (i = t - cu[s], Nq_s = cu[s + 1] - cu[s]);
// with pos = clamp_len(len_s) - Nq_s + i:
//
//   logits[t, j] = k_scale[s, j] * sum over heads h of  w'[t, h] * max(0, q8[t, h, :] . k8[s, j, :])      0 <= j <= pos
//   logits[t, j] = -inf                                                                                   pos < j < capacity
//
// and a token no sequence owns, or one at a negative position, is all -inf.  Where the decode kernel streams the keys past ONE token's Q in registers,
// this one holds the KEYS in registers and streams the tokens past them:
//
//   work split   one workgroup of eight waves per (chunk of kIdxPfChunk = 1 024 consecutive key positions, block of kIdxPfTokens = 128 consecutive
//                packed tokens).  Wave w owns the 128 keys c0 + 128 w ..: eight 16-key tiles as MFMA B operands (64 registers, loaded by
//                idx_fp8_operand: section 35's two 64-byte-per-row loads and its column order) and their scales (lane l: keys l and 64 + l of the 128).
//   ownership    the first 128 threads find (s, pos) of the block's tokens once, into LDS, with `last`: the largest position the block serves in that
//                sequence, min(len_s - 1, pos + tokens left in the block) — the same for every token of s in the block.
//   keys         a wave walks the tokens in order.  A token that is not owned, or whose pos lies below the wave's first key, gets the wave's -inf
//                stores and nothing else.  Otherwise, when the token's sequence is not the one whose keys the wave holds (wave-uniform), it loads
//                them: row min(key, last) through the page of min(unit's first key, last) — unconditional loads of live rows, as in the decode kernel,
//                with `last` where that kernel has pos.  The keys beyond a token's own pos are live rows of its sequence whose products the select
//                before the store replaces by -inf.  A block of decode rows therefore loads what the decode kernel loads; a prefill chunk uses each
//                key row for up to 128 tokens.
//   Q            tokens cross LDS in groups of four (e4m3 q) or two (16-bit q: twice the bytes per token, the same 16 registers of loads in flight
//                at H_idx 64; four spilled).  A token's image is H_idx rows of 128 code bytes and H_idx weights.  Two buffers; the
//                next group's global loads (16 bytes per lane and load) are issued before the current group's MFMAs, its LDS writes come after them,
//                and ONE barrier ends the group (every read of a buffer lies before the barrier that precedes its next write).  A 16-bit q_idx is
//                quantised between its load and the LDS write, once per (workgroup, token): sixteen lanes hold a head's 128 columns, four cross-lane
//                maxima give amax, and s, the codes and w' = w * s are idx_fp8_quant_q's arithmetic (any order of maxima gives the same amax).
//   swizzle      the image's row pitch is 128 bytes, and the sixteen lanes of a lane group read the SAME 16-byte column of sixteen head rows.  A row's
//                16-byte unit u is therefore stored at unit u ^ ((row / 2) % 8): rows 2 r and 2 r + 1 keep their unit, neighbouring pairs permute it,
//                so the sixteen reads of a ds_read_b128 quarter cover sixteen different 16-byte slots of 256 bytes.  XOR, not padding: the image stays
//                a power of two and the 16-bit path's 8-byte writes stay inside one unit.
//   per token    HB x 8 MFMAs per wave, then section 35's epilogue and summation order exactly — one v_mfma_f32_16x16x128_f8f6f4 per (16 heads x 16
//                keys), head blocks ascending and j ascending through fmaf(w, max(acc, 0), sum), the lane ^ 16 add, the lane ^ 32 add, the key scale
//                last — so a packed call equals the uniform call on each sequence bit for bit.  Two coalesced stores of 64 floats per wave and token.
//
// Safety (cu_seqlens_q, the lengths and the block table are device data nobody validated): a token index is below total_q before any q or weight row is
// addressed; a sequence index comes from kvappend_varlen_token alone, which names s in [0, B) with 0 <= i < Nq_s or nothing; len is clamped into
// [0, capacity_keys], page ids into the pool; a row index is at most last < len_s, so dead rows, dead scales and dead pages are never addressed and
// the block-table entries of pages beyond `last` are never read.
#pragma once
#include <stdint.h>

#include "fa2_mla_indexer_fp8.hip.h"      // idx_fp8_operand, the q forms, the unit's includes

namespace fa2 {

constexpr int kIdxPfWaves = 8;
constexpr int kIdxPfThreads = kIdxPfWaves * 64;
constexpr int kIdxPfWaveKeys = 2 * kIdxUnit;                     // two store units of 64 keys: eight MFMA tiles
constexpr int kIdxPfChunk = kIdxPfWaves * kIdxPfWaveKeys;        // 1 024 keys per workgroup
constexpr int kIdxPfTokens = 128;                                // packed tokens per workgroup
// tokens per LDS buffer: four e4m3 tokens, or two 16-bit ones (the same 16 registers of loads in flight per lane at H_idx 64)
FA2_DEC_HD inline constexpr int mla_indexer_prefill_group(int q_form) { return q_form == kIdxQE4M3 ? 4 : 2; }

struct MlaIndexerPrefillParams {
    const void* q;              // q_idx [total_q, H, 128]: e4m3 codes or the 16-bit dtype
    const uint8_t* k;           // the codes: 128 bytes per token
    const float* ksc;           // the scales: one per token
    const float* w;             // weights [total_q, H] f32, the head dim contiguous
    float* logits;              // [total_q, capacity_keys] f32, the key dim contiguous
    const int* cu;              // cu_seqlens_q [B + 1], device
    const int* lens;            // cache_seqlens [B], device
    const int* bt;              // block_table (paged) or null
    int B, H, total_q;
    int page_size, num_pages;   // page_size 0 = contiguous cache
    int64_t capacity_keys;
    int64_t qs[2];              // q element strides {token, head}
    int64_t ks[2], ss[2];       // codes BYTE strides and scales ELEMENT strides {batch | page, row}
    int64_t ws, ls, bts;        // weights and logits row strides, the block table's
};

FA2_DEC_HD inline int mla_indexer_prefill_chunks(int64_t capacity_keys) { return (int)((capacity_keys + kIdxPfChunk - 1) / kIdxPfChunk); }
FA2_DEC_HD inline int64_t mla_indexer_prefill_blocks(int64_t total_q) { return (total_q + kIdxPfTokens - 1) / kIdxPfTokens; }
// dynamic LDS: the block's (s, pos, last) entries, then two buffers of a group's token images
FA2_DEC_HD inline int mla_indexer_prefill_lds(int H, int q_form) { return kIdxPfTokens * 16 + 2 * mla_indexer_prefill_group(q_form) * H * (kIdxD + 4); }
// where unit `u` (16 bytes) of row `row` of a token image lives: see "swizzle"
FA2_DEC_HD inline int mla_indexer_prefill_unit(int row, int u) { return row * kIdxD + ((u ^ ((row >> 1) & 7)) << 4); }

#if defined(__HIPCC__)

typedef int i32x4 __attribute__((ext_vector_type(4)));

template <int QF, int HB>
__global__ __launch_bounds__(kIdxPfThreads) void mla_indexer_prefill_fp8_kernel(const MlaIndexerPrefillParams p) {
    constexpr int H = HB * 16, TOK = H * kIdxD, GROUP = mla_indexer_prefill_group(QF), BUF = GROUP * (TOK + H * 4), WOFS = GROUP * TOK;
    constexpr int NLOAD = HB;                                             // 16-byte loads per lane and group
    extern __shared__ __attribute__((aligned(16))) uint8_t idx_pf_lds[];
    i32x4* const meta = reinterpret_cast<i32x4*>(idx_pf_lds);
    uint8_t* const bufs = idx_pf_lds + kIdxPfTokens * 16;
    const float ninf = -__builtin_inff();
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, kr = lane & 15;
    const int cap = (int)p.capacity_keys;
    const int t0 = blockIdx.y * kIdxPfTokens;                             // (< total_q: the grid covers ceil(total_q / 128) blocks)
    const int nt = p.total_q - t0 < kIdxPfTokens ? p.total_q - t0 : kIdxPfTokens;
    const int wbase = blockIdx.x * kIdxPfChunk + w * kIdxPfWaveKeys;      // wave-uniform: the wave's first key

    if (tid < kIdxPfTokens) {                                             // ---- ownership, once per (workgroup, token)
        int s = -1, pos = -1, last = -1, sq, i, nq;
        if (tid < nt && kvappend_varlen_token(p.cu, p.B, (int64_t)t0 + tid, &sq, &i, &nq)) {
            const int len = decode_clamp_len(p.lens[sq], p.capacity_keys), rest = nt - 1 - tid;
            pos = len - nq + i;                                           // (nq - 1 - i >= 0 tokens of s follow: pos <= len - 1)
            if (pos >= 0) {
                s = sq;
                last = nq - 1 - i > rest ? pos + rest : len - 1;
            } else {
                pos = -1;
            }
        }
        meta[tid] = (i32x4){s, pos, last, 0};
    }

    // ---- staging: group gi's tokens t0 + 4 gi .. through registers into buffer gi % 2
    u32x4 raw[NLOAD];
    float wraw[QF == kIdxQE4M3 ? 1 : NLOAD];
    auto stage_load = [&](int gi) __attribute__((always_inline)) {
        const int tg0 = t0 + gi * GROUP;
#pragma unroll
        for (int it = 0; it < NLOAD; ++it) {
            const int u = it * kIdxPfThreads + tid;
            if constexpr (QF == kIdxQE4M3) {
                const int tg = u / (H * 8), h = (u % (H * 8)) >> 3, c = u & 7;
                const int t = tg0 + tg < p.total_q ? tg0 + tg : p.total_q - 1;
                raw[it] = *reinterpret_cast<const u32x4*>(static_cast<const uint8_t*>(p.q) + t * p.qs[0] + h * p.qs[1] + 16 * c);
            } else {
                const int hh = u >> 4, tg = hh / H, h = hh % H;
                const int t = tg0 + tg < p.total_q ? tg0 + tg : p.total_q - 1;
                raw[it] = *reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(p.q) + t * p.qs[0] + h * p.qs[1] + 8 * kr);
            }
        }
        if constexpr (QF == kIdxQE4M3) {
            const int tg = tid / H, t = tg0 + tg < p.total_q ? tg0 + tg : p.total_q - 1;
            wraw[0] = tid < GROUP * H ? p.w[t * p.ws + tid % H] : 0.f;
        }
    };
    auto stage_store = [&](int gi) __attribute__((always_inline)) {
        uint8_t* const buf = bufs + (gi & 1) * BUF;
        if constexpr (QF != kIdxQE4M3) {                                  // (the heads' weights: loaded here, so that they are not live across the MFMAs)
#pragma unroll
            for (int it = 0; it < NLOAD; ++it) {
                const int hh = (it * kIdxPfThreads + tid) >> 4, t = t0 + gi * GROUP + hh / H;
                wraw[it] = p.w[(t < p.total_q ? t : p.total_q - 1) * p.ws + hh % H];
            }
        }
#pragma unroll
        for (int it = 0; it < NLOAD; ++it) {
            const int u = it * kIdxPfThreads + tid;
            if constexpr (QF == kIdxQE4M3) {
                const int tg = u / (H * 8), h = (u % (H * 8)) >> 3, c = u & 7;
                *reinterpret_cast<u32x4*>(buf + tg * TOK + mla_indexer_prefill_unit(h, c)) = raw[it];
            } else {
                const int hh = u >> 4, tg = hh / H, h = hh % H;
                float x[8];
                append_unpack8<QF == kIdxQBF16>(raw[it], x);
                float m = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) m = __builtin_fmaxf(m, __builtin_fabsf(x[e]));
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) m = __builtin_fmaxf(m, __shfl_xor(m, d, 64));
                const float s = m > 0.f ? m / 448.0f : 1.0f;
                *reinterpret_cast<u32x2*>(buf + tg * TOK + mla_indexer_prefill_unit(h, kr >> 1) + 8 * (kr & 1)) = append_quant8(x, s);
                if (kr == 0) reinterpret_cast<float*>(buf + WOFS)[tg * H + h] = wraw[it] * s;
                __builtin_amdgcn_sched_barrier(0);                        // one head part at a time: its f32 image and the division's temporaries die here
            }
        }
        if constexpr (QF == kIdxQE4M3) {
            if (tid < GROUP * H) reinterpret_cast<float*>(buf + WOFS)[tid] = wraw[0];
        }
    };

    const int ngroups = (nt + GROUP - 1) / GROUP;
    stage_load(0);
    stage_store(0);
    __syncthreads();                                                      // (the ownership entries too)

    const int page_keys = mla_page_keys(p.page_size, p.capacity_keys);
    i32x8 kf[8];
    float ksc[2] = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 8; ++t) kf[t] = (i32x8){0, 0, 0, 0, 0, 0, 0, 0};
    int held = -1;                                                        // the sequence whose keys the wave holds

    for (int gi = 0; gi < ngroups; ++gi) {
        const bool more = gi + 1 < ngroups;                               // workgroup-uniform
        if (more) stage_load(gi + 1);
        const uint8_t* const buf = bufs + (gi & 1) * BUF;
        if (wbase < cap) {
#pragma unroll
            for (int tg = 0; tg < GROUP; ++tg) {
                const int tl = gi * GROUP + tg;
                if (tl >= nt) break;
                const i32x4 mt = meta[tl];
                const int s = __builtin_amdgcn_readfirstlane(mt[0]), pos = __builtin_amdgcn_readfirstlane(mt[1]);
                const int last = __builtin_amdgcn_readfirstlane(mt[2]);
                float* const out = p.logits + (int64_t)(t0 + tl) * p.ls;
                if (s < 0 || pos < wbase) {                               // no key of this wave is live for the token: -inf, nothing is loaded
#pragma unroll
                    for (int uu = 0; uu < 2; ++uu)
                        if (wbase + uu * kIdxUnit + lane < cap) out[wbase + uu * kIdxUnit + lane] = ninf;
                    continue;
                }
                if (s != held) {                                          // wave-uniform: the keys of the new sequence, rows at most `last`
                    held = s;
#pragma unroll
                    for (int uu = 0; uu < 2; ++uu) {
                        const int ukey = wbase + uu * kIdxUnit;
                        const int anchor = ukey < last ? ukey : last;
                        const int slot = anchor / page_keys, page0 = slot * page_keys;
                        const int64_t base = p.page_size ? (int64_t)prefill_clamp_page(p.bt[s * p.bts + slot], p.num_pages) : (int64_t)s;
                        const uint8_t* const kp = p.k + base * p.ks[0];
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const int key = ukey + t * kIdxTile + kr;
                            kf[uu * 4 + t] = idx_fp8_operand(kp + (int64_t)((key < last ? key : last) - page0) * p.ks[1], g);
                        }
                        const int mykey = ukey + lane;
                        ksc[uu] = p.ksc[base * p.ss[0] + (int64_t)((mykey < last ? mykey : last) - page0) * p.ss[1]];
                    }
                }
                i32x8 qf[HB];
                f32x4 wt[HB];
                const uint8_t* const img = buf + tg * TOK;
#pragma unroll
                for (int hb = 0; hb < HB; ++hb) {
                    const int row = hb * 16 + kr;
                    const u32x4 lo = *reinterpret_cast<const u32x4*>(img + mla_indexer_prefill_unit(row, g));
                    const u32x4 hi = *reinterpret_cast<const u32x4*>(img + mla_indexer_prefill_unit(row, 4 + g));
                    qf[hb] = (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
                    wt[hb] = *reinterpret_cast<const f32x4*>(buf + WOFS + (tg * H + hb * 16 + 4 * g) * 4);
                }
#pragma unroll
                for (int uu = 0; uu < 2; ++uu) {
                    float mine = 0.f;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        float sum = 0.f;
#pragma unroll
                        for (int hb = 0; hb < HB; ++hb) {
                            const f32x4 acc =
                                __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(qf[hb], kf[uu * 4 + t], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0, 0, 0, 0);
#pragma unroll
                            for (int j = 0; j < 4; ++j) sum = __builtin_fmaf(wt[hb][j], __builtin_fmaxf(acc[j], 0.f), sum);
                        }
                        sum += __shfl_xor(sum, 16, 64);
                        sum += __shfl_xor(sum, 32, 64);
                        mine = g == t ? sum : mine;
                    }
                    const int j = wbase + uu * kIdxUnit + lane;
                    if (j < cap) out[j] = j <= pos ? mine * ksc[uu] : ninf;
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);                                // (the writes, and a 16-bit q's quantisation, stay behind the MFMAs)
        if (more) stage_store(gi + 1);
        __syncthreads();
    }
}

#endif  // __HIPCC__

}  // namespace fa2

#if defined(__HIPCC__)
#include "fa2_launch.h"
namespace fa2 {
// mla_indexer_prefill_fp8_hip.cpp: the kernel above for a q form and H / 16 head blocks on a grid of (key chunks, token blocks) workgroups
FA2_HIDDEN int launch_mla_indexer_prefill_fp8(int q_form, const MlaIndexerPrefillParams& p, hipStream_t stream);
}  // namespace fa2
#endif
