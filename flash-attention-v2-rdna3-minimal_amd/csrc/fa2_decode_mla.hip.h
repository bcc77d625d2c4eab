// fa2_decode_mla.hip.h — decode attention on a multi-head-latent (MLA) KV cache (fa2_fwd_decode_mla; include/fa2_gfx950.h has the contract, DESIGN.md
// section 28 the reasons).
//
// The cache holds ONE row of 576 columns per token, shared by all heads: 512 of compressed KV and 64 of rotary key; its first 512 columns are also the
// value.  q [.., H, 576] is the absorbed query.  o[b, i, h] = softmax_j(scale * q[b, i, h, :] . kv[b, j, :]) . kv[b, j, :512] under decode's mask.
//
// One workgroup of four waves serves one item (sequence b, block rb of up to 64 packed rows r = i * H + h, part s).  The part sweeps the 32-key tiles
// mla_part_range gives it.  Every tile is loaded from memory ONCE per workgroup (16-byte loads, register staging) into a double-buffered LDS image of
// 32 rows of 1 152 + 16 bytes, and serves both products from there:
//
//   S^T[key, row] = K[key, :] . Q[row, :]       A = K fragment, ds_read_b128 from the image (the lane's key, 8 of its columns), B = Q fragment: the
//                                               wave's 16 rows x 576 columns stay in 72 registers for the whole sweep
//   O^T[d, row]  += V^T[d, key] . P^T[key, row]  A = V^T fragment: ds_read_b64_tr_b16 on the SAME image (columns 0 .. 511), in the k order the S^T
//                                               accumulator already has (fa2_decode.hip.h), B = P rounded to the I/O dtype; no lane movement
//
// Each wave owns one 16-row tile of the block — m, l and the 32 f32x4 accumulator blocks (128 registers) are private — so there is no merge across the
// waves at the end, and one workgroup barrier per key tile: tile t + 1 travels global -> registers while tile t is computed on, is written to the other
// buffer, and the barrier behind that write is the one that frees tile t's buffer (its readers have passed it).
//
// Safety (fa2_decode.hip.h's rules): len is clamped into [0, capacity_keys], every page id into [0, num_pages), every row index of a tile into its
// live rows before it becomes an address; addresses are formed in 64 bits.  Keys at or beyond len: their rows in the image are zero bits (a select on
// the staged registers; 0 * NaN is NaN) and their scores -inf (a select on the position).
#pragma once
#include <stdint.h>

#include "fa2_decode.hip.h"          // DecodeParams, decode_part_range, decode_clamp_len, decode_mfma, the group reductions, decode_combine_kernel
#include "fa2_prefill.h"             // prefill_page_keys, prefill_clamp_page

namespace fa2 {

constexpr int kMlaD = 576;             // columns of a cache row and of q: the contraction of S
constexpr int kMlaDv = 512;            // leading columns that are the value: the width of o
constexpr int kMlaTile = kDecodeTile;  // 32 keys: divides 64, so a tile never straddles a page
constexpr int kMlaBlockRows = 64;      // packed rows per workgroup: four waves, one 16-row tile each
constexpr int kMlaMaxHeads = 128;
constexpr int kMlaMaxRows = 512;       // Nq * H
// Parts per (sequence, row block).  A workgroup holds 73 KiB of LDS and more than 256 registers per lane: one per CU.  A B = 1 call on all 128 heads is
// two row blocks, so 128 parts put one workgroup on each of 256 CUs (decode's cap of 16 would leave it on 32 of them).  What bounds the split in
// practice is kMlaMinPartTiles: a part leaves 64 rows x 513 floats (128 KiB) for the combine kernel to read back, which is what 7 key tiles of the cache
// weigh (32 x 1 152 bytes each), so a part of fewer than 8 tiles moves more workspace than cache.
constexpr int kMlaMaxSplit = 128;
constexpr int kMlaMinPartTiles = 8;
constexpr int kMlaRowBytes = kMlaD * 2 + 16;                  // a key's row in the LDS image (the pad moves consecutive rows 4 banks apart)
constexpr int kMlaLdsBytes = 2 * kMlaTile * kMlaRowBytes;     // 74 752: two buffers

// ---- the arithmetic the host plan, the C-ABI (fa2_decode_mla_part_range, fa2_decode_mla_tile) and the kernel share
// the key tiles of a part: decode_part_range's rule on 32-key tiles (len clamped into [0, capacity_keys] there)
FA2_DEC_HD inline void mla_part_range(int64_t len, int64_t capacity_keys, int nsplit, int part, int* first, int* n) {
    decode_part_range(len, capacity_keys, 1, kMlaTile, nsplit, part, first, n);
}
// keys per page as the kernel counts them: a pool's page size, or — the contiguous layout, one page per sequence — the capacity in whole tiles
FA2_DEC_HD inline int mla_page_keys(int page_size, int64_t capacity_keys) { return prefill_page_keys(page_size, capacity_keys); }
// Tile t of a sequence of `len` keys (clamped already): the block-table slot of its page, its first row inside that page and how many of its 32 rows
// hold a key of the sequence (0: the tile lies at or beyond the length)
struct MlaTile { int slot, row, rows; };
FA2_DEC_HD inline MlaTile mla_tile(int t, int len, int page_keys) {
    const int64_t key0 = (int64_t)t * kMlaTile;
    const int64_t left = len - key0;
    MlaTile r;
    r.slot = (int)(key0 / page_keys);
    r.row = (int)(key0 - (int64_t)r.slot * page_keys);
    r.rows = left <= 0 ? 0 : left < kMlaTile ? (int)left : kMlaTile;
    return r;
}
// row blocks of a call
FA2_DEC_HD inline int mla_row_blocks(int rows) { return (rows + kMlaBlockRows - 1) / kMlaBlockRows; }

#if defined(__HIPCC__)

// DecodeParams as fa2_fwd_decode_mla fills it: k = the latent cache (v unused), Hkv = 1, G = H, rows = Nq * H, ks = {batch | page, -, row}
template <bool BF16>
__global__ __launch_bounds__(kDecodeWaves * 64) void decode_mla_kernel(const DecodeParams p) {
    constexpr int T = kMlaTile, DC = kMlaD / 32, DB = kMlaDv / 16, ROWB = kMlaRowBytes, BUF = T * ROWB;
    constexpr int CH = kMlaD / 8;                      // 16-byte chunks of a row: 72
    constexpr int NL = T * CH / (kDecodeWaves * 64);   // staged chunks per thread: 9
    static_assert(NL * kDecodeWaves * 64 == T * CH && T == 32, "tile geometry");
    extern __shared__ __attribute__((aligned(16))) char mla_lds[];
    const float ninf = -__builtin_inff();

    const int part = blockIdx.x, rb = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, qi = lane & 15;
    const int len = decode_clamp_len(p.lens[b], p.capacity_keys);
    int first, nt;
    mla_part_range(len, p.capacity_keys, p.nsplit, part, &first, &nt);
    float* const ws_o = p.ws + (((int64_t)b * p.nsplit + part) * p.rows) * kMlaDv;
    float* const ws_l = p.ws + (int64_t)p.B * p.nsplit * p.rows * kMlaDv + ((int64_t)b * p.nsplit + part) * p.rows;

    if (p.nsplit > 1 && nt == 0) {                     // an empty part: lse = -inf, no O (the combine never reads a part of weight 0)
        const int r = rb * kMlaBlockRows + tid;
        if (tid < kMlaBlockRows && r < p.rows) ws_l[r] = ninf;
        return;
    }

    // the lane's query row: packed row r = i * H + h -> query i, head h, at key position len - Nq + i
    const int r = rb * kMlaBlockRows + w * 16 + qi;
    const bool live = r < p.rows;
    const bool wave_live = rb * kMlaBlockRows + w * 16 < p.rows;      // (wave-uniform) a wave without rows stages and waits, no more
    const int qrow_i = live ? r / p.G : 0, qrow_h = live ? r % p.G : 0;
    const int pos = live ? len - p.Nq + qrow_i : -1;
    u32x4 qf[DC];
    {
        const uint16_t* row = static_cast<const uint16_t*>(p.q) + b * p.qs[0] + qrow_h * p.qs[1] + qrow_i * p.qs[2] + 8 * g;
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) qf[dc] = live ? *reinterpret_cast<const u32x4*>(row + dc * 32) : (u32x4){0u, 0u, 0u, 0u};
    }

    const int page_keys = mla_page_keys(p.page_size, p.capacity_keys);
    // one tile into registers as it lies in memory: chunk c = i * 256 + tid of its 32 x 72 chunks; rows at or beyond len as zero bits
    auto load_tile = [&](int t, u32x4 (&st)[NL]) {
        const MlaTile mt = mla_tile(t, len, page_keys);
        int64_t base;
        if (p.page_size) base = (int64_t)prefill_clamp_page(p.bt[b * p.bts + mt.slot], p.num_pages) * p.ks[0];
        else base = b * p.ks[0];
        const int last = mt.rows - 1;                  // >= 0: every tile of a part holds a valid key; a row index is clamped to it
        const uint16_t* const kb = static_cast<const uint16_t*>(p.k) + base;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int ch = i * (kDecodeWaves * 64) + tid, kk = ch / CH, col = ch % CH;
            const u32x4 x = *reinterpret_cast<const u32x4*>(kb + (int64_t)(mt.row + (kk < last ? kk : last)) * p.ks[2] + col * 8);
            st[i] = kk <= last ? x : (u32x4){0u, 0u, 0u, 0u};
        }
    };
    auto store_tile = [&](char* buf, const u32x4 (&st)[NL]) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int ch = i * (kDecodeWaves * 64) + tid;
            *reinterpret_cast<u32x4*>(buf + (ch / CH) * ROWB + (ch % CH) * 16) = st[i];
        }
    };

    float m = ninf, l = 0.f;
    f32x4 acc[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) acc[db] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int tend = first + nt;
    u32x4 st[NL];
    if (nt > 0) {
        load_tile(first, st);
        store_tile(mla_lds, st);
    }
    __syncthreads();
    int cur = 0;
    for (int t = first; t < tend; ++t) {
        const bool more = t + 1 < tend;
        if (more) load_tile(t + 1, st);                // in flight while this tile is computed on
        const char* const img = mla_lds + cur * BUF;
        if (wave_live) {
            // S^T = K Q^T: one 16 x 16 block per 16-key block
            f32x4 s[2];
            const char* const ka = img + qi * ROWB + g * 16;
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                s[blk] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dc = 0; dc < DC; ++dc)
                    s[blk] = decode_mfma<BF16>(*reinterpret_cast<const u32x4*>(ka + blk * 16 * ROWB + dc * 64), qf[dc], s[blk]);
            }
            // online softmax: scores scaled in f32, f32 maxima and row sums of the unrounded P, P rounded to the I/O dtype for P . V
            const int key0 = t * T;
            float x[8];
            float mt = ninf;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = key0 + 16 * (j >> 2) + 4 * g + (j & 3);
                x[j] = key <= pos ? s[j >> 2][j & 3] * p.c : ninf;
                mt = __builtin_fmaxf(mt, x[j]);
            }
            mt = decode_group_max(mt);
            const float mn = __builtin_fmaxf(m, mt), mu = mn == ninf ? 0.f : mn;
            const float alpha = __builtin_amdgcn_exp2f(m - mu);
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                x[j] = __builtin_amdgcn_exp2f(x[j] - mu);
                sum += x[j];
            }
            l = l * alpha + decode_group_sum(sum);
            m = mn;
            const u32x4 pf = {pack2<BF16>(x[0], x[1]), pack2<BF16>(x[2], x[3]), pack2<BF16>(x[4], x[5]), pack2<BF16>(x[6], x[7])};
            // O^T = alpha O^T + V^T P^T: the transposed reads deliver keys 4 g .. 4 g + 3 and the same 16 rows further down — P's k order
            const char* const tr_addr = img + (4 * g + (qi >> 2)) * ROWB + 8 * (qi & 3);      // lane 4 q + p of a group supplies row q, columns 4 p ..
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                const u32x2 lo = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(tr_addr + db * 32)));
                const u32x2 hi = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(tr_addr + db * 32 + 16 * ROWB)));
                const u32x4 vf = {lo[0], lo[1], hi[0], hi[1]};
                acc[db] = decode_mfma<BF16>(vf, pf, acc[db] * alpha);
            }
        }
        if (more) store_tile(mla_lds + (cur ^ 1) * BUF, st);
        __syncthreads();                               // tile t + 1 is visible, and tile t's buffer is free for t + 2
        cur ^= 1;
    }

    // each wave owns its rows: acc[db][e] = O^T[d = 16 db + 4 g + e][row qi], normalised once, rounded once
    if (!live) return;
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    // log2(l) with one Newton step on v_log_f32's answer y: y += (l 2^-y - 1) log2(e).  v_log_f32 is good to an ulp of its RESULT, and at a few hundred
    // keys per part that ulp is 2^-20: the parts' errors reach the merged LSE one to one
    const float l1 = l > 0.f ? l : 1.0f;
    float lg = __builtin_amdgcn_logf(l1);
    lg = __builtin_fmaf(__builtin_fmaf(l1, __builtin_amdgcn_exp2f(-lg), -1.0f), 1.4426950408889634f, lg);
    const float lse2 = l > 0.f ? m + lg : ninf;
    if (p.nsplit > 1) {
        float* dst = ws_o + (int64_t)r * kMlaDv + 4 * g;
#pragma unroll
        for (int db = 0; db < DB; ++db) *reinterpret_cast<f32x4*>(dst + db * 16) = acc[db] * inv;
        if (g == 0) ws_l[r] = lse2;
    } else {
        uint16_t* dst = static_cast<uint16_t*>(p.o) + b * p.os[0] + qrow_h * p.os[1] + qrow_i * p.os[2] + 4 * g;
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            const f32x4 a = acc[db] * inv;
            *reinterpret_cast<u32x2*>(dst + db * 16) = (u32x2){pack2<BF16>(a[0], a[1]), pack2<BF16>(a[2], a[3])};
        }
        if (g == 0) p.lse[b * p.ls[0] + qrow_h * p.ls[1] + qrow_i] = lse2;
    }
}

#endif  // __HIPCC__

}  // namespace fa2

#if defined(__HIPCC__)
#include "fa2_launch.h"              // (includes nothing of this file: the launcher's declaration needs FA2_LAUNCHER alone)
namespace fa2 {
// decode_mla_hip.cpp: the kernel above on a grid of (p.nsplit, row blocks, B) workgroups, then — p.nsplit > 1 — decode_combine_kernel at head dim 512
FA2_LAUNCHER(launch_decode_mla, (const DecodeParams& p, hipStream_t stream), (p, stream))
}  // namespace fa2
#endif
