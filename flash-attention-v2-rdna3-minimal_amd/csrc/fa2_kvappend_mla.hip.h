// fa2_kvappend_mla.hip.h — the append for a latent (MLA) KV cache (fa2_kvcache_append_mla, fa2_kvcache_append_mla_varlen; include/fa2_gfx950.h has the
// contract, DESIGN.md section 29 the reasons): the write side of fa2_fwd_decode_mla.  One launch turns the new tokens' kv_c rows (512 columns) and k_pe
// rows (64 columns) into cache rows of 576 columns at the key position only the device knows, rotating the TRAILING 64 columns by that position, and —
// when q is given — writes q with its trailing 64 columns rotated to q_out.
//
// Work is section 22's: blockIdx.x is the (sequence, token) group (the packed call: the packed token, whose sequence kvappend_varlen_token finds), so
// the length, the position, the page id and the table row are uniform over the workgroup; blockIdx.y * blockDim.x + threadIdx.x is the lane's unit among
// the group's R * 36 units, R = 1 + H rows: the latent row, then the H rows of q.  A row is 72 chunks of 16 bytes and a unit is TWO of them
// (mla_append_chunks, host and device): chunks (2u, 2u + 1) everywhere but in the rotated tail of a GPT-NeoX row, where unit 32 + c takes chunk 64 + c
// and its partner 68 + c — both members of every pair in one lane, no value crosses lanes.  Chunks 0 .. 63 of the latent row come from kv_c, chunks
// 64 .. 71 from k_pe; a unit never straddles the two (units 0 .. 31 and 32 .. 35).  What is not rotated goes from its 16-byte load to its 16-byte
// store without a conversion.
//
// Safety is fa2_kvappend.hip.h's: kvappend_slot gives the key position or "skip", a page id outside [0, num_pages) skips too (mla_append_cache_row,
// host and device), the table row is clamped into [0, seqlen_ro - 1], nothing is clamped onto a live row, every address is a 64-bit product of validated
// sizes and a value inside its range.
#pragma once
#include <stdint.h>

#include "fa2_decode_mla.hip.h"      // kMlaD, kMlaDv, kMlaMaxHeads: the cache this file writes is the one that file reads
#include "fa2_kvappend.hip.h"        // append_threads, append_unpack8, append_table, append_pack8; kvappend_slot, kvappend_varlen_token; the rotary arithmetic

namespace fa2 {

constexpr int kMlaRot = kMlaD - kMlaDv;          // 64: the rotary key, the trailing columns of a row
constexpr int kMlaChunks = kMlaD / 8;            // 72 chunks of 16 bytes per row
constexpr int kMlaUnits = kMlaChunks / 2;        // 36 units per row
constexpr int kMlaTailChunk = kMlaDv / 8;        // 64: the first chunk of the rotated tail
constexpr int kMlaTailUnit = kMlaTailChunk / 2;  // 32: the first unit of the rotated tail

struct KvAppendMlaParams {
    const void *kv_c, *k_pe;        // B x Nnew x 512 and B x Nnew x 64 (packed: total x ..), the I/O dtype
    void* kv_cache;                 // fa2_fwd_decode_mla's latent cache, the I/O dtype
    const void* q;                  // B x H x Nnew x 576 or null
    void* q_out;
    const void *cos, *sin;          // [seqlen_ro, 32], f32 or the I/O dtype (tab16); null: k_pe is copied bit for bit
    const int* lens;                // cache_seqlens [B], device: the lengths AFTER the append
    const int* bt;                  // block_table (paged) or null
    const int* cu;                  // the packed call's cu_seqlens [B + 1], device
    int B, H, Nnew;                 // (Nnew: the uniform call's)
    int interleaved, tab16;
    int page_size, num_pages;
    int R;                          // rows per group: 1 + H
    int64_t capacity_keys, seqlen_ro;
    int64_t cs[2], ps[2];           // kv_c and k_pe element strides {batch, row} (the packed call: {0, row})
    int64_t ks[3];                  // the cache's {batch | page, -, row}
    int64_t qs[3], qos[3];          // {batch, head, row} (the packed call: {0, head, row})
    int64_t bts, ros;               // block-table row stride, table row stride
};

// The two chunks of unit u (0 .. 35) of a row.  halves: the row's tail is rotated with the GPT-NeoX pairing (512 + j, 512 + 32 + j).
FA2_DEC_HD inline void mla_append_chunks(int u, bool halves, int* a, int* b) {
    if (halves && u >= kMlaTailUnit) {
        *a = kMlaTailChunk + (u - kMlaTailUnit);
        *b = *a + kMlaRot / 16;
    } else {
        *a = 2 * u;
        *b = 2 * u + 1;
    }
}

// The element offset of key slot `slot` (kvappend_slot's, >= 0) of sequence b in the latent cache, or -1: its page id lies outside [0, num_pages) and
// the token is skipped.  slot < capacity * page_size, so the block-table entry read is one of the sequence's `capacity`.
FA2_DEC_HD inline int64_t mla_append_cache_row(int64_t slot, int b, const int* bt, int64_t bts, int page_size, int num_pages, const int64_t* ks) {
    int64_t base = b, r = slot;
    if (page_size) {
        const int64_t pg = slot / page_size;
        const int pid = bt[b * bts + pg];
        if (pid < 0 || pid >= num_pages) return -1;
        base = pid;
        r = slot - pg * page_size;
    }
    return base * ks[0] + r * ks[2];
}

// One unit of one token, as both kernels and the host walk of tools/kvappend_mla_sanitize.cpp address it.  (b, i, nnew), (sb, sr) and owned are
// kvappend_row's: the sequence and the token's index among its nnew new tokens; the batch and the row of the token's source rows (the uniform call:
// (b, i); the packed call: (0, t)); owned = false (the packed call alone: a token no sequence owns): the latent row is skipped and the q row copied,
// no length or table entry is read, b being no index then.  -> false: the unit moves nothing (beyond the group's units, a skipped token).
struct MlaAppendUnit {
    const uint16_t* src;            // the row the two chunks are read from, at the column of destination column `sc`
    uint16_t* dst;                  // the destination row: 576 columns of the cache or of q_out
    int ca, cb, sc;                 // the two chunks (of the destination row); source column = 8 * chunk - sc
    bool rotate;                    // the unit holds pairs j0 .. j0 + 7 of the tail, rotated by table row offset tr
    int64_t tr;
    int j0;
};
FA2_DEC_HD inline bool mla_append_unit(const KvAppendMlaParams& p, int unit, int b, int i, int nnew, int64_t sb, int64_t sr, bool owned, MlaAppendUnit* w) {
    if (unit >= p.R * kMlaUnits) return false;
    const int row = unit / kMlaUnits, u = unit - row * kMlaUnits;
    const bool isq = row > 0;
    if (!owned && !isq) return false;

    const int64_t len = owned ? p.lens[b] : 0;
    const int64_t pos = len - nnew + i;                          // the position q row i and new key i share
    const bool tail = u >= kMlaTailUnit;
    w->rotate = p.cos != nullptr && owned && tail;
    mla_append_chunks(u, w->rotate && !p.interleaved, &w->ca, &w->cb);
    w->sc = 0;
    if (isq) {
        const int h = row - 1;
        w->src = static_cast<const uint16_t*>(p.q) + sb * p.qs[0] + h * p.qs[1] + sr * p.qs[2];
        w->dst = static_cast<uint16_t*>(p.q_out) + sb * p.qos[0] + h * p.qos[1] + sr * p.qos[2];
    } else {
        const int64_t slot = kvappend_slot(len, p.capacity_keys, nnew, i);
        if (slot < 0) return false;                              // a skipped token: nothing is written
        const int64_t ofs = mla_append_cache_row(slot, b, p.bt, p.bts, p.page_size, p.num_pages, p.ks);
        if (ofs < 0) return false;                               // a page id outside the pool: skipped, never clamped onto a live page
        w->dst = static_cast<uint16_t*>(p.kv_cache) + ofs;
        if (tail) {
            w->src = static_cast<const uint16_t*>(p.k_pe) + sb * p.ps[0] + sr * p.ps[1];
            w->sc = kMlaDv;
        } else {
            w->src = static_cast<const uint16_t*>(p.kv_c) + sb * p.cs[0] + sr * p.cs[1];
        }
    }
    // unit 32 + k holds pairs 8k .. 8k + 7 under either pairing: one table read, then (xa[e], xb[e]) or the neighbours inside xa and inside xb
    w->tr = w->rotate ? rotary_table_row(pos, p.seqlen_ro) * p.ros : 0;
    w->j0 = 8 * (u - kMlaTailUnit);
    return true;
}

#if defined(__HIPCC__)

template <bool BF16>
__device__ __forceinline__ void kvappend_mla_row(const KvAppendMlaParams& p, int b, int i, int nnew, int64_t sb, int64_t sr, bool owned) {
    MlaAppendUnit w;
    if (!mla_append_unit(p, blockIdx.y * blockDim.x + threadIdx.x, b, i, nnew, sb, sr, owned, &w)) return;
    const u32x4 wa = *reinterpret_cast<const u32x4*>(w.src + (8 * w.ca - w.sc));
    const u32x4 wb = *reinterpret_cast<const u32x4*>(w.src + (8 * w.cb - w.sc));
    if (!w.rotate) {                                             // bit for bit
        *reinterpret_cast<u32x4*>(w.dst + 8 * w.ca) = wa;
        *reinterpret_cast<u32x4*>(w.dst + 8 * w.cb) = wb;
        return;
    }

    float xa[8], xb[8], c[8], s[8];
    append_table<BF16, 8>(p.cos, w.tr, w.j0, p.tab16 != 0, c);
    append_table<BF16, 8>(p.sin, w.tr, w.j0, p.tab16 != 0, s);
    append_unpack8<BF16>(wa, xa);
    append_unpack8<BF16>(wb, xb);
    if (!p.interleaved) {
#pragma unroll
        for (int e = 0; e < 8; ++e) rotary_pair(xa[e], xb[e], c[e], s[e], &xa[e], &xb[e]);
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            rotary_pair(xa[2 * m], xa[2 * m + 1], c[m], s[m], &xa[2 * m], &xa[2 * m + 1]);
            rotary_pair(xb[2 * m], xb[2 * m + 1], c[4 + m], s[4 + m], &xb[2 * m], &xb[2 * m + 1]);
        }
    }
    *reinterpret_cast<u32x4*>(w.dst + 8 * w.ca) = append_pack8<BF16>(xa);
    *reinterpret_cast<u32x4*>(w.dst + 8 * w.cb) = append_pack8<BF16>(xb);
}

// the uniform call: blockIdx.x is the (sequence, token) group of Nnew tokens per sequence
template <bool BF16>
__global__ __launch_bounds__(kAppendThreads) void kvappend_mla_kernel(const KvAppendMlaParams p) {
    const int tok = blockIdx.x;
    const int b = tok / p.Nnew, i = tok - b * p.Nnew;
    kvappend_mla_row<BF16>(p, b, i, p.Nnew, b, i, true);
}

// the packed call: blockIdx.x is the packed token t; kvappend_varlen_token finds the sequence that owns it in cu_seqlens — device data nobody
// validated — or none
template <bool BF16>
__global__ __launch_bounds__(kAppendThreads) void kvappend_mla_varlen_kernel(const KvAppendMlaParams p) {
    const int t = blockIdx.x;
    int s, i, nnew;
    const bool owned = kvappend_varlen_token(p.cu, p.B, t, &s, &i, &nnew);
    kvappend_mla_row<BF16>(p, owned ? s : 0, owned ? i : 0, owned ? nnew : 1, 0, t, owned);
}

#endif  // __HIPCC__

}  // namespace fa2

#if defined(__HIPCC__)
#include "fa2_launch.h"              // FA2_LAUNCHER
namespace fa2 {
// kvappend_mla_hip.cpp: grid x = groups (B * Nnew, or the packed call's total), y = slices of the group's R * 36 units; packed: the varlen kernel
FA2_LAUNCHER(launch_kvappend_mla, (const KvAppendMlaParams& p, int64_t groups, bool packed, hipStream_t stream), (p, groups, packed, stream))
}  // namespace fa2
#endif
