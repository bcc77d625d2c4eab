// fa2_kvappend.hip.h — KV-cache append with rotary embedding and e4m3 quantisation (fa2_kvcache_append; include/fa2_gfx950.h has the contract, DESIGN.md
// section 22 the reasons): the write side of the decode path.  One launch moves the new tokens' K rows and V rows into the cache — contiguous or paged,
// 16-bit or e4m3 — at the key position only the device knows, and, when q is given, writes the rotated q rows to q_out.
//
// Work is (sequence, token) groups of R = 2 Hkv (+ H) rows: blockIdx.x is the group, so the length, the position, the page id and the table row are
// uniform over the workgroup (scalar loads: read once per group, not per lane); blockIdx.y * blockDim.x + threadIdx.x is the lane's unit inside the
// group (64, 128 or 256 lanes per workgroup: the smallest that holds the group's units, so that a K / V-only append of few heads idles no wave).
// A unit is TWO 16-byte chunks of one row (8 columns of the 16-bit source each): chunks (2u, 2u + 1) — 16 consecutive columns, one 16-byte store into
// an e4m3 cache — except in the rotated span of a non-interleaved (GPT-NeoX) row, where unit u < rotary_dim / 16 takes chunk u and its partner chunk
// u + rotary_dim / 16: both halves of every pair are in one lane, and no value crosses lanes.  (rotary_dim is a multiple of 16, so the rotated span is
// an even number of chunks and the units behind it are again the pairs (2u, 2u + 1).)
//
// The packed (ragged) form, fa2_kvcache_append_varlen: k_new / v_new / q are [total, heads, D], blockIdx.x is the packed token t, and
// kvappend_varlen_token (fa2_decode.hip.h, host and device) finds the sequence s that owns it in cu_seqlens [B + 1] — a binary search of a fixed trip
// count whose probes stay inside cu[1 .. B] whatever the array holds, then the explicit check cu[s] <= t < cu[s + 1].  From there on the row is the uniform
// call's (kvappend_row, the one body of both kernels) with Nnew = cu[s + 1] - cu[s].  A token no sequence owns writes no K / V; its q row is copied.
//
// Safety (the lengths, the block table and cu_seqlens are device data nobody validated): kvappend_slot (fa2_decode.hip.h, host and device) gives the key position
// or "skip"; a page id outside [0, num_pages) skips too; the table row is clamped into [0, seqlen_ro - 1].  Nothing is clamped onto a valid cache row.
// Every address is a 64-bit product of validated sizes and a value inside its range, so no device value can move a write outside the two caches.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include "fa2_fwd_kernel.hip.h"      // the vector types, pack2
#endif
#include "fa2_decode.hip.h"          // kvappend_slot
#include "fa2_rotary.h"

namespace fa2 {

constexpr int kAppendThreads = 256;      // the largest workgroup; a group of fewer units runs 64 or 128 lanes (append_threads)
inline int append_threads(int units) { return units <= 64 ? 64 : units <= 128 ? 128 : kAppendThreads; }

struct KvAppendParams {
    const void *k_new, *v_new;      // B x Hkv x Nnew x D, the I/O dtype
    void *k_cache, *v_cache;        // decode's layouts; the I/O dtype or e4m3 bytes
    const void* q;                  // B x H x Nnew x D or null
    void* q_out;
    const void *cos, *sin;          // [seqlen_ro, rot / 2], f32 or the I/O dtype (tab16); null: no rotary
    const int* lens;                // cache_seqlens [B], device: the lengths AFTER the append
    const int* bt;                  // block_table (paged) or null
    const float *kd, *vd;           // e4m3 caches: descales [B, Hkv], device, null = 1.0
    int B, Hkv, H, Nnew, D;
    int rot, interleaved, tab16;
    int page_size, num_pages;
    int R, UR;                      // rows per (sequence, token) group; units per row = ceil(D / 16)
    int64_t capacity_keys, seqlen_ro;
    int64_t kns[3], vns[3], ks[3], vs[3], qs[3], qos[3];      // element strides {batch | page, head, row}
    int64_t bts, ros, ds[2];        // block-table row stride, table row stride, descale strides {batch, K / V head}
};

// the packed call's: the shared description (B: sequences; Nnew unused; the source strides' [0] unused) and the row offsets
struct KvAppendVarlenParams : KvAppendParams {
    const int* cu;                  // cu_seqlens [B + 1], device: sequence s owns the packed rows [cu[s], cu[s + 1])
};

#if defined(__HIPCC__)

// one 32-bit word of two I/O dtype values -> f32
template <bool BF16>
__device__ __forceinline__ void append_unpack2(uint32_t w, float* lo, float* hi) {
    if constexpr (BF16) {
        *lo = __builtin_bit_cast(float, w << 16);
        *hi = __builtin_bit_cast(float, w & 0xffff0000u);
    } else {
        const f16x2 h = __builtin_bit_cast(f16x2, w);
        *lo = (float)h[0];
        *hi = (float)h[1];
    }
}
template <bool BF16>
__device__ __forceinline__ void append_unpack8(u32x4 w, float (&x)[8]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) append_unpack2<BF16>(w[k], &x[2 * k], &x[2 * k + 1]);
}

// N (4 or 8) entries of a table row from entry j0 (a multiple of N) on: f32 or the I/O dtype
template <bool BF16, int N>
__device__ __forceinline__ void append_table(const void* tab, int64_t row_ofs, int j0, bool tab16, float (&c)[8]) {
    if (tab16) {
        const uint16_t* r = static_cast<const uint16_t*>(tab) + row_ofs + j0;
        if constexpr (N == 8) {
            append_unpack8<BF16>(*reinterpret_cast<const u32x4*>(r), c);
        } else {
            const u32x2 w = *reinterpret_cast<const u32x2*>(r);
            append_unpack2<BF16>(w[0], &c[0], &c[1]);
            append_unpack2<BF16>(w[1], &c[2], &c[3]);
        }
    } else {
        const float* r = static_cast<const float*>(tab) + row_ofs + j0;
#pragma unroll
        for (int k = 0; k < N / 4; ++k) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(r + 4 * k);
            c[4 * k] = v[0]; c[4 * k + 1] = v[1]; c[4 * k + 2] = v[2]; c[4 * k + 3] = v[3];
        }
    }
}

// eight f32 values -> eight e4m3 bytes: code = rne_e4m3(clamp(y / descale, +-448)).  The division is the correctly rounded one; the clamp is two
// selects that a NaN falls through (this unit is compiled with NaNs honoured), so the convert never sees a value beyond the format's range and its
// overflow mode does not matter; a NaN converts to a NaN code.
__device__ __forceinline__ u32x2 append_quant8(const float (&y)[8], float d) {
    float t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float v = y[k] / d;
        v = v > 448.0f ? 448.0f : v;
        v = v < -448.0f ? -448.0f : v;
        t[k] = v;
    }
    int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], 0, false);
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], w0, true);
    int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(t[4], t[5], 0, false);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(t[6], t[7], w1, true);
    return (u32x2){(uint32_t)w0, (uint32_t)w1};
}

template <bool BF16>
__device__ __forceinline__ u32x4 append_pack8(const float (&y)[8]) {
    return (u32x4){pack2<BF16>(y[0], y[1]), pack2<BF16>(y[2], y[3]), pack2<BF16>(y[4], y[5]), pack2<BF16>(y[6], y[7])};
}

// One row unit of one token: what both kernels run.  (b, i, nnew): the sequence, the token's index among the sequence's nnew new tokens; (sb, sr): the
// batch and the row of the token's source rows in k_new / v_new / q / q_out (the uniform call: (b, i); the packed call: (0, t)).  owned = false (the
// packed call alone: a token that belongs to no sequence): K and V rows are skipped and the q row is copied to q_out bit for bit; no length, table
// entry or descale is read, b being no index then.
// FP8: the caches hold OCP e4m3 bytes; k_new, v_new, q, q_out stay in the I/O dtype.
template <bool BF16, bool FP8>
__device__ __forceinline__ void kvappend_row(const KvAppendParams& p, int b, int i, int nnew, int64_t sb, int64_t sr, bool owned) {
    const int unit = blockIdx.y * blockDim.x + threadIdx.x;
    if (unit >= p.R * p.UR) return;
    const int row = unit / p.UR, u = unit - row * p.UR;
    const bool isq = row >= 2 * p.Hkv, isv = !isq && row >= p.Hkv;
    const int h = isq ? row - 2 * p.Hkv : isv ? row - p.Hkv : row;
    if (!owned && !isq) return;

    const int64_t len = owned ? p.lens[b] : 0;
    const int64_t pos = len - nnew + i;                          // the position q row i and new key i share
    const int64_t slot = kvappend_slot(len, p.capacity_keys, nnew, i);
    if (!isq && slot < 0) return;                                // a skipped token: nothing is written

    // the row's source and destination
    const uint16_t* src;
    char* dst;
    if (isq) {
        src = static_cast<const uint16_t*>(p.q) + sb * p.qs[0] + h * p.qs[1] + sr * p.qs[2];
        dst = reinterpret_cast<char*>(static_cast<uint16_t*>(p.q_out) + sb * p.qos[0] + h * p.qos[1] + sr * p.qos[2]);
    } else {
        const int64_t* ns = isv ? p.vns : p.kns;
        const int64_t* cs = isv ? p.vs : p.ks;
        src = static_cast<const uint16_t*>(isv ? p.v_new : p.k_new) + sb * ns[0] + h * ns[1] + sr * ns[2];
        int64_t base = b, r = slot;
        if (p.page_size) {
            const int64_t pg = slot / p.page_size;               // < the block-table entries per sequence: slot < capacity * page_size
            const int pid = p.bt[b * p.bts + pg];
            if (pid < 0 || pid >= p.num_pages) return;           // a page id outside the pool: skipped, never clamped onto a live page
            base = pid;
            r = slot - pg * p.page_size;
        }
        dst = static_cast<char*>(isv ? p.v_cache : p.k_cache) + (base * cs[0] + h * cs[1] + r * cs[2]) * (FP8 ? 1 : 2);
    }

    const int CH = p.D >> 3, rh = p.rot >> 4;
    const bool rotate = p.cos != nullptr && !isv && owned;
    const bool halves = rotate && !p.interleaved && u < rh;     // chunk u and its partner chunk u + rh
    const int ca = halves ? u : 2 * u, cb = halves ? u + rh : 2 * u + 1;
    const bool hasb = cb < CH;
    const u32x4 wa = *reinterpret_cast<const u32x4*>(src + 8 * ca);
    const u32x4 wb = hasb ? *reinterpret_cast<const u32x4*>(src + 8 * cb) : (u32x4){0u, 0u, 0u, 0u};
    const bool to8 = FP8 && !isq;

    float xa[8], xb[8];
    bool rota = false, rotb = false;
    if (rotate || to8) {
        append_unpack8<BF16>(wa, xa);
        append_unpack8<BF16>(wb, xb);
    }
    if (rotate) {
        const int64_t tr = rotary_table_row(pos, p.seqlen_ro) * p.ros;
        float c[8], s[8];
        if (halves) {
            append_table<BF16, 8>(p.cos, tr, 8 * u, p.tab16 != 0, c);
            append_table<BF16, 8>(p.sin, tr, 8 * u, p.tab16 != 0, s);
#pragma unroll
            for (int e = 0; e < 8; ++e) rotary_pair(xa[e], xb[e], c[e], s[e], &xa[e], &xb[e]);
            rota = rotb = true;
        } else if (p.interleaved) {
            if (8 * ca < p.rot) {
                append_table<BF16, 4>(p.cos, tr, 4 * ca, p.tab16 != 0, c);
                append_table<BF16, 4>(p.sin, tr, 4 * ca, p.tab16 != 0, s);
#pragma unroll
                for (int m = 0; m < 4; ++m) rotary_pair(xa[2 * m], xa[2 * m + 1], c[m], s[m], &xa[2 * m], &xa[2 * m + 1]);
                rota = true;
            }
            if (hasb && 8 * cb < p.rot) {
                append_table<BF16, 4>(p.cos, tr, 4 * cb, p.tab16 != 0, c);
                append_table<BF16, 4>(p.sin, tr, 4 * cb, p.tab16 != 0, s);
#pragma unroll
                for (int m = 0; m < 4; ++m) rotary_pair(xb[2 * m], xb[2 * m + 1], c[m], s[m], &xb[2 * m], &xb[2 * m + 1]);
                rotb = true;
            }
        }
    }

    if (to8) {
        const float* dp = isv ? p.vd : p.kd;
        const float d = dp ? dp[b * p.ds[0] + h * p.ds[1]] : 1.0f;
        const u32x2 qa = append_quant8(xa, d);
        if (hasb) {
            const u32x2 qb = append_quant8(xb, d);
            if (!halves) {                                       // 16 consecutive columns: one 16-byte store
                *reinterpret_cast<u32x4*>(dst + 8 * ca) = (u32x4){qa[0], qa[1], qb[0], qb[1]};
            } else {
                *reinterpret_cast<u32x2*>(dst + 8 * ca) = qa;
                *reinterpret_cast<u32x2*>(dst + 8 * cb) = qb;
            }
        } else {
            *reinterpret_cast<u32x2*>(dst + 8 * ca) = qa;
        }
    } else {                                                     // a 16-bit row: what was not rotated lands bit for bit
        *reinterpret_cast<u32x4*>(dst + 16 * ca) = rota ? append_pack8<BF16>(xa) : wa;
        if (hasb) *reinterpret_cast<u32x4*>(dst + 16 * cb) = rotb ? append_pack8<BF16>(xb) : wb;
    }
}

// the uniform call: blockIdx.x is the (sequence, token) group of Nnew tokens per sequence
template <bool BF16, bool FP8>
__global__ __launch_bounds__(kAppendThreads) void kvappend_kernel(const KvAppendParams p) {
    const int tok = blockIdx.x;                                  // uniform: the (sequence, token) group
    const int b = tok / p.Nnew, i = tok - b * p.Nnew;
    kvappend_row<BF16, FP8>(p, b, i, p.Nnew, b, i, true);
}

// the packed call (fa2_kvcache_append_varlen): blockIdx.x is the packed token t; kvappend_varlen_token (fa2_decode.hip.h, host and device) finds the
// sequence that owns it in cu_seqlens — device data nobody validated — or none.  Everything it reads is uniform over the workgroup.
template <bool BF16, bool FP8>
__global__ __launch_bounds__(kAppendThreads) void kvappend_varlen_kernel(const KvAppendVarlenParams p) {
    const int t = blockIdx.x;
    int s, i, nnew;
    const bool owned = kvappend_varlen_token(p.cu, p.B, t, &s, &i, &nnew);
    kvappend_row<BF16, FP8>(p, owned ? s : 0, owned ? i : 0, owned ? nnew : 1, 0, t, owned);
}

#endif  // __HIPCC__

}  // namespace fa2
