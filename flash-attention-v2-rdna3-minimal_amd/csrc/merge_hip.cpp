// merge_hip.cpp — merge of partial attention results (fa2_merge_fwd / fa2_merge_bwd; include/fa2_gfx950.h has the contract): attention computed over
// disjoint pieces of the KV axis leaves (O_k, lse_k) pairs, and
//     m = max_k lse_k,  w_k = 2^(lse_k - m) / sum_k 2^(lse_k - m),  O = sum_k w_k O_k,  lse = m + log2 sum_k 2^(lse_k - m)
// is the result over the union.  Memory-bound work, no matrix pipe and no LDS: a row of D elements is served by D / 8 lanes with one 16-byte load per
// lane and part (a group of the next power of two lanes, so that the backward's row sums are xor butterflies inside a wave), rows are spread over the
// wave and the grid, the parts' pointers travel by value in the kernel's argument block (no device copy: the call can be captured in a graph), every
// output element has one owner (no atomics).  The forward reads every part's bytes once; the backward reads the parts and dO once and re-reads nothing
// (dO.O is formed as sum_k w_k (dO.O_k)).  A part of weight exactly 0 — lse_k = -inf, or 2^(lse_k - m) underflowed — is never read: its O_k may hold
// anything.  One translation unit serves both dtypes.
#include "fa2_launch.h"

#include "fa2_gfx950.h"

namespace fa2 {
namespace {

constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;
constexpr int kMergeThreads = 256;

template <bool BF16>
__device__ __forceinline__ void unpack8(u32x4 a, float (&x)[8]) {
    if constexpr (BF16) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            x[2 * w] = __uint_as_float(a[w] << 16);
            x[2 * w + 1] = __uint_as_float(a[w] & 0xffff0000u);
        }
    } else {
        const f16x8 h = __builtin_bit_cast(f16x8, a);      // (whole-vector bit_cast: fa2_bwd_kernel.hip.h, dot8)
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = (float)h[e];
    }
}

template <bool BF16>
__device__ __forceinline__ u32x4 pack8(const float (&x)[8]) {
    return (u32x4){pack2<BF16>(x[0], x[1]), pack2<BF16>(x[2], x[3]), pack2<BF16>(x[4], x[5]), pack2<BF16>(x[6], x[7])};
}

// the lane's row and 8-column granule: groups of `group` lanes (a power of two <= 64) own one row each, the first `lanes` of them a granule
struct MergeLane { int64_t b, h, n; int col; bool active, first; };
__device__ __forceinline__ MergeLane merge_lane(const MergeParams& p) {
    const int g = threadIdx.x & (p.group - 1);
    const int64_t row = (int64_t)blockIdx.x * (kMergeThreads / p.group) + threadIdx.x / p.group;
    MergeLane l;
    l.active = row < p.rows && g < p.lanes;
    l.first = row < p.rows && g == 0;
    const int64_t r = row < p.rows ? row : 0;
    l.b = r / ((int64_t)p.H * p.Nq);
    l.h = (r / p.Nq) % p.H;
    l.n = r % p.Nq;
    l.col = 8 * g;
    return l;
}

template <bool BF16>
__global__ __launch_bounds__(kMergeThreads) void merge_fwd_kernel(const MergeParams p) {
    const MergeLane l = merge_lane(p);
    if (!l.active) return;
    // (the LSEs stay in their own unit until a DIFFERENCE is formed: lse_k - m is exact or nearly so, lse_k * log2(e) - m * log2(e) carries two roundings at
    //  the LSEs' magnitude — with one part the merged LSE must be that part's, bit for bit, and the backward's weight exactly 1)
    const float in_unit = p.natural ? kLog2e : 1.0f, out_unit = p.natural ? kLn2 : 1.0f;
    const int64_t lo = l.b * p.pls[0] + l.h * p.pls[1] + l.n, po = l.b * p.ps[0] + l.h * p.ps[1] + l.n * p.ps[2] + l.col;
    float ls[kMergeMaxParts];
    float m = -__builtin_inff();
#pragma unroll
    for (int k = 0; k < kMergeMaxParts; ++k) {
        ls[k] = k < p.nparts ? p.lse_parts[k][lo] : -__builtin_inff();
        m = __builtin_fmaxf(m, ls[k]);
    }
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float sum = 0.f;
    if (m != -__builtin_inff()) {
#pragma unroll
        for (int k = 0; k < kMergeMaxParts; ++k) {
            const float w = __builtin_amdgcn_exp2f((ls[k] - m) * in_unit);
            if (k < p.nparts && w != 0.f) {
                float x[8];
                unpack8<BF16>(*(const u32x4*)((const uint16_t*)p.o_parts[k] + po), x);
                sum += w;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(w, x[e], acc[e]);
            }
        }
        const float inv = 1.0f / sum;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] *= inv;
    }
    *(u32x4*)((uint16_t*)p.o + l.b * p.os[0] + l.h * p.os[1] + l.n * p.os[2] + l.col) = pack8<BF16>(acc);
    if (l.first) p.lse[l.b * p.ls[0] + l.h * p.ls[1] + l.n] = m != -__builtin_inff() ? __builtin_fmaf(__builtin_amdgcn_logf(sum), out_unit, m) : m;
}

// dO_k = w_k dO;  dlse_k = w_k (dlse + dO.(O_k - O)) with dO.O = sum_k w_k (dO.O_k) — in the LSEs' own unit: the dot term carries ln 2 when they are log2
template <bool BF16>
__global__ __launch_bounds__(kMergeThreads) void merge_bwd_kernel(const MergeParams p) {
    const MergeLane l = merge_lane(p);
    // (no early return: the lanes of a group that own no granule — head dims whose D / 8 is no power of two — still take part in the butterflies below)
    const float in_unit = p.natural ? kLog2e : 1.0f, dot_unit = p.natural ? 1.0f : kLn2;
    const int64_t lo = l.b * p.pls[0] + l.h * p.pls[1] + l.n, po = l.b * p.ps[0] + l.h * p.ps[1] + l.n * p.ps[2] + l.col;
    const int64_t dlo = l.b * p.dpls[0] + l.h * p.dpls[1] + l.n, dpo = l.b * p.dps[0] + l.h * p.dps[1] + l.n * p.dps[2] + l.col;
    const float lse = l.first || l.active ? p.lse[l.b * p.ls[0] + l.h * p.ls[1] + l.n] : -__builtin_inff();      // (its own unit: merge_fwd_kernel)
    const bool live = lse != -__builtin_inff();
    float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (l.active) unpack8<BF16>(*(const u32x4*)((const uint16_t*)p.dout + l.b * p.dos[0] + l.h * p.dos[1] + l.n * p.dos[2] + l.col), g);
    float w[kMergeMaxParts], d[kMergeMaxParts];
#pragma unroll
    for (int k = 0; k < kMergeMaxParts; ++k) {
        w[k] = 0.f;
        d[k] = 0.f;
        if (k < p.nparts) {
            if (live && (l.active || l.first)) w[k] = __builtin_amdgcn_exp2f((p.lse_parts[k][lo] - lse) * in_unit);
            if (l.active) {
                float y[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (w[k] != 0.f) {
                    float x[8];
                    unpack8<BF16>(*(const u32x4*)((const uint16_t*)p.o_parts[k] + po), x);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        d[k] = __builtin_fmaf(g[e], x[e], d[k]);
                        y[e] = w[k] * g[e];
                    }
                }
                *(u32x4*)((uint16_t*)p.do_parts[k] + dpo) = pack8<BF16>(y);
            }
        }
    }
    // row sums of dO.O_k over the group's lanes (xor butterflies: a group never straddles a wave), then dO.O
    float dot_o = 0.f;
#pragma unroll
    for (int k = 0; k < kMergeMaxParts; ++k) {
        if (k < p.nparts) {
            for (int s = p.group >> 1; s > 0; s >>= 1) d[k] += __shfl_xor(d[k], s, 64);
            dot_o = __builtin_fmaf(w[k], d[k], dot_o);
        }
    }
    if (!l.first) return;
    const float gl = p.dlse != nullptr && live ? p.dlse[l.b * p.dls[0] + l.h * p.dls[1] + l.n] : 0.f;
#pragma unroll
    for (int k = 0; k < kMergeMaxParts; ++k)
        if (k < p.nparts) p.dlse_parts[k][dlo] = w[k] != 0.f ? w[k] * (gl + dot_unit * (d[k] - dot_o)) : 0.f;
}

template <auto Kernel>
int launch_merge(MergeParams& p, hipStream_t stream) {
    p.lanes = p.D / 8;
    p.group = 1;
    while (p.group < p.lanes) p.group <<= 1;
    p.rows = (int64_t)p.B * p.H * p.Nq;
    const int64_t per_block = kMergeThreads / p.group, blocks = (p.rows + per_block - 1) / per_block;
    if (blocks > 0x7fffffffLL) return FA2_ERR_GRID;
    return launch<Kernel>(dim3((unsigned)blocks), dim3(kMergeThreads), 0, stream, p);
}

}  // namespace

int launch_merge_fwd(bool bf16, MergeParams& p, hipStream_t stream) {
    return bf16 ? launch_merge<merge_fwd_kernel<true>>(p, stream) : launch_merge<merge_fwd_kernel<false>>(p, stream);
}
int launch_merge_bwd(bool bf16, MergeParams& p, hipStream_t stream) {
    return bf16 ? launch_merge<merge_bwd_kernel<true>>(p, stream) : launch_merge<merge_bwd_kernel<false>>(p, stream);
}

}  // namespace fa2
