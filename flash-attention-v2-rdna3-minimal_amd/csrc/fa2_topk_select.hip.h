// fa2_topk_select.hip.h — deterministic top-k selection over the indexer's logits (fa2_topk_indices; include/fa2_gfx950.h has the contract, DESIGN.md
// section 34 the reasons): it emits exactly the `indices` tensor fa2_fwd_decode_mla_sparse consumes.  Per row (b, i), over s in [0, pos] only
// (pos = len_b - Nq + i): the min(topk, pos + 1) positions of the largest logits IN ASCENDING POSITION ORDER, then -1.  Among equal logits the lowest
// positions win; a NaN ranks as -inf; -0 equals +0.
//
// One workgroup of 16 waves per row; a radix select on the order-preserving 32-bit image of the float (topk_key):
//
//   threshold    four passes over [0, pos], one 8-bit digit each from the top: an LDS histogram of the digit among the keys that share the digits
//                found so far, then a scan from the highest digit down finds the digit of the topk-th largest key and how many keys are still
//                wanted below it.  After the fourth pass the threshold key T is known exactly, and with it `take`: how many keys equal to T belong
//                to the list.  A bin has eight copies on eight LDS banks (a lane adds to copy lane % 8): real logits share their exponent, so the first
//                digit of most keys is the same one, and same-address LDS atomics of a wave run one after the other.
//   compaction   one ordered pass in blocks of 1 024 positions: two ballots and a lane-mask population count place a key among its wave's, the waves'
//                totals cross LDS (one barrier per block, two buffers), and two running counts — keys above T, keys equal to T — place the block.
//                A key above T lands at (keys above T before it) + min(keys equal to T before it, take); a key equal to T is kept while fewer than
//                `take` came before it.  Positions therefore come out ascending, ties go to the lowest positions, and exactly topk entries are
//                written; the pass stops when the list is full.
//
// pos + 1 <= topk writes 0 .. pos and the -1 tail without reading a logit.  Only [0, pos] of a row is ever read.  No global atomics; the LDS atomics are
// integer counts: the result is a pure function of the row, bit for bit from run to run.
#pragma once
#include <stdint.h>

#include "fa2_decode.hip.h"          // decode_clamp_len, FA2_DEC_HD

namespace fa2 {

constexpr int kTopkWaves = 16;
constexpr int kTopkThreads = kTopkWaves * 64;
constexpr int kTopkCopies = 8;              // copies of a histogram bin, on consecutive LDS banks

struct TopkParams {
    const float* logits;        // [B, Nq, capacity_keys] f32, device; the key dim contiguous
    int* idx;                   // indices [B, Nq, topk] int32, device; the last dim contiguous
    const int* lens;            // cache_seqlens [B], device
    int B, Nq, topk;
    int64_t capacity_keys;
    int64_t ls[2], is[2];       // element strides {batch, row}
    const int* cu;              // the packed geometry alone: cu_seqlens_q [B + 1], device; the row is packed token t and Nq counts all of them
};

// The order-preserving image of a float32's bits: a < b as floats <=> topk_key(a) < topk_key(b), with every NaN at -inf's place and -0 at +0's.
FA2_DEC_HD inline uint32_t topk_key(uint32_t bits) {
    if ((bits & 0x7fffffffu) > 0x7f800000u) bits = 0xff800000u;
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

#if defined(__HIPCC__)

// (a template so that the header can be included by more than one unit: topk_select_hip.cpp alone instantiates it)
// PACKED (fa2_topk_indices_varlen): the row is packed token t of [total_q, capacity]; kvappend_varlen_token names its sequence s,
// i = t - cu[s] and Nq_s, pos = clamp_len(len_s) - Nq_s + i, and a row no sequence owns is all -1 (as is one at a negative position, by n <= 0).
template <int THREADS, bool PACKED = false>
__global__ __launch_bounds__(THREADS) void topk_select_kernel(const TopkParams p) {
    static_assert(THREADS == kTopkThreads, "one workgroup shape");
    __shared__ uint32_t hist[256 * kTopkCopies];
    __shared__ uint32_t wsum[2][kTopkWaves];
    __shared__ uint32_t found[2];
    int b, i, pos;
    if constexpr (PACKED) {
        int s, si, nq;
        const bool owned = kvappend_varlen_token(p.cu, p.B, blockIdx.x, &s, &si, &nq);
        pos = owned ? decode_clamp_len(p.lens[s], p.capacity_keys) - nq + si : -1;
        b = 0;                                                            // (the row strides alone address a packed row)
        i = blockIdx.x;
    } else {
        const int row = blockIdx.x;
        b = row / p.Nq;
        i = row - b * p.Nq;
        pos = decode_clamp_len(p.lens[b], p.capacity_keys) - p.Nq + i;
    }
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = pos + 1, topk = p.topk;
    int* const out = p.idx + b * p.is[0] + i * p.is[1];
    if (n <= topk) {                                                      // every position is selected (n <= 0: none): no logit is read
        for (int t = tid; t < topk; t += kTopkThreads) out[t] = t < n ? t : -1;
        return;
    }
    const uint32_t* const x = reinterpret_cast<const uint32_t*>(p.logits + b * p.ls[0] + i * p.ls[1]);

    // ---- the threshold key T: its four digits from the top; `need` = the keys still wanted among those that share the digits found so far
    uint32_t T = 0, need = (uint32_t)topk;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const uint32_t hi = (uint32_t)~((1ull << (shift + 8)) - 1);      // the digits found so far (pass 0: none)
        for (int t = tid; t < 256 * kTopkCopies; t += kTopkThreads) hist[t] = 0;
        __syncthreads();
        for (int s = tid; s < n; s += kTopkThreads) {
            const uint32_t key = topk_key(x[s]);
            if ((key & hi) == T) atomicAdd(&hist[((key >> shift) & 255) * kTopkCopies + (lane & (kTopkCopies - 1))], 1u);
        }
        __syncthreads();
        // thread t < 256 owns digit 255 - t: an inclusive scan over the first four waves counts the keys at or above its digit
        uint32_t v = 0;
        if (tid < 256)
            for (int c = 0; c < kTopkCopies; ++c) v += hist[(255 - tid) * kTopkCopies + c];
        uint32_t inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (tid < 256 && lane == 63) wsum[0][w] = inc;
        __syncthreads();
        if (tid < 256) {
            for (int ww = 0; ww < w; ++ww) inc += wsum[0][ww];
            if (inc >= need && inc - v < need) {                          // exactly one digit: the counts of this pass sum to at least `need`
                found[0] = (uint32_t)(255 - tid);
                found[1] = need - (inc - v);
            }
        }
        __syncthreads();
        T |= found[0] << shift;
        need = found[1];
    }
    const uint32_t take = need;                                           // keys equal to T that belong to the list (>= 1)

    // ---- the ordered compaction
    uint32_t run_gt = 0, run_eq = 0;
    for (int s0 = 0, it = 0; s0 < n; s0 += kTopkThreads, ++it) {
        const int s = s0 + tid;
        const uint32_t key = s < n ? topk_key(x[s]) : 0u;                 // (0 is below every image: T >= the image of -inf)
        const bool gt = key > T, eq = key == T;
        const uint64_t mgt = __builtin_amdgcn_ballot_w64(gt), meq = __builtin_amdgcn_ballot_w64(eq), below = (1ull << lane) - 1;
        if (lane == 0) wsum[it & 1][w] = (uint32_t)__builtin_popcountll(mgt) | ((uint32_t)__builtin_popcountll(meq) << 16);
        __syncthreads();
        uint32_t before_gt = run_gt + (uint32_t)__builtin_popcountll(mgt & below), before_eq = run_eq + (uint32_t)__builtin_popcountll(meq & below);
        for (int ww = 0; ww < kTopkWaves; ++ww) {
            const uint32_t c = wsum[it & 1][ww];
            if (ww < w) { before_gt += c & 0xffffu; before_eq += c >> 16; }
            run_gt += c & 0xffffu;
            run_eq += c >> 16;
        }
        // (count of keys above T + take == topk, so a slot is below topk by construction; the comparison keeps a store inside the row regardless)
        const uint32_t slot = before_gt + (before_eq < take ? before_eq : take);
        if ((gt || (eq && before_eq < take)) && slot < (uint32_t)topk) out[slot] = s;
        if (run_gt + (run_eq < take ? run_eq : take) >= (uint32_t)topk) break;      // the list is full (workgroup-uniform)
    }
}

#endif  // __HIPCC__

}  // namespace fa2

#if defined(__HIPCC__)
#include "fa2_launch.h"
namespace fa2 {
// topk_select_hip.cpp: the kernel above, one workgroup per row (b, i)
FA2_HIDDEN int launch_topk_select(const TopkParams& p, hipStream_t stream);
// ... and its packed form, one workgroup per packed token (p.Nq = total_q, p.cu set)
FA2_HIDDEN int launch_topk_select_varlen(const TopkParams& p, hipStream_t stream);
}  // namespace fa2
#endif
