// fa2_prefill_mla_sparse.hip.h — sparse (top-k indexed) attention for PACKED query tokens on a latent (MLA) KV cache (fa2_fwd_prefill_mla_sparse;
// include/fa2_gfx950.h has the contract, DESIGN.md section 37 the reasons): the prefill step of DeepSeek-V3.2 style models, and the consumer of the
// int32 [total_q, topk] lists fa2_topk_indices_varlen writes.  Packed token t belongs to the sequence s that kvappend_varlen_token names
// (i = t - cu[s], Nq_s = cu[s + 1] - cu[s]); with pos = clamp_len(len_s) - Nq_s + i:
//
//   o[t, h] = sum over the VALID entries e of softmax_e(scale * q[t, h, :] . kv[s, j_e, :]) . kv[s, j_e, :512],  j_e = indices[t, e], 0 <= j_e <= pos
//
// The per-tile arithmetic is decode_mla_sparse_kernel's, statement for statement (csrc/fa2_decode_mla_sparse_sweep.h: 36 + 32 MFMAs of 16 x 16 x 32 on
// one 32-entry LDS image, Q in 72 registers, the f32 online softmax, the Newton step on the LSE), swept over the whole list in one part, so the rows of
// a sequence equal that kernel's under num_splits = 1 bit for bit.  What differs lies around it:
//
//   work split   one workgroup of four waves per (token, block of up to 64 heads) on a ONE-dimensional grid of total_q * ceil(H / 64) workgroups,
//                item = token * head blocks + head block.  A prefill step has thousands of them, so there is no list split, no workspace and no
//                combine kernel.  The owner of the token is found once per workgroup: kvappend_varlen_token on a workgroup-uniform t (scalar loads
//                of cu_seqlens_q, ceil(log2(B + 1)) probes).  A token nobody owns, or one at a negative position, writes its zeros and -inf and
//                ends before it has read q.  (A map of the workgroup id that kept a token's head blocks and its neighbours on one XCD was measured
//                and changed nothing beyond the spreads: DESIGN.md section 37.  It is not here.)
//   gather       no load is predicated per lane: a lane whose entry is invalid takes the tile's FIRST VALID entry in its place (the ballot's lowest
//                bit, one v_readlane of the entry), resolves that — the same block-table slot, the same row — and loads it; the zero-select happens
//                when the registers are written to LDS, behind the MFMAs.  A tile without a valid entry loads nothing (a wave-uniform branch) and
//                is all zeros by the same select.
//   pipeline     one stage deeper than the decode kernel's, so that every load is issued AHEAD of a tile's MFMAs and nothing it returns is looked
//                at before them: while tile t is computed on, the rows of tile t + 1, the block-table entries of tile t + 2 and the list entries
//                of tile t + 3 are in flight.  (Under the decode kernel's three stages the compiler waits vmcnt(0) for the entries of t + 2 right
//                behind the row loads, because a conditionally issued load cannot be counted past.)
//
// Safety: cu_seqlens_q, the lengths, the lists and the block table are device data nobody validated.  A sequence index comes from
// kvappend_varlen_token alone; len is clamped into [0, capacity_keys]; an address is formed from a VALID entry only (0 <= j <= pos < len), its own or
// the tile's first, so no cache row and no block-table entry is addressed that a valid entry of this token does not name; page ids are clamped into
// the pool; t < total_q by the grid.
#pragma once
#include <stdint.h>

#include "fa2_decode_mla_sparse.hip.h"      // mla_sparse_entry, mla_sparse_head_blocks, the dense kernel's constants and staging helpers

namespace fa2 {

struct PrefillMlaSparseParams {
    const void *q, *k;          // q [total_q, H, 576]; the latent cache (16-bit, or e4m3 rows of 656 bytes)
    void* o;                    // [total_q, H, 512]
    float* lse;                 // [H, total_q] f32, log2 units as every kernel here writes it
    const int* idx;             // indices [total_q, topk] int32: logical key positions of the token's sequence
    const int* cu;              // cu_seqlens_q [B + 1], device
    const int* lens;            // cache_seqlens [B], device
    const int* bt;              // block_table (paged) or null
    int B, H, topk;
    int page_size, num_pages;   // page_size 0 = contiguous cache
    int64_t capacity_keys;
    int64_t qs[2], os[2];       // element strides {token, head}
    int64_t ks[3];              // {batch | page, -, row}: elements, or bytes of an e4m3 cache
    int64_t ls, is, bts;        // the lse head stride, the indices row stride, the block-table row stride
    float c;                    // scale * log2(e)
};

#if defined(__HIPCC__)

// the zero-select of the e4m3 staging: a row no valid entry names travels as zero bits (codes, scales and the rotary chunk), whatever was loaded
__device__ __forceinline__ void mla_fp8_keep(MlaFp8Regs& s, bool keep) {
    const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) s.code[i] = keep ? s.code[i] : zero;
    s.scale = keep ? s.scale : zero;
    s.rope = keep ? s.rope : zero;
}

// (the cache format: the compile-time constant FP8 of the one body, csrc/fa2_prefill_mla_sparse_sweep.h, as in csrc/fa2_decode_mla_sparse.hip.h)
template <bool BF16>
__global__ __launch_bounds__(kDecodeWaves * 64) void prefill_mla_sparse_kernel(const PrefillMlaSparseParams p) {
    constexpr bool FP8 = false;
#include "fa2_prefill_mla_sparse_sweep.h"
}
// ... on an e4m3 latent cache (prefill_mla_sparse_fp8_hip.cpp)
template <bool BF16>
__global__ __launch_bounds__(kDecodeWaves * 64) void prefill_mla_sparse_fp8_kernel(const PrefillMlaSparseParams p) {
    constexpr bool FP8 = true;
#include "fa2_prefill_mla_sparse_sweep.h"
}

#endif  // __HIPCC__

}  // namespace fa2

#if defined(__HIPCC__)
#include "fa2_launch.h"
namespace fa2 {
// prefill_mla_sparse_hip.cpp: the kernel above on a grid of `items` = total_q * head blocks workgroups
FA2_LAUNCHER(launch_prefill_mla_sparse, (const PrefillMlaSparseParams& p, uint32_t items, hipStream_t stream), (p, items, stream))
// prefill_mla_sparse_fp8_hip.cpp: the same grid on prefill_mla_sparse_fp8_kernel
FA2_LAUNCHER(launch_prefill_mla_sparse_fp8, (const PrefillMlaSparseParams& p, uint32_t items, hipStream_t stream), (p, items, stream))
}  // namespace fa2
#endif
