// fa2_decode_mla_sparse.hip.h — sparse (top-k indexed) decode attention on a latent (MLA) KV cache (fa2_fwd_decode_mla_sparse; include/fa2_gfx950.h has
// the contract, DESIGN.md section 31 the reasons): the decode step of DeepSeek-V3.2 style models, whose indexer names, per query token, the `topk`
// cache positions that token attends.  All heads of a token share its list.
//
//   o[b, i, h] = sum over the VALID entries t of softmax_t(scale * q[b, i, h, :] . kv[b, j_t, :]) . kv[b, j_t, :512],  j_t = indices[b, i, t]
//
// An entry is a LOGICAL key position of sequence b, resolved through the block table here; it is valid iff 0 <= j <= pos, pos = len_b - Nq + i.  A
// position named twice counts twice.  The per-tile arithmetic is decode_mla_kernel's, statement for statement (csrc/fa2_decode_mla.hip.h: 36 + 32 MFMAs
// of 16 x 16 x 32 on one LDS image of 32 rows of 1 152 + 16 bytes, Q in 72 registers, f32 online softmax of the unrounded P, one barrier per tile); a
// "tile" here is 32 consecutive ENTRIES of the list, and everything that decides which cache row lies where is new:
//
//   work split   one workgroup of four waves per (part, token i x block of up to 64 heads, sequence): a block never spans two tokens, so the list, pos
//                and with them the validity of every entry are uniform over the workgroup.  A wave owns 16 heads of the token.  Parts split the LIST
//                (mla_part_range on topk), never the sequence: the plan stays a function of shapes, and work per row is topk whatever the lengths are.
//   gather       lanes 0 .. 31 of EVERY wave resolve one entry of the tile each (mla_sparse_entry, then the block table, then the 64-bit element
//                offset of the row), so a wave needs nothing from another wave and no barrier lies between resolving and fetching.  The validity of
//                the 32 entries is one wave-uniform ballot: its bit kk zeroes the staged registers of row kk and sends the scores of key kk to -inf.
//                A thread's nine 16-byte chunks lie in up to two rows of the tile; it takes each row's offset from the resolving lane by ds_bpermute.
//   pipeline     the dependent chain is one load longer than the dense kernel's (index -> block table -> row), so it runs one stage further ahead:
//                while tile t is computed on, the rows of tile t + 1 travel to registers and the entries of tile t + 2 are resolved.
//
// Safety: an invalid entry (padding, negative, above pos, INT32_MIN / INT32_MAX) never becomes part of an address — neither its block-table entry nor
// its row is loaded (the loads are predicated on the validity bit).  A valid entry is below len <= capacity_keys, so its slot lies in the block table;
// the page id is clamped into the pool (prefill_clamp_page).  A tile without a valid entry loads nothing.
#pragma once
#include <stdint.h>

#include "fa2_decode_mla.hip.h"      // the dense kernel's constants and shared arithmetic, DecodeParams, decode_combine_kernel

namespace fa2 {

// What the sparse call adds to DecodeParams (a further kernel argument: the dense kernels keep their kernarg segment)
struct MlaSparse {
    const int* idx;             // indices [B, Nq, topk] int32, device: logical key positions
    int topk;
    int64_t is[2];              // element strides {batch, row}; the last dim is contiguous
};

// ---- the arithmetic the host (fa2_decode_mla_sparse_entry) and the kernel share
// Entry j of a row at position pos: valid iff 0 <= j <= pos; then the block-table slot of its page and its row inside that page.  An invalid entry
// answers slot 0, row 0 and is never addressed.
struct MlaSparseEntry { int valid, slot, row; };
FA2_DEC_HD inline MlaSparseEntry mla_sparse_entry(int j, int64_t pos, int page_keys) {
    MlaSparseEntry r;
    r.valid = j >= 0 && j <= pos;
    const int jj = r.valid ? j : 0;
    r.slot = jj / page_keys;
    r.row = jj - r.slot * page_keys;
    return r;
}
// blocks of up to 64 heads per token, and the row blocks (workgroups per part and sequence) of a call
FA2_DEC_HD inline int mla_sparse_head_blocks(int H) { return (H + kMlaBlockRows - 1) / kMlaBlockRows; }
FA2_DEC_HD inline int mla_sparse_row_blocks(int Nq, int H) { return Nq * mla_sparse_head_blocks(H); }

#if defined(__HIPCC__)

// DecodeParams as fa2_fwd_decode_mla fills it (rows = Nq * H: the workspace row of (token i, head h) stays r = i * H + h, so decode_combine_kernel<512>
// merges a split call unchanged)
// (the cache format: the compile-time constant FP8 of the one body, csrc/fa2_decode_mla_sparse_sweep.h, which both kernels include — FP8: e4m3 rows of
// 656 bytes, ks in bytes, csrc/fa2_decode_mla.hip.h has the format and the staging)
template <bool BF16>
__global__ __launch_bounds__(kDecodeWaves * 64) void decode_mla_sparse_kernel(const DecodeParams p, const MlaSparse sp) {
    constexpr bool FP8 = false;
#include "fa2_decode_mla_sparse_sweep.h"
}
// ... on an e4m3 latent cache (decode_mla_sparse_fp8_hip.cpp)
template <bool BF16>
__global__ __launch_bounds__(kDecodeWaves * 64) void decode_mla_sparse_fp8_kernel(const DecodeParams p, const MlaSparse sp) {
    constexpr bool FP8 = true;
#include "fa2_decode_mla_sparse_sweep.h"
}

#endif  // __HIPCC__

}  // namespace fa2

#if defined(__HIPCC__)
#include "fa2_launch.h"
namespace fa2 {
// decode_mla_sparse_hip.cpp: the kernel above on a grid of (p.nsplit, Nq * head blocks, B) workgroups, then — p.nsplit > 1 — decode_combine_kernel<512>
FA2_LAUNCHER(launch_decode_mla_sparse, (const DecodeParams& p, const MlaSparse& sp, hipStream_t stream), (p, sp, stream))
// decode_mla_sparse_fp8_hip.cpp: the same grid and combine on decode_mla_sparse_fp8_kernel
FA2_LAUNCHER(launch_decode_mla_sparse_fp8, (const DecodeParams& p, const MlaSparse& sp, hipStream_t stream), (p, sp, stream))
}  // namespace fa2
#endif
