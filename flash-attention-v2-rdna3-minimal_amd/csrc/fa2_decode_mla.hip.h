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
//
// e4m3 latents (fa2_fwd_decode_mla_fp8): rows of 656 bytes — 512 codes, four f32 scales, 64 rotary columns in the I/O dtype —
// staged through 24 registers and converted on the way into the same LDS image (decode_mla_fp8_kernel, below); everything that reads the image is shared.
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

// ---- the e4m3 latent row (fa2_fwd_decode_mla_fp8): 512 OCP e4m3 codes, four f32 scales (scale g: columns 128 g .. 128 g + 127),
// then the 64 rotary columns in the I/O dtype — 656 bytes, 41 chunks of 16.  The cache's strides count BYTES.
constexpr int kMlaFp8ScaleOff = kMlaDv;                        // 512
constexpr int kMlaFp8RopeOff = kMlaFp8ScaleOff + 16;           // 528
constexpr int kMlaFp8RowBytes = kMlaFp8RopeOff + (kMlaD - kMlaDv) * 2;      // 656
constexpr int kMlaFp8Group = 128;                              // columns per scale
// a row stride the kernel can address: whole rows that do not overlap, every chunk 16-byte aligned
FA2_DEC_HD inline bool mla_fp8_row_stride_ok(int64_t bytes) { return bytes >= kMlaFp8RowBytes && (bytes & 15) == 0; }
// The staging map of a 32-key tile onto 256 threads: thread t serves ONE row, t / 8, and the column eighth e = t % 8 of it.  Its load i (0 .. 3) is
// code chunk 8 i + e — the eight threads of a row read 128 consecutive bytes, a whole cache line, per load, and the chunk's scale group is i, the
// same for all threads, so the row's four scales are ONE 16-byte load — and its one rotary chunk is chunk e of the row's eight.
struct MlaFp8Stage { int row, eighth; };
FA2_DEC_HD inline MlaFp8Stage mla_fp8_stage(int t) { return MlaFp8Stage{t >> 3, t & 7}; }
FA2_DEC_HD inline int mla_fp8_code_chunk(int i, int eighth) { return 8 * i + eighth; }              // its byte offset in the row: 16 x; its scale group: i
FA2_DEC_HD inline int mla_fp8_scale_group(int chunk) { return chunk * 16 / kMlaFp8Group; }

#if defined(__HIPCC__)

// One thread's share of a staged e4m3 tile, as it lies in memory: 24 registers where the 16-bit kernel holds 36
struct MlaFp8Regs { u32x4 code[4], scale, rope; };
constexpr int kMlaFp8Pieces = 9;       // LDS writes of 16 bytes a thread owes a tile: eight half chunks of codes, one rotary chunk
// The staged registers as values made HERE (no instruction): what is computed from them stays behind this point.  Without it the compiler hoists the
// conversion above the S MFMAs, next to the loads, where it waits for them at once and holds 36 converted registers through the first product.
__device__ __forceinline__ void mla_fp8_pin(MlaFp8Regs& s) {
    asm volatile("" : "+v"(s.code[0]), "+v"(s.code[1]), "+v"(s.code[2]), "+v"(s.code[3]), "+v"(s.scale), "+v"(s.rope));
}

// Piece j of a thread's share -> the LDS image of the 16-bit kernel.  j < 8: codes 8 (j & 1) .. + 7 of code chunk j / 2, each
// rne_io(float(code) * scale) — the packed e4m3 -> f32 conversion (exact), ONE f32 multiply by the group's scale, one rounding (pack2).
// v_cvt_scalef32_pk_{f16,bf16}_fp8's scale operand serves powers of two alone, and cvt2_e4m3 followed by a 16-bit multiply would round twice.
template <bool BF16>
__device__ __forceinline__ void mla_fp8_store_piece(char* row_img, int eighth, const MlaFp8Regs& st, int j) {
    if (j == kMlaFp8Pieces - 1) {
        *reinterpret_cast<u32x4*>(row_img + kMlaDv * 2 + eighth * 16) = st.rope;
        return;
    }
    const int i = j >> 1, h = j & 1;
    const uint32_t sbits = st.scale[i];                // (a copy first: __builtin_bit_cast on the vector element itself reads element 0)
    const float sc = __builtin_bit_cast(float, sbits);
    const uint32_t w0 = st.code[i][2 * h], w1 = st.code[i][2 * h + 1];
    const f32x2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w0, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w0, 1.0f, true);
    const f32x2 c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w1, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w1, 1.0f, true);
    *reinterpret_cast<u32x4*>(row_img + mla_fp8_code_chunk(i, eighth) * 32 + h * 16) =
        (u32x4){pack2<BF16>(a[0] * sc, a[1] * sc), pack2<BF16>(b[0] * sc, b[1] * sc), pack2<BF16>(c[0] * sc, c[1] * sc), pack2<BF16>(d[0] * sc, d[1] * sc)};
}

// DecodeParams as fa2_fwd_decode_mla fills it: k = the latent cache (v unused), Hkv = 1, G = H, rows = Nq * H, ks = {batch | page, -, row}.
// FP8: the cache holds e4m3 rows (above; ks in bytes).  Only the staging differs: global -> 24 registers as the bytes lie in memory -> converted on the
// way into the SAME LDS image, so every read of the image, the softmax and the epilogue are the 16-bit kernel's statements.  The conversion of tile
// t + 1 is spread over tile t's 32 P . V MFMAs, nine pieces three MFMAs apart: its ~150 VALU instructions issue in the MFMAs' shadow (a workgroup owns
// its CU, one wave per SIMD: nothing else would fill it), and it sits in the SECOND product so that the loads, issued before the first, have had the
// 72 S MFMAs to land.  The barrier stays where it was: behind the last write of tile t + 1, which frees tile t's buffer.
// The cache format is the compile-time constant FP8 of the one body, csrc/fa2_decode_mla_sweep.h, which both kernels include.
template <bool BF16>
__global__ __launch_bounds__(kDecodeWaves * 64) void decode_mla_kernel(const DecodeParams p) {
    constexpr bool FP8 = false;
#include "fa2_decode_mla_sweep.h"
}
// ... on an e4m3 latent cache (decode_mla_fp8_hip.cpp)
template <bool BF16>
__global__ __launch_bounds__(kDecodeWaves * 64) void decode_mla_fp8_kernel(const DecodeParams p) {
    constexpr bool FP8 = true;
#include "fa2_decode_mla_sweep.h"
}

#endif  // __HIPCC__

}  // namespace fa2

#if defined(__HIPCC__)
#include "fa2_launch.h"              // (includes nothing of this file: the launcher's declaration needs FA2_LAUNCHER alone)
namespace fa2 {
// decode_mla_hip.cpp: the kernel above on a grid of (p.nsplit, row blocks, B) workgroups, then — p.nsplit > 1 — decode_combine_kernel at head dim 512
FA2_LAUNCHER(launch_decode_mla, (const DecodeParams& p, hipStream_t stream), (p, stream))
// decode_mla_fp8_hip.cpp: the same grid and combine on decode_mla_fp8_kernel
FA2_LAUNCHER(launch_decode_mla_fp8, (const DecodeParams& p, hipStream_t stream), (p, stream))
}  // namespace fa2
#endif
