// fa2_decode.hip.h — KV-cache decode attention (fa2_fwd_decode; include/fa2_gfx950.h has the contract, DESIGN.md section 20 the reasons).
//
// A few new query tokens per sequence against a preallocated cache whose valid length lives on the device.  One workgroup serves one item
// (sequence b, K / V head hkv, part s): the Nq * G query rows of the group (G = H / Hkv) are the M rows of v_mfma_f32_16x16x32, in RT row tiles of
// 16, so K and V are fetched once per group and not once per query head.  The part sweeps the key tiles decode_part_range gives it (the ONE place
// that decides it, host and device); its four waves take those tiles in turn, each with a private online-softmax state, and are merged through LDS
// at the end.
//
//   S^T[key, row] = K[key, :] . Q[row, :]      A = K fragment, loaded from global memory STRAIGHT into VGPRs (16 bytes per lane: the lane's key, 8 of
//                                              its columns — the operand map itself), B = Q fragment (registers for the whole sweep)
//   O^T[d, row]  += V^T[d, key] . P^T[key, row] A = V^T fragment, B = P: the S^T accumulator of a lane holds 4 keys of ONE row in each 16-key block,
//                                              so the two blocks of a 32-key tile, rounded to the I/O dtype, ARE the B fragment (k slot j of lane
//                                              group g = key 16 (j >> 2) + 4 g + (j & 3)); no lane movement for P.
// K is used once per workgroup, so it never visits LDS.  V needs its keys along the MFMA k dimension, which a row-major 16-byte load cannot give: a
// wave writes its V tile to a PRIVATE LDS slab as it came from memory (coalesced 256-byte rows) and reads it back with ds_read_b64_tr_b16 in exactly
// the k order P has.  The slab is private to the wave, so the sweep has no workgroup barrier; the tiles of the next step are loaded into registers
// before the current one is computed on.
//
// Safety (the lengths and the block table are device data nobody validated): len is clamped into [0, capacity_keys], every page id into
// [0, num_pages), every key index a lane forms into [0, len - 1] before it becomes an address.  Keys at or beyond len contribute nothing whatever
// the cache holds there: their scores are replaced by -inf (a select on the position, not arithmetic on the score) and their V rows by zero bits
// before they reach LDS, since 0 * NaN is NaN.
//
// FP8 caches (fa2_fwd_decode_fp8): the same body with the compile-time cache format FP8.  K and V are OCP e4m3 bytes, half the
// bytes per key, and become the I/O dtype in registers (v_cvt_scalef32_pk_{f16,bf16}_fp8 at scale 1: exact, every finite e4m3 value is a f16 and a
// bf16 value).  A lane still takes 16 bytes of its key per load — now 16 columns, which feed TWO k-steps of S^T = K Q^T; the contraction index may be
// permuted freely, so Q's B fragments are loaded once in the same permutation (k-step dc of lane group g = columns 64 (dc >> 1) + 16 g + 8 (dc & 1) ..).
// V is converted between the registers and the slab, whose format, transposed reads and P . V MFMAs are unchanged.  k_descale[b, hkv] is folded into
// the f32 score scale, v_descale[b, hkv] multiplies the normalised f32 row before its one rounding (split calls: before the workspace, so the combine
// kernel is the same).  The zero-bit select of V rows at or beyond len acts on the raw bytes (0x00 is +0), the -inf select of the scores on positions.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "fa2_scoremod.h"            // smod_cap, smod_alibi: the one copy of the score modifiers' arithmetic

#if defined(__HIPCC__) || defined(__CUDACC__)
#include "fa2_fwd_kernel.hip.h"      // the vector types, pack2, cvt8_e4m3
#define FA2_DEC_HD __host__ __device__
#else
#define FA2_DEC_HD
#endif

namespace fa2 {

constexpr int kDecodeTile = 32;        // keys per tile: divides 64, so a tile never straddles a page (page sizes are multiples of 64)
constexpr int kDecodeMaxSplit = 16;    // parts per item
constexpr int kDecodeMaxRows = 64;     // Nq * G query rows per K / V head: four row tiles of 16
constexpr int kDecodeWaves = 4;

FA2_DEC_HD inline int decode_clamp_len(int64_t len, int64_t capacity_keys) {
    return (int)(len < 0 ? 0 : len > capacity_keys ? capacity_keys : len);
}

// The key tiles part `part` of `nsplit` sweeps for a sequence of `len` keys: [*first, *first + *n).  tiles = ceil(len / tile), per = ceil(tiles / nsplit),
// part s takes [s * per, min((s + 1) * per, tiles)).  len is clamped into [0, capacity_keys] HERE.  (Nq does not shorten the sweep: the last query row
// sits at position len - 1 and sees every valid key.)
FA2_DEC_HD inline void decode_part_range(int64_t len, int64_t capacity_keys, int Nq, int tile, int nsplit, int part, int* first, int* n) {
    (void)Nq;
    const int l = decode_clamp_len(len, capacity_keys);
    const int tiles = (int)(((int64_t)l + tile - 1) / tile);
    const int per = (tiles + nsplit - 1) / nsplit;
    const int64_t lo = (int64_t)part * per, hi = lo + per < tiles ? lo + per : tiles;
    *first = lo < hi ? (int)lo : 0;
    *n = lo < hi ? (int)(hi - lo) : 0;
}

// The lowest key any query row of a sequence sees under a window of `window_left` keys (-1: no window): row 0 sits at len - Nq and keeps the keys
// j >= len - Nq - window_left.  len: already clamped.
FA2_DEC_HD inline int decode_window_lo(int len, int Nq, int window_left) {
    const int64_t lo = window_left < 0 ? 0 : (int64_t)len - Nq - window_left;
    return lo < 0 ? 0 : (int)lo;
}

// ... and the key tiles of a part under that window (fa2_fwd_decode_window): the sweep starts at the tile that holds `lo`,
// t0 = lo / tile, t1 = ceil(len / tile), per = ceil((t1 - t0) / nsplit), part s takes [t0 + s * per, min(t0 + (s + 1) * per, t1)).  A tile that lies
// wholly below lo is in no part: its page is never addressed.  window_left = -1 gives exactly decode_part_range's answer.
FA2_DEC_HD inline void decode_window_part_range(int64_t len, int64_t capacity_keys, int Nq, int window_left, int tile, int nsplit, int part, int* first,
                                                int* n) {
    const int l = decode_clamp_len(len, capacity_keys);
    const int t0 = decode_window_lo(l, Nq, window_left) / tile, t1 = (int)(((int64_t)l + tile - 1) / tile);
    const int per = (t1 - t0 + nsplit - 1) / nsplit;
    const int64_t lo = t0 + (int64_t)part * per, hi = lo + per < t1 ? lo + per : t1;
    *first = lo < hi ? (int)lo : 0;
    *n = lo < hi ? (int)(hi - lo) : 0;
}

// The key position new token `i` of `Nnew` is appended at (fa2_kvcache_append; csrc/fa2_kvappend.hip.h), host and device: `len` counts the valid keys
// INCLUDING the new tokens, so token i sits at len - Nnew + i — the position decode's query row i has.  -1 = skipped: a position outside
// [0, capacity_keys) is never clamped onto a valid row, because a clamped write would destroy a live key.
FA2_DEC_HD inline int64_t kvappend_slot(int64_t len, int64_t capacity_keys, int Nnew, int i) {
    const int64_t p = len - Nnew + i;
    return p < 0 || p >= capacity_keys ? -1 : p;
}

// The sequence that owns packed token `t` (fa2_kvcache_append_varlen; csrc/fa2_kvappend.hip.h), host and device: cu[0 .. B] are the row offsets of B
// sequences, sequence s owning the rows [cu[s], cu[s + 1]).  -> true with *s in [0, B), *i = t - cu[s] in [0, *nnew) and *nnew = cu[s + 1] - cu[s];
// false: no sequence owns t (t < cu[0], t >= cu[B], or an array that is no ascending list of offsets).  cu is device data nobody validated: the search
// is an upper bound over cu[1 .. B] whose probes lo + half stay inside [1, B] whatever it reads (lo + n <= B is kept by both branches) and whose trip
// count depends on B alone (n halves, rounding down: ceil(log2(B + 1)) probes); on an ascending array it ends at the last j with cu[j] <= t, which
// skips every zero-length sequence that shares t's offset.  The explicit check behind it makes the answer consistent on ANY array: a sequence is
// named only when 0 <= cu[s] <= t < cu[s + 1], so i and nnew are what the caller's arithmetic assumes (and fit an int), or nothing is named.
FA2_DEC_HD inline bool kvappend_varlen_token(const int* cu, int B, int64_t t, int* s, int* i, int* nnew) {
    int lo = 0;
    for (int n = B; n > 0;) {
        const int half = (n + 1) >> 1;
        if (cu[lo + half] <= t) lo += half;
        n -= half;
    }
    if (lo >= B) return false;
    const int64_t c0 = cu[lo], c1 = cu[lo + 1];
    if (c0 < 0 || t < c0 || t >= c1) return false;
    *s = lo;
    *i = (int)(t - c0);
    *nnew = (int)(c1 - c0);
    return true;
}

struct DecodeParams {
    const void *q, *k, *v;
    void* o;
    float* lse;
    const int* lens;            // cache_seqlens [B], device
    const int* bt;              // block_table (paged) or null
    float* ws;                  // nsplit > 1: [item][part][row][HD] normalised f32 partial rows, then [item][part][row] log2 LSEs
    int B, H, Hkv, Nq, G, rows; // rows = Nq * G live query rows per K / V head
    int page_size, num_pages;   // page_size 0 = contiguous cache
    int nsplit;
    int64_t capacity_keys;      // Nmax, or max_pages * page_size
    int64_t qs[3], ks[3], vs[3], os[3], ls[2], bts;      // element strides {batch | page, head, row}; lse {batch, head}; block-table row stride
    float c;                    // scale * log2(e)
    const float *kd, *vd;       // FP8 caches: k_descale / v_descale [B, Hkv], device, null = 1.0
    int64_t ds[2];              // their element strides {batch, K / V head}
    // the BAND kernels alone (fa2_fwd_decode_window), behind everything the plain kernels read:
    int window_left;            // row i also needs j >= pos_i - window_left; -1 = no window
    float softcap, inv_softcap; // 0 = no capping (make_scoremod's pair)
    float scale;                // the scale in natural units (c = scale * log2(e) serves the plain kernels)
    const float* slopes;        // ALiBi slopes f32 [.., H], device, null = none
    int64_t slope_stride;       // elements between the slope vectors of two sequences (0: one vector for all)
};

// workspace bytes of a split call (live rows only)
FA2_DEC_HD inline int64_t decode_ws_bytes(int64_t items, int nsplit, int rows, int HD) { return nsplit > 1 ? items * nsplit * rows * (HD + 1) * 4 : 0; }

#if defined(__HIPCC__)

template <bool BF16>
__device__ __forceinline__ f32x4 decode_mfma(u32x4 a, u32x4 b, f32x4 c) {
    if constexpr (BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// max / sum over the four 16-lane groups of a wave (the lanes that hold the same query row)
__device__ __forceinline__ float decode_group_max(float x) {
    x = __builtin_fmaxf(x, __shfl_xor(x, 16, 64));
    return __builtin_fmaxf(x, __shfl_xor(x, 32, 64));
}
__device__ __forceinline__ float decode_group_sum(float x) {
    x += __shfl_xor(x, 16, 64);
    return x + __shfl_xor(x, 32, 64);
}

// memory operations of the wave's lanes on its private LDS slab stay on their side of this point (no instruction: a wave's DS operations run in order)
__device__ __forceinline__ void decode_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// FP8: the caches hold OCP e4m3 bytes (KV = bytes per cache element); q, o and the arithmetic stay in the I/O dtype.
// BAND (fa2_fwd_decode_window): a sliding window, logit soft-capping and ALiBi slopes.  The part sweeps decode_window_part_range's
// tiles; a score is formed in natural units, capped (csrc/fa2_scoremod.h), biased by -slope * (pos - key) and brought to log2 units, and only then
// the position select — now with a lower bound — replaces it; V rows below the window's lowest key are zero bits like the rows at or beyond len.
template <int HD, bool BF16, int RT, bool FP8 = false, bool BAND = false>
__global__ __launch_bounds__(kDecodeWaves * 64) void decode_kernel(const DecodeParams p) {
    constexpr int KV = FP8 ? 1 : 2;
    using cache_t = typename std::conditional<FP8, uint8_t, uint16_t>::type;
    constexpr int E16 = 16 / KV;                       // cache elements per 16-byte load
    constexpr int NW = kDecodeWaves, T = kDecodeTile, DC = HD / 32, DB = HD / 16, VL = T * HD * KV / 16 / 64, GR = HD / 8;
    constexpr int KC = DC * KV / 2;                    // 16-byte loads per key of a lane: 32 columns apart (16-bit), 64 (FP8: one load feeds two k-steps)
    constexpr int VGR = HD * KV / 16;                  // 16-byte chunks of a V row in memory
    constexpr int VROWB = HD * 2 + 16;                 // bytes of a V row in the slab
    constexpr int SLAB = T * VROWB;                    // one wave's slab: its V tile, later its f32 accumulator tile [16 rows][HD + 4]
    constexpr int XROW = HD + 4;
    static_assert(16 * XROW * 4 <= SLAB, "the accumulator exchange reuses the V slab");
    static_assert(VL * 64 * 16 == T * HD * KV && T == 32 && KC >= 1, "tile geometry");
    __shared__ __attribute__((aligned(16))) char lds[NW * SLAB + 2 * NW * kDecodeMaxRows * 4];
    float* const sm = reinterpret_cast<float*>(lds + NW * SLAB);          // [NW][64] running maxima, then [NW][64] row sums
    float* const sl = sm + NW * kDecodeMaxRows;
    const float ninf = -__builtin_inff();

    const int part = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, qi = lane & 15;
    const int len = decode_clamp_len(p.lens[b], p.capacity_keys);
    int first, nt;
    if constexpr (BAND) decode_window_part_range(len, p.capacity_keys, p.Nq, p.window_left, T, p.nsplit, part, &first, &nt);
    else decode_part_range(len, p.capacity_keys, p.Nq, T, p.nsplit, part, &first, &nt);
    const int64_t item = (int64_t)b * p.Hkv + hkv;
    float* const ws_o = p.ws + ((item * p.nsplit + part) * p.rows) * HD;
    float* const ws_l = p.ws + (int64_t)p.B * p.Hkv * p.nsplit * p.rows * HD + (item * p.nsplit + part) * p.rows;

    if (p.nsplit > 1 && nt == 0) {                     // an empty part: lse = -inf, no O (the combine never reads a part of weight 0)
        if (tid < p.rows) ws_l[tid] = ninf;
        return;
    }

    // the lane's query row in each row tile: packed row r = i * G + gq -> query i, head hkv * G + gq, at key position len - Nq + i
    const uint16_t* const qbase = static_cast<const uint16_t*>(p.q) + b * p.qs[0];
    u32x4 qf[RT][DC];
    int pos[RT];
    float slope[BAND ? RT : 1];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int r = rt * 16 + qi;
        const bool live = r < p.rows;
        const int i = live ? r / p.G : 0, h = hkv * p.G + (live ? r % p.G : 0);
        pos[rt] = live ? len - p.Nq + i : -1;
        const uint16_t* row = qbase + h * p.qs[1] + i * p.qs[2] + (FP8 ? 16 : 8) * g;
#pragma unroll
        for (int dc = 0; dc < DC; ++dc)                // FP8: the column order of K's 16-byte loads
            qf[rt][dc] = live ? *reinterpret_cast<const u32x4*>(row + (FP8 ? 64 * (dc >> 1) + 8 * (dc & 1) : dc * 32)) : (u32x4){0u, 0u, 0u, 0u};
        if constexpr (BAND) slope[rt] = live && p.slopes ? p.slopes[b * p.slope_stride + h] : 0.f;      // the QUERY head's, through the map that loads q
    }
    // BAND: the widest distance pos - key a row keeps (no window: every distance a key at or below pos has; a key above pos has a negative one, which
    // the unsigned comparison refuses), and the lowest key any row of the item keeps
    const uint32_t reach = BAND ? (p.window_left < 0 ? 0x7fffffffu : (uint32_t)p.window_left) : 0u;
    const int lo = BAND ? decode_window_lo(len, p.Nq, p.window_left) : 0;
    (void)slope; (void)reach; (void)lo;
    // the score scale and the output scale of the item (FP8: the descales are device data, like the lengths); BAND: the scale in natural units
    float c = BAND ? p.scale : p.c, vd = 1.f;
    if constexpr (FP8) {
        const int64_t di = b * p.ds[0] + hkv * p.ds[1];
        if (p.kd) c *= p.kd[di];
        if (p.vd) vd = p.vd[di];
    }

    // one tile into registers: K as MFMA A fragments [16-key block][32-column chunk] (FP8: the bytes of two chunks), V as it lies in memory (chunk
    // c = i * 64 + lane of the tile's 16-byte chunks; rows at or beyond len as zero bits)
    auto load_tile = [&](int t, u32x4 (&kf)[2][KC], u32x4 (&vr)[VL]) {
        const int key0 = t * T;
        int64_t kofs, vofs;
        int row0 = key0;
        if (p.page_size) {
            const int pg = key0 / p.page_size;
            int pid = p.bt[b * p.bts + pg];
            pid = pid < 0 ? 0 : pid >= p.num_pages ? p.num_pages - 1 : pid;
            row0 = key0 - pg * p.page_size;
            kofs = pid * p.ks[0] + hkv * p.ks[1];
            vofs = pid * p.vs[0] + hkv * p.vs[1];
        } else {
            kofs = b * p.ks[0] + hkv * p.ks[1];
            vofs = b * p.vs[0] + hkv * p.vs[1];
        }
        const int last = len - 1 - key0;               // >= 0: the tile holds a valid key; a lane's key index is clamped to it
        const cache_t* const kb = static_cast<const cache_t*>(p.k) + kofs + E16 * g;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const int kk = blk * 16 + qi;
            const cache_t* row = kb + (int64_t)(row0 + (kk < last ? kk : last)) * p.ks[2];
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) kf[blk][kc] = *reinterpret_cast<const u32x4*>(row + kc * 4 * E16);
        }
        const cache_t* const vb = static_cast<const cache_t*>(p.v) + vofs;
#pragma unroll
        for (int i = 0; i < VL; ++i) {
            const int ch = i * 64 + lane, kk = ch / VGR, col = ch % VGR;
            const u32x4 x = *reinterpret_cast<const u32x4*>(vb + (int64_t)(row0 + (kk < last ? kk : last)) * p.vs[2] + col * E16);
            if constexpr (BAND) vr[i] = kk <= last && key0 + kk >= lo ? x : (u32x4){0u, 0u, 0u, 0u};
            else vr[i] = kk <= last ? x : (u32x4){0u, 0u, 0u, 0u};
        }
    };

    float m[RT], l[RT];
    f32x4 acc[RT][DB];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        m[rt] = ninf;
        l[rt] = 0.f;
#pragma unroll
        for (int db = 0; db < DB; ++db) acc[rt][db] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    char* const slab = lds + w * SLAB;
    char* const tr_addr = slab + (4 * g + (qi >> 2)) * VROWB + 8 * (qi & 3);      // ds_read_b64_tr_b16: lane 4 q + p of a group supplies row q, columns 4 p ..

    const int tend = first + nt;
    int t = first + w;
    u32x4 kf[2][KC], vr[VL];
    if (t < tend) load_tile(t, kf, vr);
    while (t < tend) {
        const int tn = t + NW;
        u32x4 kfn[2][KC] = {}, vrn[VL] = {};
        if (tn < tend) load_tile(tn, kfn, vrn);        // the next step's tiles are in flight while this one is computed on

        // S^T = K Q^T, one 16 x 16 block per (row tile, 16-key block)
        f32x4 s[RT][2];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                s[rt][blk] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dc = 0; dc < DC; ++dc) {
                    u32x4 a;
                    if constexpr (FP8) a = cvt8_e4m3<BF16>(kf[blk][dc >> 1][2 * (dc & 1)], kf[blk][dc >> 1][2 * (dc & 1) + 1]);
                    else a = kf[blk][dc];
                    s[rt][blk] = decode_mfma<BF16>(a, qf[rt][dc], s[rt][blk]);
                }
            }

        // V tile -> the wave's slab, rows as they lie in memory
        decode_wave_sync();                            // (the previous step's transposed reads come first)
#pragma unroll
        for (int i = 0; i < VL; ++i) {
            const int ch = i * 64 + lane;
            if constexpr (FP8) {                       // 16 columns of a key: converted here, the slab holds the I/O dtype as ever
                char* const dst = slab + (ch / VGR) * VROWB + (ch % VGR) * 32;
                *reinterpret_cast<u32x4*>(dst) = cvt8_e4m3<BF16>(vr[i][0], vr[i][1]);
                *reinterpret_cast<u32x4*>(dst + 16) = cvt8_e4m3<BF16>(vr[i][2], vr[i][3]);
            } else {
                *reinterpret_cast<u32x4*>(slab + (ch / GR) * VROWB + (ch % GR) * 16) = vr[i];
            }
        }
        decode_wave_sync();

        // online softmax: scores scaled in f32, f32 maxima and row sums, P rounded to the I/O dtype for P . V
        const int key0 = t * T;
        u32x4 pf[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            float x[8];
            float mt = ninf;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = key0 + 16 * (j >> 2) + 4 * g + (j & 3);
                if constexpr (BAND) {
                    const int dist = pos[rt] - key;
                    float y = s[rt][j >> 2][j & 3] * c;
                    if (p.softcap > 0.f) {             // wave-uniform
                        float th;
                        y = smod_cap(y, p.softcap, p.inv_softcap, &th);
                    }
                    y = smod_alibi(y, slope[rt], (float)dist) * kSmodLog2e;
                    x[j] = (uint32_t)dist <= reach ? y : ninf;      // the masks come last: 0 <= pos - key <= window_left
                } else {
                    x[j] = key <= pos[rt] ? s[rt][j >> 2][j & 3] * c : ninf;
                }
                mt = __builtin_fmaxf(mt, x[j]);
            }
            mt = decode_group_max(mt);
            const float mn = __builtin_fmaxf(m[rt], mt), mu = mn == ninf ? 0.f : mn;
            const float alpha = __builtin_amdgcn_exp2f(m[rt] - mu);
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                x[j] = __builtin_amdgcn_exp2f(x[j] - mu);
                sum += x[j];
            }
            l[rt] = l[rt] * alpha + decode_group_sum(sum);
            m[rt] = mn;
            pf[rt] = (u32x4){pack2<BF16>(x[0], x[1]), pack2<BF16>(x[2], x[3]), pack2<BF16>(x[4], x[5]), pack2<BF16>(x[6], x[7])};
#pragma unroll
            for (int db = 0; db < DB; ++db) acc[rt][db] *= alpha;
        }

        // O^T += V^T P^T: the transposed reads deliver keys 4 g .. 4 g + 3 and the same 16 rows further down — P's k order
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            const u32x2 lo = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(tr_addr + db * 32)));
            const u32x2 hi = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(tr_addr + db * 32 + 16 * VROWB)));
            const u32x4 vf = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt][db] = decode_mfma<BF16>(vf, pf[rt], acc[rt][db]);
        }

#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) kf[blk][kc] = kfn[blk][kc];
#pragma unroll
        for (int i = 0; i < VL; ++i) vr[i] = vrn[i];
        t = tn;
    }

    // merge the four waves' states: maxima and sums first, then one row tile of accumulators at a time through the slabs
    if (g == 0) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            sm[w * kDecodeMaxRows + rt * 16 + qi] = m[rt];
            sl[w * kDecodeMaxRows + rt * 16 + qi] = l[rt];
        }
    }
    const int orow = tid / GR, ogr = tid % GR;          // the thread's (row of the tile, 8-column granule) in the output step
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        decode_wave_sync();
        float* const xs = reinterpret_cast<float*>(slab) + qi * XROW + 4 * g;
#pragma unroll
        for (int db = 0; db < DB; ++db) *reinterpret_cast<f32x4*>(xs + db * 16) = acc[rt][db];      // acc[db][e] = O^T[d = 16 db + 4 g + e][row qi]
        __syncthreads();
        const int r = rt * 16 + orow;
        if (orow < 16 && r < p.rows) {
            float f[NW];
            float M = ninf, L = 0.f;
#pragma unroll
            for (int k = 0; k < NW; ++k) M = __builtin_fmaxf(M, sm[k * kDecodeMaxRows + r]);
            const float mu = M == ninf ? 0.f : M;
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                f[k] = __builtin_amdgcn_exp2f(sm[k * kDecodeMaxRows + r] - mu);
                L = __builtin_fmaf(f[k], sl[k * kDecodeMaxRows + r], L);
            }
            float out[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                const float* src = reinterpret_cast<const float*>(lds + k * SLAB) + orow * XROW + ogr * 8;
                const f32x4 a = *reinterpret_cast<const f32x4*>(src), c = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    out[e] = __builtin_fmaf(f[k], a[e], out[e]);
                    out[4 + e] = __builtin_fmaf(f[k], c[e], out[4 + e]);
                }
            }
            const float inv = L > 0.f ? 1.0f / L : 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) out[e] *= inv;
            if constexpr (FP8) {                       // v_descale: f32, on the normalised row, before its one rounding (or the workspace)
#pragma unroll
                for (int e = 0; e < 8; ++e) out[e] *= vd;
            }
            const float lse2 = L > 0.f ? M + __builtin_amdgcn_logf(L) : ninf;
            if (p.nsplit > 1) {
                float* dst = ws_o + (int64_t)r * HD + ogr * 8;
                *reinterpret_cast<f32x4*>(dst) = (f32x4){out[0], out[1], out[2], out[3]};
                *reinterpret_cast<f32x4*>(dst + 4) = (f32x4){out[4], out[5], out[6], out[7]};
                if (ogr == 0) ws_l[r] = lse2;
            } else {
                const int i = r / p.G, h = hkv * p.G + r % p.G;
                uint16_t* dst = static_cast<uint16_t*>(p.o) + b * p.os[0] + h * p.os[1] + i * p.os[2] + ogr * 8;
                *reinterpret_cast<u32x4*>(dst) = (u32x4){pack2<BF16>(out[0], out[1]), pack2<BF16>(out[2], out[3]), pack2<BF16>(out[4], out[5]),
                                                         pack2<BF16>(out[6], out[7])};
                if (ogr == 0) p.lse[b * p.ls[0] + h * p.ls[1] + i] = lse2;
            }
        }
        __syncthreads();                               // the slabs are rewritten for the next row tile
    }
}

// merge of the parts a split launch left in p.ws: one thread per (item, live row, 8-column granule); weights 2^(lse_s - max), parts of weight 0 are
// never read (an empty part wrote no O), one rounding.  Every part empty: zeros and -inf.
template <int HD, bool BF16>
__global__ __launch_bounds__(256) void decode_combine_kernel(const DecodeParams p) {
    constexpr int GR = HD / 8;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, total = (int64_t)p.B * p.Hkv * p.rows * GR;
    if (idx >= total) return;
    const int gr = (int)(idx % GR), r = (int)((idx / GR) % p.rows);
    const int64_t item = idx / GR / p.rows;
    const int b = (int)(item / p.Hkv), hkv = (int)(item % p.Hkv);
    const float ninf = -__builtin_inff();
    const float* const ws_l = p.ws + (int64_t)p.B * p.Hkv * p.nsplit * p.rows * HD + item * p.nsplit * p.rows + r;
    const float* const ws_o = p.ws + (item * p.nsplit * p.rows + r) * HD + gr * 8;
    float M = ninf;
    for (int s = 0; s < p.nsplit; ++s) M = __builtin_fmaxf(M, ws_l[(int64_t)s * p.rows]);
    float out[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float L = 0.f;
    if (M != ninf) {
        for (int s = 0; s < p.nsplit; ++s) {
            const float f = __builtin_amdgcn_exp2f(ws_l[(int64_t)s * p.rows] - M);
            if (f != 0.f) {
                const float* src = ws_o + (int64_t)s * p.rows * HD;
                const f32x4 a = *reinterpret_cast<const f32x4*>(src), c = *reinterpret_cast<const f32x4*>(src + 4);
                L += f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    out[e] = __builtin_fmaf(f, a[e], out[e]);
                    out[4 + e] = __builtin_fmaf(f, c[e], out[4 + e]);
                }
            }
        }
        const float inv = 1.0f / L;
#pragma unroll
        for (int e = 0; e < 8; ++e) out[e] *= inv;
    }
    const int i = r / p.G, h = hkv * p.G + r % p.G;
    uint16_t* dst = static_cast<uint16_t*>(p.o) + b * p.os[0] + h * p.os[1] + i * p.os[2] + gr * 8;
    *reinterpret_cast<u32x4*>(dst) = (u32x4){pack2<BF16>(out[0], out[1]), pack2<BF16>(out[2], out[3]), pack2<BF16>(out[4], out[5]), pack2<BF16>(out[6], out[7])};
    if (gr == 0) p.lse[b * p.ls[0] + h * p.ls[1] + i] = M != ninf ? M + __builtin_amdgcn_logf(L) : ninf;
}

#endif  // __HIPCC__

}  // namespace fa2
