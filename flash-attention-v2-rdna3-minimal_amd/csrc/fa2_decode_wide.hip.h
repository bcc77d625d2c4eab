// fa2_decode_wide.hip.h — KV-cache decode attention at head dim 256 (fa2_fwd_decode_wide; include/fa2_gfx950.h has the contract, DESIGN.md section 38 the
// reasons).  The contract, the products and the data paths are csrc/fa2_decode.hip.h's: S^T = K Q^T with K loaded from memory straight into A fragments,
// O^T += V^T P^T with V through a wave-private LDS slab read by ds_read_b64_tr_b16 and P going from accumulator to operand in place, 32-key tiles, four waves
// that take the tiles of a part in turn and merge at the end, decode_part_range / decode_window_part_range as the one place that names a part's tiles.
//
// What is its own is where the operands live, because at 256 columns that kernel's plan (the whole next tile, the current K fragments, Q and O^T of every
// row tile resident per wave) needs more than the 512 registers a lane of a four-wave workgroup has as soon as there are two row tiles:
//
//   rows        a workgroup serves at most TWO row tiles (32 rows).  33 .. 64 rows per K / V head run as two row blocks — one more factor of grid.x — that
//               stream K and V once each and write their own rows of the same parts, so the workspace and the combine see `rows` as ever.
//   O^T         RT * 64 f32 registers per lane, the accumulator operand of the second product; they are rescaled only in a step whose running maximum
//               moved in some lane of the wave (a wave-uniform branch; multiplying by 1.0f is exact, so the bits do not depend on it).
//   Q           one row tile: 32 registers, resident.  Two row tiles: NOT in registers — the workgroup writes the block's 32 rows once into an LDS image
//               (pitch 528 bytes: the 16 lanes of a ds_read_b128 phase hit 16 distinct groups of four banks) and each k-step reads its two B fragments.
//   K, V        one row tile: the next tile is loaded into a second register set a whole step ahead (128 + 128 registers: there is room).  Two row
//               tiles: ONE register set.  A step's K fragments are dead after the first product and its V rows after they are stored to the slab, so the
//               next tile's K loads are issued behind the first product and its V loads behind the slab stores; both fly under the softmax and the
//               second product.
//   merge       maxima and sums, then one f32 row tile at a time through the slabs: 16 * (256 + 4) * 4 = 16 640 bytes fit a 16 896-byte slab; 256 threads
//               cover 8 rows of 32 granules, so a row tile leaves in two halves.
//
// LDS: four slabs of 16 896 bytes, the Q image (two row tiles) of 16 896, 1 KiB of maxima and sums — 68 608 / 85 504 bytes, dynamic, one workgroup per CU
// (which is what the registers allow).  Safety is fa2_decode.hip.h's, clamp for clamp: the length, every page id, every key index; -inf selected on the
// position, zero bits selected for V rows no query row may see.
#pragma once
#include "fa2_decode.hip.h"

namespace fa2 {

constexpr int kDecodeWideHD = 256;
constexpr int kDecodeWideBlockRows = 32;       // query rows per workgroup: two row tiles

FA2_DEC_HD inline int decode_wide_row_tiles(int rows) { return rows <= 16 ? 1 : 2; }
FA2_DEC_HD inline int decode_wide_row_blocks(int rows) { return (rows + kDecodeWideBlockRows - 1) / kDecodeWideBlockRows; }
FA2_DEC_HD constexpr int decode_wide_lds_bytes(int row_tiles) {
    return (kDecodeWaves + (row_tiles > 1 ? 1 : 0)) * kDecodeTile * (kDecodeWideHD * 2 + 16) + 2 * kDecodeWaves * kDecodeWideBlockRows * 4;
}

#if defined(__HIPCC__)

template <bool BF16, int RT, bool FP8, bool BAND>
__global__ __launch_bounds__(kDecodeWaves * 64) void decode_wide_kernel(const DecodeParams p) {
    static_assert(RT == 1 || RT == 2, "a workgroup serves one or two row tiles");
    constexpr int HD = kDecodeWideHD, KV = FP8 ? 1 : 2;
    using cache_t = typename std::conditional<FP8, uint8_t, uint16_t>::type;
    constexpr int E16 = 16 / KV;
    constexpr int NW = kDecodeWaves, T = kDecodeTile, DC = HD / 32, DB = HD / 16, VL = T * HD * KV / 16 / 64, GR = HD / 8;
    constexpr int KC = DC * KV / 2, VGR = HD * KV / 16;
    constexpr int ROWB = HD * 2 + 16;                  // bytes of a row in a slab and in the Q image
    constexpr int SLAB = T * ROWB, XROW = HD + 4, BR = 16 * RT;
    constexpr bool DEEP = RT == 1;                     // the next tile in a second register set, a whole step ahead
    static_assert(16 * XROW * 4 <= SLAB && VL * 64 * 16 == T * HD * KV && T == 32, "tile geometry");
    extern __shared__ __attribute__((aligned(16))) char wide_lds[];
    char* const qimg = wide_lds + NW * SLAB;                                               // RT == 2: [32 rows][ROWB]
    float* const sm = reinterpret_cast<float*>(qimg + (RT > 1 ? SLAB : 0));                // [NW][32] running maxima, then [NW][32] row sums
    float* const sl = sm + NW * kDecodeWideBlockRows;
    const float ninf = -__builtin_inff();

    const int part = blockIdx.x % p.nsplit, rb = blockIdx.x / p.nsplit, hkv = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, qi = lane & 15;
    const int len = decode_clamp_len(p.lens[b], p.capacity_keys);
    int first, nt;
    if constexpr (BAND) decode_window_part_range(len, p.capacity_keys, p.Nq, p.window_left, T, p.nsplit, part, &first, &nt);
    else decode_part_range(len, p.capacity_keys, p.Nq, T, p.nsplit, part, &first, &nt);
    const int64_t item = (int64_t)b * p.Hkv + hkv;
    float* const ws_o = p.ws + ((item * p.nsplit + part) * p.rows) * HD;
    float* const ws_l = p.ws + (int64_t)p.B * p.Hkv * p.nsplit * p.rows * HD + (item * p.nsplit + part) * p.rows;
    const int row0 = rb * kDecodeWideBlockRows;        // the block's first packed row

    if (p.nsplit > 1 && nt == 0) {                     // an empty part: lse = -inf, no O (the combine never reads a part of weight 0)
        if (tid < BR && row0 + tid < p.rows) ws_l[row0 + tid] = ninf;
        return;
    }

    // packed row r = i * G + gq -> query i, head hkv * G + gq, at key position len - Nq + i
    const uint16_t* const qbase = static_cast<const uint16_t*>(p.q) + b * p.qs[0];
    const int qcol = (FP8 ? 16 : 8) * g;               // FP8: the column order of K's 16-byte loads (fa2_decode.hip.h)
    u32x4 qf[RT == 1 ? DC : 1];
    int pos[RT];
    float slope[BAND ? RT : 1];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int r = row0 + rt * 16 + qi;
        const bool live = r < p.rows;
        const int i = live ? r / p.G : 0, h = hkv * p.G + (live ? r % p.G : 0);
        pos[rt] = live ? len - p.Nq + i : -1;
        if constexpr (RT == 1) {
            const uint16_t* row = qbase + h * p.qs[1] + i * p.qs[2] + qcol;
#pragma unroll
            for (int dc = 0; dc < DC; ++dc)
                qf[dc] = live ? *reinterpret_cast<const u32x4*>(row + (FP8 ? 64 * (dc >> 1) + 8 * (dc & 1) : dc * 32)) : (u32x4){0u, 0u, 0u, 0u};
        }
        if constexpr (BAND) slope[rt] = live && p.slopes ? p.slopes[b * p.slope_stride + h] : 0.f;
    }
    if constexpr (RT > 1) {                            // the Q image: 32 rows of 32 16-byte chunks, dead rows as zeros
#pragma unroll
        for (int k = 0; k < BR * GR / (NW * 64); ++k) {
            const int ch = k * NW * 64 + tid, row = ch / GR, col = ch % GR, r = row0 + row;
            const bool live = r < p.rows;
            const int i = live ? r / p.G : 0, h = hkv * p.G + (live ? r % p.G : 0);
            *reinterpret_cast<u32x4*>(qimg + row * ROWB + col * 16) =
                live ? *reinterpret_cast<const u32x4*>(qbase + h * p.qs[1] + i * p.qs[2] + col * 8) : (u32x4){0u, 0u, 0u, 0u};
        }
        __syncthreads();
    }
    (void)qf;
    const uint32_t reach = BAND ? (p.window_left < 0 ? 0x7fffffffu : (uint32_t)p.window_left) : 0u;
    const int lo = BAND ? decode_window_lo(len, p.Nq, p.window_left) : 0;
    (void)slope; (void)reach; (void)lo;
    float c = BAND ? p.scale : p.c, vd = 1.f;
    if constexpr (FP8) {
        const int64_t di = b * p.ds[0] + hkv * p.ds[1];
        if (p.kd) c *= p.kd[di];
        if (p.vd) vd = p.vd[di];
    }

    // where tile t lies: the element offsets of its page (or sequence) and head in K and V, its first row there, and the last valid key of the tile
    struct Where { int64_t kofs, vofs; int row, last, key0; };
    auto where = [&](int t) {
        Where x;
        x.key0 = t * T;
        x.row = x.key0;
        if (p.page_size) {
            const int pg = x.key0 / p.page_size;
            int pid = p.bt[b * p.bts + pg];
            pid = pid < 0 ? 0 : pid >= p.num_pages ? p.num_pages - 1 : pid;
            x.row = x.key0 - pg * p.page_size;
            x.kofs = pid * p.ks[0] + hkv * p.ks[1];
            x.vofs = pid * p.vs[0] + hkv * p.vs[1];
        } else {
            x.kofs = b * p.ks[0] + hkv * p.ks[1];
            x.vofs = b * p.vs[0] + hkv * p.vs[1];
        }
        x.last = len - 1 - x.key0;                     // >= 0: the tile holds a valid key; a lane's key index is clamped to it
        return x;
    };
    // K as MFMA A fragments [16-key block][32-column chunk] (FP8: the bytes of two chunks)
    auto load_k = [&](const Where& x, u32x4 (&kf)[2][KC]) {
        const cache_t* const kb = static_cast<const cache_t*>(p.k) + x.kofs + E16 * g;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const int kk = blk * 16 + qi;
            const cache_t* row = kb + (int64_t)(x.row + (kk < x.last ? kk : x.last)) * p.ks[2];
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) kf[blk][kc] = *reinterpret_cast<const u32x4*>(row + kc * 4 * E16);
        }
    };
    // V as it lies in memory (chunk i * 64 + lane of the tile's 16-byte chunks); rows no query row may see as zero bits
    auto load_v = [&](const Where& x, u32x4 (&vr)[VL]) {
        const cache_t* const vb = static_cast<const cache_t*>(p.v) + x.vofs;
#pragma unroll
        for (int i = 0; i < VL; ++i) {
            const int ch = i * 64 + lane, kk = ch / VGR, col = ch % VGR;
            const u32x4 y = *reinterpret_cast<const u32x4*>(vb + (int64_t)(x.row + (kk < x.last ? kk : x.last)) * p.vs[2] + col * E16);
            if constexpr (BAND) vr[i] = kk <= x.last && x.key0 + kk >= lo ? y : (u32x4){0u, 0u, 0u, 0u};
            else vr[i] = kk <= x.last ? y : (u32x4){0u, 0u, 0u, 0u};
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

    char* const slab = wide_lds + w * SLAB;
    char* const tr_addr = slab + (4 * g + (qi >> 2)) * ROWB + 8 * (qi & 3);
    const char* const q_addr = qimg + qi * ROWB + 2 * qcol;

    const int tend = first + nt;
    int t = first + w;
    u32x4 kf[2][KC], vr[VL];
    if (t < tend) {
        const Where x = where(t);
        load_k(x, kf);
        load_v(x, vr);
    }
    while (t < tend) {
        const int tn = t + NW;
        u32x4 kfn[DEEP ? 2 : 1][DEEP ? KC : 1] = {}, vrn[DEEP ? VL : 1] = {};
        if constexpr (DEEP) {
            if (tn < tend) {
                const Where x = where(tn);
                load_k(x, kfn);
                load_v(x, vrn);
            }
        }

        // S^T = K Q^T, one 16 x 16 block per (row tile, 16-key block); two row tiles: the k-step's two Q fragments come from the image
        f32x4 s[RT][2];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) s[rt][0] = s[rt][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) {
            u32x4 qb[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                if constexpr (RT == 1) qb[rt] = qf[dc];
                else qb[rt] = *reinterpret_cast<const u32x4*>(q_addr + rt * 16 * ROWB + 2 * (FP8 ? 64 * (dc >> 1) + 8 * (dc & 1) : dc * 32));
            }
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                u32x4 a;
                if constexpr (FP8) a = cvt8_e4m3<BF16>(kf[blk][dc >> 1][2 * (dc & 1)], kf[blk][dc >> 1][2 * (dc & 1) + 1]);
                else a = kf[blk][dc];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) s[rt][blk] = decode_mfma<BF16>(a, qb[rt], s[rt][blk]);
            }
        }
        Where xn = {};
        if constexpr (!DEEP) {
            if (tn < tend) {
                xn = where(tn);
                load_k(xn, kf);                        // the fragments of this step are spent
            }
        }

        // V tile -> the wave's slab, rows as they lie in memory
        decode_wave_sync();                            // (the previous step's transposed reads come first)
#pragma unroll
        for (int i = 0; i < VL; ++i) {
            const int ch = i * 64 + lane;
            if constexpr (FP8) {
                char* const dst = slab + (ch / VGR) * ROWB + (ch % VGR) * 32;
                *reinterpret_cast<u32x4*>(dst) = cvt8_e4m3<BF16>(vr[i][0], vr[i][1]);
                *reinterpret_cast<u32x4*>(dst + 16) = cvt8_e4m3<BF16>(vr[i][2], vr[i][3]);
            } else {
                *reinterpret_cast<u32x4*>(slab + (ch / GR) * ROWB + (ch % GR) * 16) = vr[i];
            }
        }
        decode_wave_sync();
        if constexpr (!DEEP) {
            if (tn < tend) load_v(xn, vr);             // ... and so are its V rows
        }

        // online softmax (numerical contract 0): f32 scaled scores, f32 maxima and sums of the unrounded P, P rounded to the I/O dtype
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
                    x[j] = (uint32_t)dist <= reach ? y : ninf;
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
            if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {      // the maximum of some row moved
#pragma unroll
                for (int db = 0; db < DB; ++db) acc[rt][db] *= alpha;
            }
        }

        // O^T += V^T P^T
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            const u32x2 vlo = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(tr_addr + db * 32)));
            const u32x2 vhi = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(tr_addr + db * 32 + 16 * ROWB)));
            const u32x4 vf = {vlo[0], vlo[1], vhi[0], vhi[1]};
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt][db] = decode_mfma<BF16>(vf, pf[rt], acc[rt][db]);
        }

        if constexpr (DEEP) {
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int kc = 0; kc < KC; ++kc) kf[blk][kc] = kfn[blk][kc];
#pragma unroll
            for (int i = 0; i < VL; ++i) vr[i] = vrn[i];
        }
        t = tn;
    }

    // merge the four waves' states: maxima and sums first, then one row tile of accumulators at a time through the slabs, leaving in two halves of 8 rows
    if (g == 0) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            sm[w * kDecodeWideBlockRows + rt * 16 + qi] = m[rt];
            sl[w * kDecodeWideBlockRows + rt * 16 + qi] = l[rt];
        }
    }
    const int ogr = tid % GR;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        decode_wave_sync();
        float* const xs = reinterpret_cast<float*>(slab) + qi * XROW + 4 * g;
#pragma unroll
        for (int db = 0; db < DB; ++db) *reinterpret_cast<f32x4*>(xs + db * 16) = acc[rt][db];      // acc[db][e] = O^T[d = 16 db + 4 g + e][row qi]
        __syncthreads();
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int orow = half * 8 + tid / GR, br = rt * 16 + orow, r = row0 + br;
            if (r < p.rows) {
                float f[NW];
                float M = ninf, L = 0.f;
#pragma unroll
                for (int k = 0; k < NW; ++k) M = __builtin_fmaxf(M, sm[k * kDecodeWideBlockRows + br]);
                const float mu = M == ninf ? 0.f : M;
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    f[k] = __builtin_amdgcn_exp2f(sm[k * kDecodeWideBlockRows + br] - mu);
                    L = __builtin_fmaf(f[k], sl[k * kDecodeWideBlockRows + br], L);
                }
                float out[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    const float* src = reinterpret_cast<const float*>(wide_lds + k * SLAB) + orow * XROW + ogr * 8;
                    const f32x4 a = *reinterpret_cast<const f32x4*>(src), c2 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        out[e] = __builtin_fmaf(f[k], a[e], out[e]);
                        out[4 + e] = __builtin_fmaf(f[k], c2[e], out[4 + e]);
                    }
                }
                const float inv = L > 0.f ? 1.0f / L : 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) out[e] *= inv;
                if constexpr (FP8) {
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
        }
        __syncthreads();                               // the slabs are rewritten for the next row tile
    }
}

#endif  // __HIPCC__

}  // namespace fa2
