// fa2_decode_mla_sweep.h — the body of decode_mla_kernel and decode_mla_fp8_kernel (csrc/fa2_decode_mla.hip.h includes it once in each, behind
// `constexpr bool FP8`; it is no header of its own).  One text, so that every statement that reads the LDS image, the softmax and the epilogue exist
// once; included, not called, because a kernel that only calls the body compiles to other registers than the kernel it replaces.
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

    // e4m3: the thread's row of the tile (mla_fp8_stage) as it lies in memory.  A row at or beyond len: the codes AND the scales as zero bits, so that
    // what is written to LDS is +0 (0 * NaN is NaN), and its rotary chunk as zero bits
    const MlaFp8Stage fs = mla_fp8_stage(tid);
    auto load_tile8 = [&](int t, MlaFp8Regs& s8) {
        const MlaTile mt = mla_tile(t, len, page_keys);
        int64_t base;
        if (p.page_size) base = (int64_t)prefill_clamp_page(p.bt[b * p.bts + mt.slot], p.num_pages) * p.ks[0];
        else base = b * p.ks[0];
        const int last = mt.rows - 1;
        const char* const row = static_cast<const char*>(p.k) + base + (int64_t)(mt.row + (fs.row < last ? fs.row : last)) * p.ks[2];
        const bool in = fs.row <= last;
        const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const u32x4 x = *reinterpret_cast<const u32x4*>(row + mla_fp8_code_chunk(i, fs.eighth) * 16);
            s8.code[i] = in ? x : zero;
        }
        const u32x4 sc = *reinterpret_cast<const u32x4*>(row + kMlaFp8ScaleOff), ro = *reinterpret_cast<const u32x4*>(row + kMlaFp8RopeOff + fs.eighth * 16);
        s8.scale = in ? sc : zero;
        s8.rope = in ? ro : zero;
    };

    float m = ninf, l = 0.f;
    f32x4 acc[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) acc[db] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int tend = first + nt;
    u32x4 st[FP8 ? 1 : NL];
    MlaFp8Regs st8;
    if (nt > 0) {
        if constexpr (FP8) {
            load_tile8(first, st8);
#pragma unroll
            for (int j = 0; j < kMlaFp8Pieces; ++j) mla_fp8_store_piece<BF16>(mla_lds + fs.row * ROWB, fs.eighth, st8, j);
        } else {
            load_tile(first, st);
            store_tile(mla_lds, st);
        }
    }
    __syncthreads();
    int cur = 0;
    for (int t = first; t < tend; ++t) {
        const bool more = t + 1 < tend;
        if constexpr (FP8) {
            if (more) load_tile8(t + 1, st8);
        } else {
            if (more) load_tile(t + 1, st);            // in flight while this tile is computed on
        }
        const char* const img = mla_lds + cur * BUF;
        char* nxt_row = nullptr;                       // (FP8) where this thread's row of tile t + 1 goes
        if constexpr (FP8) nxt_row = mla_lds + (cur ^ 1) * BUF + fs.row * ROWB;
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
            if constexpr (FP8) mla_fp8_pin(st8);
            const char* const tr_addr =img + (4 * g + (qi >> 2)) * ROWB + 8 * (qi & 3);      // lane 4 q + p of a group supplies row q, columns 4 p ..
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                const u32x2 lo = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(tr_addr + db * 32)));
                const u32x2 hi = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(tr_addr + db * 32 + 16 * ROWB)));
                const u32x4 vf = {lo[0], lo[1], hi[0], hi[1]};
                acc[db] = decode_mfma<BF16>(vf, pf, acc[db] * alpha);
                // (FP8) a piece of tile t + 1 every third MFMA.  Not under `more`: behind the last tile the other buffer is free and never read
                // again, and straight-line code is what lets the pieces be scheduled between the MFMAs
                if constexpr (FP8)
                    if (db % 3 == 1 && db / 3 < kMlaFp8Pieces) mla_fp8_store_piece<BF16>(nxt_row, fs.eighth, st8, db / 3);
            }
        }
        if constexpr (FP8) {
            if (!wave_live) {                          // a wave without rows has no MFMAs to hide behind: its share in one go
#pragma unroll
                for (int j = 0; j < kMlaFp8Pieces; ++j) mla_fp8_store_piece<BF16>(nxt_row, fs.eighth, st8, j);
            }
        } else {
            if (more) store_tile(mla_lds + (cur ^ 1) * BUF, st);
        }
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
