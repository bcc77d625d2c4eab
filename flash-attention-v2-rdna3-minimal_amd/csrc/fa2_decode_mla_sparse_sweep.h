// fa2_decode_mla_sparse_sweep.h — the body of decode_mla_sparse_kernel and decode_mla_sparse_fp8_kernel (csrc/fa2_decode_mla_sparse.hip.h includes it once
// in each, behind `constexpr bool FP8`; it is no header of its own; csrc/fa2_decode_mla_sweep.h says why it is included and not called).
    constexpr int T = kMlaTile, DC = kMlaD / 32, DB = kMlaDv / 16, ROWB = kMlaRowBytes, BUF = T * ROWB;
    constexpr int CH = kMlaD / 8;                      // 16-byte chunks of a row: 72
    constexpr int NL = T * CH / (kDecodeWaves * 64);   // staged chunks per thread: 9
    static_assert(NL * kDecodeWaves * 64 == T * CH && T == 32, "tile geometry");
    extern __shared__ __attribute__((aligned(16))) char mla_lds[];
    const float ninf = -__builtin_inff();

    const int hb = mla_sparse_head_blocks(p.H);
    const int part = blockIdx.x, qi_tok = blockIdx.y / hb, h0 = (blockIdx.y % hb) * kMlaBlockRows, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, qi = lane & 15;
    const int len = decode_clamp_len(p.lens[b], p.capacity_keys);
    const int pos = len - p.Nq + qi_tok;               // (workgroup-uniform; negative: every entry is invalid)
    int first, nt;
    mla_part_range(sp.topk, sp.topk, p.nsplit, part, &first, &nt);
    float* const ws_o = p.ws + (((int64_t)b * p.nsplit + part) * p.rows) * kMlaDv;
    float* const ws_l = p.ws + (int64_t)p.B * p.nsplit * p.rows * kMlaDv + ((int64_t)b * p.nsplit + part) * p.rows;

    if (p.nsplit > 1 && nt == 0) {                     // a part without entries: lse = -inf, no O (the combine never reads a part of weight 0)
        if (tid < kMlaBlockRows && h0 + tid < p.H) ws_l[qi_tok * p.H + h0 + tid] = ninf;
        return;
    }

    // the lane's query row: head h of the block's token
    const int h = h0 + w * 16 + qi;
    const bool live = h < p.H;
    const bool wave_live = h0 + w * 16 < p.H;          // (wave-uniform) a wave without heads stages and waits, no more
    const int r = qi_tok * p.H + h;
    u32x4 qf[DC];
    {
        const uint16_t* row = static_cast<const uint16_t*>(p.q) + b * p.qs[0] + (live ? h : 0) * p.qs[1] + qi_tok * p.qs[2] + 8 * g;
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) qf[dc] = live ? *reinterpret_cast<const u32x4*>(row + dc * 32) : (u32x4){0u, 0u, 0u, 0u};
    }

    const int page_keys = mla_page_keys(p.page_size, p.capacity_keys);
    const int* const list = sp.idx + b * sp.is[0] + qi_tok * sp.is[1];
    // the chain's first link: entry `lane` of tile t (lanes 32 .. 63 and entries at or beyond topk: -1, invalid)
    auto load_entry = [&](int t) -> int {
        const int64_t e = (int64_t)t * T + lane;
        return lane < T && e < sp.topk ? list[e] : -1;
    };
    // ... its second: validity (-> the wave-uniform mask of the tile) and, for a valid entry alone, the block-table read -> the row's element offset
    auto resolve = [&](int j, int64_t* off) -> uint32_t {
        const MlaSparseEntry se = mla_sparse_entry(j, pos, page_keys);
        int64_t o = 0;
        if (se.valid) {
            if (p.page_size) o = (int64_t)prefill_clamp_page(p.bt[b * p.bts + se.slot], p.num_pages) * p.ks[0];
            else o = b * p.ks[0];
            o += (int64_t)se.row * p.ks[2];
        }
        *off = o;
        return (uint32_t)__builtin_amdgcn_ballot_w64(se.valid != 0);
    };
    // ... its third: chunk c = i * 256 + tid of the tile's 32 x 72 chunks, from the row its chunk number names; rows of invalid entries are not loaded
    // and travel as zero bits
    const uint16_t* const kb = static_cast<const uint16_t*>(p.k);
    auto load_tile = [&](int64_t off, uint32_t mask, u32x4 (&st)[NL]) {
        const int olo = (int)(uint32_t)off, ohi = (int)(off >> 32);
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int ch = i * (kDecodeWaves * 64) + tid, kk = ch / CH, col = ch % CH;
            const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(kk * 4, olo), hi = (uint32_t)__builtin_amdgcn_ds_bpermute(kk * 4, ohi);
            const int64_t ro = (int64_t)(((uint64_t)hi << 32) | lo);
            st[i] = (u32x4){0u, 0u, 0u, 0u};
            if ((mask >> kk) & 1u) st[i] = *reinterpret_cast<const u32x4*>(kb + ro + col * 8);
        }
    };
    auto store_tile = [&](char* buf, const u32x4 (&st)[NL]) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int ch = i * (kDecodeWaves * 64) + tid;
            *reinterpret_cast<u32x4*>(buf + (ch / CH) * ROWB + (ch % CH) * 16) = st[i];
        }
    };
    // e4m3 (mla_fp8_stage): a thread's six chunks lie in ONE row of the tile, so it takes one offset from the resolving lane (two ds_bpermute where the
    // 16-bit map needs eighteen) and one validity bit guards all its loads.  An invalid entry's row: not loaded; codes, scales and rotary chunk zero bits
    const MlaFp8Stage fs = mla_fp8_stage(tid);
    auto load_tile8 = [&](int64_t off, uint32_t mask, MlaFp8Regs& s8) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(fs.row * 4, (int)(uint32_t)off);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(fs.row * 4, (int)(off >> 32));
        const char* const row = static_cast<const char*>(p.k) + (int64_t)(((uint64_t)hi << 32) | lo);
        const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i) s8.code[i] = zero;
        s8.scale = zero;
        s8.rope = zero;
        if ((mask >> fs.row) & 1u) {
#pragma unroll
            for (int i = 0; i < 4; ++i) s8.code[i] = *reinterpret_cast<const u32x4*>(row + mla_fp8_code_chunk(i, fs.eighth) * 16);
            s8.scale = *reinterpret_cast<const u32x4*>(row + kMlaFp8ScaleOff);
            s8.rope = *reinterpret_cast<const u32x4*>(row + kMlaFp8RopeOff + fs.eighth * 16);
        }
    };

    float m = ninf, l = 0.f;
    f32x4 acc[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) acc[db] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int tend = first + nt;
    u32x4 st[FP8 ? 1 : NL];
    MlaFp8Regs st8;
    // mask0 / the image: tile t; off1, mask1: tile t + 1, resolved; j2: tile t + 2, its entries on their way
    int64_t off1 = 0;
    uint32_t mask0 = 0, mask1 = 0;
    if (nt > 0) {
        int64_t off0;
        mask0 = resolve(load_entry(first), &off0);
        if constexpr (FP8) load_tile8(off0, mask0, st8);
        else load_tile(off0, mask0, st);
        if (nt > 1) mask1 = resolve(load_entry(first + 1), &off1);
        if constexpr (FP8) {
#pragma unroll
            for (int j = 0; j < kMlaFp8Pieces; ++j) mla_fp8_store_piece<BF16>(mla_lds + fs.row * ROWB, fs.eighth, st8, j);
        } else {
            store_tile(mla_lds, st);
        }
    }
    __syncthreads();
    int cur = 0;
    for (int t = first; t < tend; ++t) {
        const bool more = t + 1 < tend, more2 = t + 2 < tend;
        int j2 = -1;
        if (more2) j2 = load_entry(t + 2);             // issued ahead of the rows: waiting for it leaves them in flight
        if constexpr (FP8) {
            if (more) load_tile8(off1, mask1, st8);
        } else {
            if (more) load_tile(off1, mask1, st);      // in flight while this tile is computed on
        }
        int64_t off2 = 0;
        uint32_t mask2 = 0;
        if (more2) mask2 = resolve(j2, &off2);
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
            float x[8];
            float mt = ninf;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = 16 * (j >> 2) + 4 * g + (j & 3);       // the entry of the tile this score belongs to
                x[j] = (mask0 >> key) & 1u ? s[j >> 2][j & 3] * p.c : ninf;
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
                // (FP8) a piece of tile t + 1 every third MFMA, not under `more` (csrc/fa2_decode_mla_sweep.h has the reasons)
                if constexpr (FP8)
                    if (db % 3 == 1 && db / 3 < kMlaFp8Pieces) mla_fp8_store_piece<BF16>(nxt_row, fs.eighth, st8, db / 3);
            }
        }
        if constexpr (FP8) {
            if (!wave_live) {                          // a wave without heads has no MFMAs to hide behind: its share in one go
#pragma unroll
                for (int j = 0; j < kMlaFp8Pieces; ++j) mla_fp8_store_piece<BF16>(nxt_row, fs.eighth, st8, j);
            }
        } else {
            if (more) store_tile(mla_lds + (cur ^ 1) * BUF, st);
        }
        __syncthreads();                               // tile t + 1 is visible, and tile t's buffer is free for t + 2
        cur ^= 1;
        mask0 = mask1;
        mask1 = mask2;
        off1 = off2;
    }

    // each wave owns its rows: acc[db][e] = O^T[d = 16 db + 4 g + e][head qi], normalised once, rounded once.  No valid entry: zeros and -inf
    if (!live) return;
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    // log2(l) with one Newton step on v_log_f32's answer (csrc/fa2_decode_mla.hip.h has the reason)
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
        uint16_t* dst = static_cast<uint16_t*>(p.o) + b * p.os[0] + h * p.os[1] + qi_tok * p.os[2] + 4 * g;
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            const f32x4 a = acc[db] * inv;
            *reinterpret_cast<u32x2*>(dst + db * 16) = (u32x2){pack2<BF16>(a[0], a[1]), pack2<BF16>(a[2], a[3])};
        }
        if (g == 0) p.lse[b * p.ls[0] + h * p.ls[1] + qi_tok] = lse2;
    }
