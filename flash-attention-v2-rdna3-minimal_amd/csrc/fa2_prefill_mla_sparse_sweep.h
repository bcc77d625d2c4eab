// fa2_prefill_mla_sparse_sweep.h — the body of prefill_mla_sparse_kernel and prefill_mla_sparse_fp8_kernel (csrc/fa2_prefill_mla_sparse.hip.h includes it
// once in each, behind `constexpr bool FP8`; it is no header of its own; csrc/fa2_decode_mla_sweep.h says why it is included and not called).  The
// statements between "S^T" and the LSE are csrc/fa2_decode_mla_sparse_sweep.h's, unchanged: the bit-for-bit property rests on that.
    constexpr int T = kMlaTile, DC = kMlaD / 32, DB = kMlaDv / 16, ROWB = kMlaRowBytes, BUF = T * ROWB;
    constexpr int CH = kMlaD / 8;                      // 16-byte chunks of a row: 72
    constexpr int NL = T * CH / (kDecodeWaves * 64);   // staged chunks per thread: 9
    static_assert(NL * kDecodeWaves * 64 == T * CH && T == 32, "tile geometry");
    extern __shared__ __attribute__((aligned(16))) char mla_lds[];
    const float ninf = -__builtin_inff();

    // the work item: (token, head block), both workgroup-uniform
    const uint32_t hb = (uint32_t)mla_sparse_head_blocks(p.H);
    const uint32_t item = blockIdx.x;
    const int64_t tok = item / hb;                     // (< total_q: the grid is total_q * hb)
    const int h0 = (int)(item % hb) * kMlaBlockRows;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, qi = lane & 15;
    const int h = h0 + w * 16 + qi;
    const bool live = h < p.H;
    const bool wave_live = h0 + w * 16 < p.H;          // (wave-uniform) a wave without heads stages and waits, no more

    // ownership, once per workgroup: scalar loads of cu_seqlens_q and of one length
    int sq = 0, ti = 0, nq = 0, pos = -1;
    if (kvappend_varlen_token(p.cu, p.B, tok, &sq, &ti, &nq)) pos = decode_clamp_len(p.lens[sq], p.capacity_keys) - nq + ti;
    uint16_t* const orow = static_cast<uint16_t*>(p.o) + tok * p.os[0] + (live ? h : 0) * p.os[1] + 4 * g;
    float* const lrow = p.lse + (live ? h : 0) * p.ls + tok;
    if (pos < 0) {                                     // nobody's token, or one at a negative position: zeros and -inf, nothing is read
        if (live) {
#pragma unroll
            for (int db = 0; db < DB; ++db) *reinterpret_cast<u32x2*>(orow + db * 16) = (u32x2){0u, 0u};
            if (g == 0) *lrow = ninf;
        }
        return;
    }

    u32x4 qf[DC];
    {
        const uint16_t* row = static_cast<const uint16_t*>(p.q) + tok * p.qs[0] + (live ? h : 0) * p.qs[1] + 8 * g;
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) qf[dc] = live ? *reinterpret_cast<const u32x4*>(row + dc * 32) : (u32x4){0u, 0u, 0u, 0u};
    }

    const int page_keys = mla_page_keys(p.page_size, p.capacity_keys);
    const int* const list = p.idx + tok * p.is;
    const int ntiles = (int)(((int64_t)p.topk + T - 1) / T);
    // the chain's first link: entry `lane` of tile t (lanes 32 .. 63 and entries at or beyond topk: -1, invalid) in two steps, the load and the
    // select, so that the select can wait behind a tile's MFMAs.  The load is unconditional: a lane without an entry reads the list's last one
    auto load_entry_raw = [&](int t) -> int {
        const int64_t e = (int64_t)t * T + (lane & (T - 1));
        return list[e < p.topk ? e : (int64_t)p.topk - 1];
    };
    auto entry_or_none = [&](int raw, int t) -> int { return lane < T && (int64_t)t * T + lane < p.topk ? raw : -1; };
    auto load_entry = [&](int t) -> int { return entry_or_none(load_entry_raw(t), t); };
    // ... its second, in three steps so that the block-table read can be in flight across a tile's MFMAs.  entry_pick: validity (-> the wave-uniform
    // mask of the tile) and the entry EVERY lane resolves — its own if valid, else the tile's first valid one (the ballot's lowest bit, one v_readlane)
    // — so the block-table read and the row loads behind it need no per-lane predicate.  No valid entry in the tile (wave-uniform): nothing is read
    auto entry_pick = [&](int j, int* jj) -> uint32_t {
        const bool valid = mla_sparse_entry(j, pos, page_keys).valid != 0;
        const uint32_t mask = (uint32_t)__builtin_amdgcn_ballot_w64(valid);
        int pick = 0;
        if (mask) pick = valid ? j : __builtin_amdgcn_readlane(j, __builtin_ctz(mask));
        *jj = pick;
        return mask;
    };
    // entry_page: the page id of that entry, as the block table holds it (a contiguous cache, or a tile without a valid entry: no read)
    auto entry_page = [&](int jj, uint32_t mask) -> int {
        return mask && p.page_size ? p.bt[sq * p.bts + mla_sparse_entry(jj, pos, page_keys).slot] : 0;
    };
    // entry_offset: the row's offset in the cache
    auto entry_offset = [&](int jj, int page) -> int64_t {
        const int64_t base = p.page_size ? (int64_t)prefill_clamp_page(page, p.num_pages) : (int64_t)sq;
        return base * p.ks[0] + (int64_t)mla_sparse_entry(jj, pos, page_keys).row * p.ks[2];
    };
    auto resolve = [&](int j, int64_t* off) -> uint32_t {
        int jj;
        const uint32_t mask = entry_pick(j, &jj);
        *off = entry_offset(jj, entry_page(jj, mask));
        return mask;
    };
    // ... its third: chunk c = i * 256 + tid of the tile's 32 x 72 chunks, from the row its chunk number names (a valid entry's row in every lane)
    const uint16_t* const kb = static_cast<const uint16_t*>(p.k);
    auto load_tile = [&](int64_t off, uint32_t mask, u32x4 (&st)[NL]) {
        if (!mask) return;
        const int olo = (int)(uint32_t)off, ohi = (int)(off >> 32);
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int ch = i * (kDecodeWaves * 64) + tid, kk = ch / CH, col = ch % CH;
            const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(kk * 4, olo), hi = (uint32_t)__builtin_amdgcn_ds_bpermute(kk * 4, ohi);
            const int64_t ro = (int64_t)(((uint64_t)hi << 32) | lo);
            st[i] = *reinterpret_cast<const u32x4*>(kb + ro + col * 8);
        }
    };
    // the zero-select lies HERE, where the registers are first needed: rows of invalid entries enter the image as zero bits
    auto store_tile = [&](char* buf, uint32_t mask, const u32x4 (&st)[NL]) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int ch = i * (kDecodeWaves * 64) + tid, kk = ch / CH;
            *reinterpret_cast<u32x4*>(buf + kk * ROWB + (ch % CH) * 16) = (mask >> kk) & 1u ? st[i] : (u32x4){0u, 0u, 0u, 0u};
        }
    };
    // e4m3 (mla_fp8_stage): a thread's six chunks lie in ONE row of the tile: one offset from the resolving lane, six unconditional loads
    const MlaFp8Stage fs = mla_fp8_stage(tid);
    auto load_tile8 = [&](int64_t off, uint32_t mask, MlaFp8Regs& s8) {
        if (!mask) return;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(fs.row * 4, (int)(uint32_t)off);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(fs.row * 4, (int)(off >> 32));
        const char* const row = static_cast<const char*>(p.k) + (int64_t)(((uint64_t)hi << 32) | lo);
#pragma unroll
        for (int i = 0; i < 4; ++i) s8.code[i] = *reinterpret_cast<const u32x4*>(row + mla_fp8_code_chunk(i, fs.eighth) * 16);
        s8.scale = *reinterpret_cast<const u32x4*>(row + kMlaFp8ScaleOff);
        s8.rope = *reinterpret_cast<const u32x4*>(row + kMlaFp8RopeOff + fs.eighth * 16);
    };

    float m = ninf, l = 0.f;
    f32x4 acc[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) acc[db] = (f32x4){0.f, 0.f, 0.f, 0.f};

    u32x4 st[FP8 ? 1 : NL];
    MlaFp8Regs st8;
#pragma unroll
    for (int i = 0; i < (FP8 ? 1 : NL); ++i) st[i] = (u32x4){0u, 0u, 0u, 0u};
    mla_fp8_keep(st8, false);                          // (a tile that loads nothing leaves the registers as they are: they hold bits, never garbage)
    // mask0 / the image: tile t; off1, mask1: tile t + 1, resolved; j2: the entries of tile t + 2, arrived; j3: those of tile t + 3, on their way
    int64_t off1 = 0;
    uint32_t mask0 = 0, mask1 = 0;
    int j2 = -1;
    {
        int64_t off0;
        const int j0 = load_entry(0), j1 = load_entry(1);
        j2 = load_entry(2);
        mask0 = resolve(j0, &off0);
        if constexpr (FP8) load_tile8(off0, mask0, st8);
        else load_tile(off0, mask0, st);
        mask1 = resolve(j1, &off1);
        if constexpr (FP8) {
            mla_fp8_keep(st8, (mask0 >> fs.row) & 1u);
#pragma unroll
            for (int j = 0; j < kMlaFp8Pieces; ++j) mla_fp8_store_piece<BF16>(mla_lds + fs.row * ROWB, fs.eighth, st8, j);
        } else {
            store_tile(mla_lds, mask0, st);
        }
    }
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < ntiles; ++t) {
        const bool more = t + 1 < ntiles;
        // every load of the iteration is issued HERE, ahead of the MFMAs, and nothing it returns is looked at before them: the block-table entries of
        // tile t + 2 (its list entries arrived an iteration ago), the list entries of tile t + 3, the rows of tile t + 1
        int jj2;
        const uint32_t mask2 = entry_pick(j2, &jj2);
        const int page2 = entry_page(jj2, mask2);
        const int raw3 = load_entry_raw(t + 3);         // (beyond the list: its last entry, dropped below)
        if constexpr (FP8) {
            if (more) load_tile8(off1, mask1, st8);
        } else {
            if (more) load_tile(off1, mask1, st);      // in flight while this tile is computed on
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
            if constexpr (FP8) {
                mla_fp8_pin(st8);
                mla_fp8_keep(st8, (mask1 >> fs.row) & 1u);             // the zero-select, behind the first product: the loads have had its MFMAs to land
            }
            const char* const tr_addr = img + (4 * g + (qi >> 2)) * ROWB + 8 * (qi & 3);      // lane 4 q + p of a group supplies row q, columns 4 p ..
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
                mla_fp8_keep(st8, (mask1 >> fs.row) & 1u);
#pragma unroll
                for (int j = 0; j < kMlaFp8Pieces; ++j) mla_fp8_store_piece<BF16>(nxt_row, fs.eighth, st8, j);
            }
        } else {
            if (more) store_tile(mla_lds + (cur ^ 1) * BUF, mask1, st);
        }
        const int64_t off2 = entry_offset(jj2, page2); // (behind the MFMAs and the rows' wait: the block-table entry has long arrived)
        __syncthreads();                               // tile t + 1 is visible, and tile t's buffer is free for t + 2
        cur ^= 1;
        mask0 = mask1;
        mask1 = mask2;
        off1 = off2;
        j2 = entry_or_none(raw3, t + 3);
    }

    // each wave owns its rows: acc[db][e] = O^T[d = 16 db + 4 g + e][head qi], normalised once, rounded once.  No valid entry: zeros and -inf
    if (!live) return;
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    // log2(l) with one Newton step on v_log_f32's answer (csrc/fa2_decode_mla.hip.h has the reason)
    const float l1 = l > 0.f ? l : 1.0f;
    float lg = __builtin_amdgcn_logf(l1);
    lg = __builtin_fmaf(__builtin_fmaf(l1, __builtin_amdgcn_exp2f(-lg), -1.0f), 1.4426950408889634f, lg);
#pragma unroll
    for (int db = 0; db < DB; ++db) {
        const f32x4 a = acc[db] * inv;
        *reinterpret_cast<u32x2*>(orow + db * 16) = (u32x2){pack2<BF16>(a[0], a[1]), pack2<BF16>(a[2], a[3])};
    }
    if (g == 0) *lrow = l > 0.f ? m + lg : ninf;
