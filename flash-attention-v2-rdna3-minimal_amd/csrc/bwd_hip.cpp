// bwd_hip.cpp — instantiations and launchers of the compiler-scheduled backward kernels (fa2_bwd_kernel.hip.h) for ONE dtype:
// build.py compiles this file twice, -DFA2_TU_BF16=0 and =1.  Reference counterpart: backward_fp16 / backward_bf16
// (kernel_fp16.cu:878-1028).
// The passes themselves (kernel, grid, LDS size, split plan and merge) are fa2_pass_launch.h's; this file decides which of them run: the 4-wave dQ pass
// of small grids, the dK / dV shape per head dim, the trimmed instantiations, and it holds the merge kernel of the split passes.
#include "fa2_pass_launch.h"

#include "fa2_bwd_short.hip.h"

// -DFA2_TU_TRIM=1: this unit holds the TRIMMED instantiations instead (head dims well below the kernel's HD run only the MFMA k-steps and
// accumulator column blocks that hold real columns: fa2_bwd_kernel.hip.h, KSN / DTN) and exports launch_bwd_hip_trim_{f16,bf16}.
#ifndef FA2_TU_TRIM
#define FA2_TU_TRIM 0
#endif
#ifndef FA2_TRIM          // 0: never dispatch to the trimmed kernels (A/B builds, tools/kbench.py)
#define FA2_TRIM 1
#endif
#ifndef FA2_BWD_FUSE256   // 0: trimmed head dims 129..224 keep the separate dV and dK sweeps (A/B builds)
#define FA2_BWD_FUSE256 1
#endif

namespace {

// (batch, K / V head) owners of the dK / dV passes: B * H / kv_group (grouped-query attention: one owner per K / V head)
int64_t kv_owners(const fa2::BwdParams& p) { return (int64_t)p.B * (p.H / p.kv_group); }

// sum of the parts a split pass left in p.ws (bwd_merge_kernel): which = 1: dQ, 2: dK and dV
template <int HD>
int merge_split_parts(const fa2::BwdParams& p, int which, hipStream_t stream) {
    if constexpr (HD <= 128) {
        fa2::BwdMergeParams m;
        m.ws = p.ws;
        m.H = which == 1 ? p.H : p.H / p.kv_group;      // the dK / dV tiles belong to K / V heads
        m.nbh = p.B * m.H; m.nblk = p.nblk; m.D = p.D;
        m.full_items = p.full_items; m.split_items = p.split_items; m.nsplit = p.nsplit;
        if (which == 1) {
            m.out[0] = p.dq; m.out[1] = nullptr; m.mul[0] = p.scale; m.mul[1] = 0.f; m.nrows = p.Nq;
            for (int i = 0; i < 3; ++i) { m.os[0][i] = p.dqs[i]; m.os[1][i] = 0; }
        } else {
            m.out[0] = p.dk; m.out[1] = p.dv; m.mul[0] = p.scale; m.mul[1] = 1.0f; m.nrows = p.Nkv;
            for (int i = 0; i < 3; ++i) { m.os[0][i] = p.dks[i]; m.os[1][i] = p.dvs[i]; }
        }
        const int64_t threads = (int64_t)p.split_items * fa2::kSplitRows * (HD / 8);
        return fa2::launch<fa2::bwd_merge_kernel<HD, kBF16>>(dim3((unsigned)((threads + 255) / 256), which == 1 ? 1 : 2), dim3(256), 0, stream, m);
    } else {
        return FA2_ERR_HEAD_DIM;
    }
}

// Which passes (fa2_pass_launch.h) run at head dims up to 256.  parts: bit 0 = the dQ pass (which also fills the delta workspace), bit 1 = the dK / dV pass(es)
template <int HD, bool CAUSAL, int KSN = HD / 16, int DTN = HD / 32>
int launch_bwd_t(const fa2::BwdParams& p0, int parts, hipStream_t stream) {
    constexpr int NW = bwd_waves(HD);          // D = 256: one wave per SIMD (512 registers), single LDS stage
    fa2::BwdParams p = p0;
    p.nsplit = 0;
    // split of a partly filled last round (fa2_bwd_ws: the caller handed over scratch memory; fa2_launch.h has the plan, which is empty for causal
    // calls and above head dim 128): the dQ pass splits its KV sweep, the fused dK / dV pass of head dims <= 64 its Q sweep
    fa2::SplitPlan sp_dq, sp_dkv;
    bwd_split_plans(HD, p, CAUSAL, &sp_dq, &sp_dkv);
    if (parts & 1) {
        // Grids that would cover at most half of the CUs with 256-row workgroups (SD-size training shapes) run as 128-row,
        // 4-wave workgroups instead — twice as many, one wave per SIMD each.
        bool dq_small = false;
        if constexpr (NW == 8) {
            const int forced = fa2::options().rows.load(std::memory_order_relaxed);      // option "rows" pins this shape too
            const int64_t w = (int64_t)p.B * p.H * ((p.Nq + 255) / 256), cus = fa2::device_cus();
            // ... and, at head dims <= 64, grids of one to one and a half rounds of 256-row workgroups (the forward's short_second_round): measured
            // (tools/bwd_rows_ab.py, whole backward) SDXL 64x64 B2 H10 N4096 428 -> 396 us, B1 H24 N3072 328 -> 300, N4096 430 -> 410, SD1.5 B3 H8 395 -> 371;
            // at exactly one round (SD1.5 B2 H8: 218 vs 229) and at D = 80 (349 vs 365) the 8-wave shape stays ahead
            dq_small = forced == 128 || (forced != 256 && (w <= cus / 2 || (HD <= 64 && w > cus && w <= cus + cus / 2)));
            if (sp_dq.nsplit > 1) dq_small = false;      // the split last round balances better than smaller workgroups
        }
        int rc = 0;
        if constexpr (NW == 8) {
            if (dq_small) rc = launch_dq<HD, CAUSAL, 4, 0, KSN, DTN>(p, NoSplit(), stream);
            else rc = launch_dq<HD, CAUSAL, NW, 0, KSN, DTN>(p, sp_dq, stream);
        } else {
            rc = launch_dq<HD, CAUSAL, NW, 0, KSN, DTN>(p, NoSplit(), stream);
        }
        if (rc) return rc;
    }
    if (!(parts & 2)) return 0;
    if constexpr (HD == 128) {
        // D in 65..128: wave pairs
        if (kv_owners(p) * ((p.Nkv + 127) / 128) > 0x7fffffffLL) return FA2_ERR_GRID;
        return launch_dkv_pair<HD, CAUSAL, KSN, DTN>(p, kv_owners(p), stream);
    } else if constexpr (HD <= 64) {
        // D <= 64: both accumulators fit one wave, one sweep forms S and P once for dK and dV
        return launch_dkv_fused<HD, CAUSAL, NW, 0, KSN, DTN>(p, kv_owners(p), sp_dkv, stream);
    } else {
#if FA2_BWD_FUSE256
        // trimmed head dims 129..224: both KV-owned accumulators (2 x DTN blocks) and the K / V fragments of KSN k-steps fit the 512-register budget
        // of one wave per SIMD, so dK and dV come from ONE sweep that forms S and dP once (4 GEMMs instead of 2 + 3, one launch less).  Measured
        // (tools/trim_ab.py --bwd --dmin 129, profiles/r08_fuse256_ab.txt, whole backward B1 H24 N4096): D 144 / 160 1 277 / 1 287 -> 1 143 / 1 142 us,
        // 176 / 192 1 490 / 1 498 -> 1 304 / 1 319, 208 / 224 1 707 / 1 771 -> 1 627 / 1 716, B1 H8 N1024 D160 115 -> 97
        if constexpr (HD == 256 && !CAUSAL && DTN <= 7)     // (causal: 11 spilled registers at 5 blocks, 100+ above; measured -5 .. -9 %)
            return launch_dkv_fused<HD, CAUSAL, NW, 0, KSN, DTN>(p, kv_owners(p), NoSplit(), stream);
#endif
        return launch_dv_dk<HD, CAUSAL, NW, 0, KSN, DTN>(p, kv_owners(p), stream);      // dV, dK: two sweeps
    }
}

// Head dims above 256 (kernel head dim 512): the slab passes
template <bool CAUSAL, int KSN = 32>
int launch_bwd_512(const fa2::BwdParams& p, int parts, hipStream_t stream) {
    return launch_bwd_slabs<CAUSAL, KSN>(p, parts, kv_owners(p), stream);
}

#if FA2_TU_TRIM

template <int HD, int KSN, int DTN>
int launch_trim(const fa2::BwdParams& p, bool causal, int parts, hipStream_t stream) {
    return causal ? launch_bwd_t<HD, true, KSN, DTN>(p, parts, stream) : launch_bwd_t<HD, false, KSN, DTN>(p, parts, stream);
}

}  // namespace

namespace fa2 {

// Trimmed backward kernels; -1 = none for this p.D (the caller runs the full kernels).  The head dims the forward trims (fwd_hip.cpp):
//   HD  64: D <= 32 -> 2 k-steps, 1 column block;   HD 128: D <= 96 -> 6, 3;   HD 256: D <= 160 / 192 / 224 -> 10, 5 / 12, 6 / 14, 7
// Measured (tools/trim_ab.py --bwd, profiles/r08_trim_ab_bwd.txt): B1 H24 N4096 D 16 / 32 +30 %, 80 / 96 +17 %, 144 / 160 +36 %, 176 / 192 +19 %, 208 / 224 +7 %.
int FA2_DT(launch_bwd_hip_trim)(int HD, const BwdParams& p, bool causal, int parts, hipStream_t stream) {
    switch (HD) {
        case 64:
            if (p.D <= 32) return launch_trim<64, 2, 1>(p, causal, parts, stream);
            return -1;      // (3 k-steps, 2 blocks for D <= 48 measured -1 .. +3 %: the fused D <= 64 pass is not bound by its MFMAs; not instantiated)
        case 128:
            if (p.D <= 80) return launch_trim<128, 5, 3>(p, causal, parts, stream);
            if (p.D <= 96) return launch_trim<128, 6, 3>(p, causal, parts, stream);
            return -1;
        case 256:
            if (p.D <= 160) return launch_trim<256, 10, 5>(p, causal, parts, stream);
            if (p.D <= 192) return launch_trim<256, 12, 6>(p, causal, parts, stream);
            if (p.D <= 224) return launch_trim<256, 14, 7>(p, causal, parts, stream);
            return -1;
        case 512:
            if (p.D <= 320) return causal ? launch_bwd_512<true, 20>(p, parts, stream) : launch_bwd_512<false, 20>(p, parts, stream);
            if (p.D <= 384) return causal ? launch_bwd_512<true, 24>(p, parts, stream) : launch_bwd_512<false, 24>(p, parts, stream);
            if (p.D <= 448) return causal ? launch_bwd_512<true, 28>(p, parts, stream) : launch_bwd_512<false, 28>(p, parts, stream);
            return -1;
        default: return -1;
    }
}

}  // namespace fa2

#else   // !FA2_TU_TRIM

// dQ pass of KV sweeps of at most two tiles (fa2_bwd_short.hip.h): 128-row workgroups; one instantiation per count of 32-key blocks that hold a key
template <int HD, int NB>
int launch_short_dq_nb(const fa2::BwdParams& p, bool neg_delta, hipStream_t stream) {
    return fa2::launch<fa2::bwd_short_dq_kernel<HD, kBF16, NB>>(dim3((unsigned)((int64_t)p.B * p.H * p.nblk)), dim3(256), fa2::bwd_short_lds_bytes<HD>(NB), stream, p,
                                                                  (int)neg_delta);
}

template <int HD>
int launch_short_dq(const fa2::BwdParams& p0, bool neg_delta, hipStream_t stream) {
    fa2::BwdParams p = p0;
    p.nblk = (p.Nq + fa2::kBwdShortRows - 1) / fa2::kBwdShortRows;
    if ((int64_t)p.B * p.H * p.nblk > 0x7fffffffLL) return FA2_ERR_GRID;
    p.nsplit = 0;
    switch ((p.Nkv + 31) / 32) {
        case 1: return launch_short_dq_nb<HD, 1>(p, neg_delta, stream);
        case 2: return launch_short_dq_nb<HD, 2>(p, neg_delta, stream);
        case 3: return launch_short_dq_nb<HD, 3>(p, neg_delta, stream);
        case 4: return launch_short_dq_nb<HD, 4>(p, neg_delta, stream);
        default: return FA2_ERR_BAD_SHAPE;
    }
}

template <int HD>
int launch_bwd(const fa2::BwdParams& p, bool causal, int parts, hipStream_t stream) {
    return causal ? launch_bwd_t<HD, true>(p, parts, stream) : launch_bwd_t<HD, false>(p, parts, stream);
}

}  // namespace

namespace fa2 {

int FA2_DT(launch_bwd_hip)(int HD, const BwdParams& p, bool causal, int parts, hipStream_t stream) {
    if (FA2_TRIM && p.D < HD) {      // a trimmed instantiation, where one exists
        const int rc = FA2_DT(launch_bwd_hip_trim)(HD, p, causal, parts, stream);
        if (rc >= 0) return rc;
    }
    switch (HD) {
        case 64: return launch_bwd<64>(p, causal, parts, stream);
        case 128: return launch_bwd<128>(p, causal, parts, stream);
        case 256: return launch_bwd<256>(p, causal, parts, stream);
        case 512: return causal ? launch_bwd_512<true>(p, parts, stream) : launch_bwd_512<false>(p, parts, stream);
        default: return FA2_ERR_HEAD_DIM;
    }
}

int FA2_DT(launch_bwd_short_dq)(int HD, const BwdParams& p, bool neg_delta, hipStream_t stream) {
    return HD == 64 ? launch_short_dq<64>(p, neg_delta, stream) : HD == 128 ? launch_short_dq<128>(p, neg_delta, stream) : FA2_ERR_HEAD_DIM;
}

int FA2_DT(launch_bwd_merge)(int HD, const BwdParams& p, int which, hipStream_t stream) {
    return HD == 64 ? merge_split_parts<64>(p, which, stream) : HD == 128 ? merge_split_parts<128>(p, which, stream) : FA2_ERR_HEAD_DIM;
}

}  // namespace fa2

#endif  // FA2_TU_TRIM
