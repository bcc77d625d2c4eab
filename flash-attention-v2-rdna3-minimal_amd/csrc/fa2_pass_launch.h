// fa2_pass_launch.h — the passes of the compiler-scheduled kernels (fa2_fwd_kernel.hip.h, fa2_bwd_kernel.hip.h) as launches, written once for the per-dtype
// units that run them: fwd_hip.cpp, bwd_hip.cpp, bwd_bias_hip.cpp and the six family units (fa2_family_unit.h).  Host-only code: every pass names its
// kernel, its grid and its LDS size in one place; WHICH passes run for a head dim, and when, stays with the units.
// Everything here has internal linkage: a unit compiles these templates against its own dtype and, in the family units, its own kernel names.
#pragma once
#include "fa2_launch.h"

#include "fa2_gfx950.h"

#ifndef FA2_TU_BF16
#error "compile with -DFA2_TU_BF16=0 or 1"
#endif

namespace {

constexpr bool kBF16 = FA2_TU_BF16 != 0;

// ---- forward: NW waves of 32 rows per workgroup, 128-column slabs of O at head dims above 128 (grid.y).  KSQ / DTN / RTD / HDV_: the trimmed
// instantiations (fwd_hip.cpp); more: further kernel arguments (the ScoreMod block of the FA2_SMOD kernels)
template <int HD, bool CAUSAL, int NW, int BIAS = 0, int KSQ = HD / 16, int DTN = (HD > 128 ? 128 : HD) / 32, bool RTD = false, int HDV_ = 0, class... More>
int launch_fwd_shape(const fa2::FwdParams& p0, hipStream_t stream, const More&... more) {
    constexpr int HDV = HDV_ ? HDV_ : HD > 128 ? 128 : HD;       // (HDV_ = 256: one pass over all columns, trimmed head dims 129..192 only)
    constexpr int lds_kv = 2 * fa2::Geo<HD, NW>::TILEB + 2 * fa2::Geo<HDV, NW>::TILEB;
    constexpr int lds_epi = FA2_EPI_LDS ? NW * 32 * (HDV * 2 + 16) : 0;     // epilogue image (reuses the K/V space)
    // bias kernels: + NW wave-private 32-row images of the "tile" bias form where they fit (not at D = 512: 160 KiB of K / V buffers)
    // (BIAS = 2, the LDS-DMA form: NW images of 8 KiB)
    constexpr int lds_bias = BIAS == 2 ? NW * 8192 : BIAS && lds_kv + NW * 32 * 272 <= 160 * 1024 ? NW * 32 * 272 : 0;
    constexpr int lds = lds_kv + lds_bias > lds_epi ? lds_kv + lds_bias : lds_epi;
    static_assert(lds <= 160 * 1024, "LDS budget");
    fa2::FwdParams p = p0;
    p.nqblk = (p.Nq + NW * 32 - 1) / (NW * 32);
    if ((int64_t)p.nbh * p.nqblk > 0x7fffffffLL) return FA2_ERR_GRID;
    int64_t nblk = (int64_t)p.nbh * p.nqblk;
    if constexpr (NW == 8 && !BIAS && !CAUSAL && HD == HDV) {
        // KV-split tail (host.cpp: plan_split): the whole items from blk0 on, then split_items * nsplit parts
        if (p.nsplit > 1) nblk = (int64_t)p.full_items - p.blk0 + (int64_t)p.split_items * p.nsplit;
    } else {
        p.nsplit = 0;
    }
    const dim3 grid((unsigned)nblk, (p.D + HDV - 1) / HDV);      // column slabs that hold real columns (HD / HDV of them at most)
    return fa2::launch<fa2::fwd_kernel<HD, HDV, kBF16, CAUSAL, NW, 1, BIAS, KSQ, DTN, RTD>>(grid, dim3(NW * 64), lds, stream, p, more...);
}

// ---- backward.  A pass takes the parameter block BY VALUE: what it fills in (nblk, the split fields) never reaches the next pass.
// HD <= 128: two LDS stages, 8 waves of 32 rows (the dQ pass of a small grid: 4); above: one stage, 4 waves — one per SIMD with the 512-register budget.
constexpr int bwd_waves(int HD) { return HD > 128 ? 4 : 8; }
constexpr int bwd_stages(int HD) { return HD > 128 ? 1 : 2; }
template <int HD, int NW> constexpr int lds_dq() { return bwd_stages(HD) * 3 * fa2::Geo<HD, NW>::TILEB; }
template <int HD, int NW> constexpr int lds_dkv_fused() { return bwd_stages(HD) * (4 * fa2::Geo<HD, NW>::TILEB + 512); }
template <int HD, int NW> constexpr int lds_dv() { return bwd_stages(HD) * (2 * fa2::Geo<HD, NW>::TILEB + 512); }
template <int HD, int NW> constexpr int lds_dk() { return bwd_stages(HD) * (3 * fa2::Geo<HD, NW>::TILEB + 512); }
template <int HD> constexpr int lds_dkv_pair() { return 2 * (4 * fa2::Geo<HD, 8>::TILEB + 512) + 4 * 4096; }
// the slab passes of head dims above 256: the whole head dim of the contracted operands, one HDV-column slab of the others
template <int HD, int HDV, int NW> constexpr int lds_slab_dq() { return 2 * fa2::Geo<HD, NW>::TILEB + fa2::Geo<HDV, NW>::TILEB; }
template <int HD, int HDV, int NW> constexpr int lds_slab_dv() { return fa2::Geo<HD, NW>::TILEB + fa2::Geo<HDV, NW>::TILEB + 512; }
template <int HD, int HDV, int NW> constexpr int lds_slab_dk() { return 2 * fa2::Geo<HD, NW>::TILEB + fa2::Geo<HDV, NW>::TILEB + 512; }

// FORM 0: the pass's own size.  The BIAS forms stage NW wave-private bias images above it where the call has tiles (p.bias_tile, host.cpp), so their
// size varies per call: the kernels are opted in once with all 160 KiB.
template <int NW, int FORM>
fa2::LdsBytes bwd_pass_lds(int base, const fa2::BwdParams& p) {
    if constexpr (FORM == 0) return base;
    else return fa2::LdsBytes(base + (p.bias_tile ? NW * p.bias_img : 0), 160 * 1024);
}

// Split passes (fa2_launch.h: plan_bwd_split).  The plans a call may use: none without 16-byte aligned scratch memory, none that p.ws_bytes cannot hold.
inline void bwd_split_plans(int HD, const fa2::BwdParams& p, bool causal, fa2::SplitPlan* dq, fa2::SplitPlan* dkv) {
    *dq = *dkv = fa2::SplitPlan();
    if (!p.ws || (reinterpret_cast<uintptr_t>(p.ws) & 15u) != 0) return;
    fa2::plan_bwd_split(HD, p, causal, dq, dkv);
    if ((size_t)dq->bytes > p.ws_bytes) *dq = fa2::SplitPlan();
    if ((size_t)dkv->bytes > p.ws_bytes) *dkv = fa2::SplitPlan();
}
// A pass of `items` workgroups under a plan: the plan goes into the parameter block, the grid is the whole items and then split_items * nsplit parts;
// afterwards the parts are summed (merge_split_parts: defined by the unit — bwd_hip.cpp holds the kernel, bwd_bias_hip.cpp calls its exported launcher).
// NoSplit: a pass that never splits (the family units), which needs neither.
struct NoSplit {};
template <int HD>
int merge_split_parts(const fa2::BwdParams& p, int which, hipStream_t stream);
inline int64_t apply_split(fa2::BwdParams&, NoSplit, int64_t items) { return items; }
inline int64_t apply_split(fa2::BwdParams& p, const fa2::SplitPlan& sp, int64_t items) {
    if (sp.nsplit <= 1) return items;
    p.full_items = sp.full_items; p.split_items = sp.split_items; p.nsplit = sp.nsplit;
    return (int64_t)p.full_items + (int64_t)p.split_items * p.nsplit;
}
template <int HD>
int merge_if_split(const fa2::BwdParams&, NoSplit, int, hipStream_t) { return 0; }
template <int HD>
int merge_if_split(const fa2::BwdParams& p, const fa2::SplitPlan&, int which, hipStream_t stream) {
    return p.nsplit > 1 ? merge_split_parts<HD>(p, which, stream) : 0;
}

// dQ (which also writes D_i = rowsum(dO * O) to the delta workspace): one workgroup per NW * 32 Q rows
template <int HD, bool CAUSAL, int NW, int FORM = 0, int KSN = HD / 16, int DTN = HD / 32, class Split, class... More>
int launch_dq(fa2::BwdParams p, Split sp, hipStream_t stream, const More&... more) {
    const fa2::LdsBytes lds = bwd_pass_lds<NW, FORM>(lds_dq<HD, NW>(), p);
    if (lds.launch > 160 * 1024) return FA2_ERR_BAD_SHAPE;      // unreachable: bwd_bias_hip.cpp picks FORM 2 only where the largest pass fits with the images
    p.nblk = (p.Nq + NW * 32 - 1) / (NW * 32);
    const int64_t grid = apply_split(p, sp, (int64_t)p.B * p.H * p.nblk);
    if (int rc = fa2::launch<fa2::bwd_dq_kernel<HD, kBF16, CAUSAL, NW, HD, FORM, KSN, DTN>>(dim3((unsigned)grid), dim3(NW * 64), lds, stream, p, more...)) return rc;
    return merge_if_split<HD>(p, sp, 1, stream);
}

// The dK / dV passes: one workgroup per NW * 32 KV rows of each of the `owners` (batch, K / V head) pairs.
// dK and dV in ONE sweep that forms S and P once: both accumulators fit one wave (head dims <= 64; trimmed head dims 129..224)
template <int HD, bool CAUSAL, int NW, int FORM = 0, int KSN = HD / 16, int DTN = HD / 32, class Split, class... More>
int launch_dkv_fused(fa2::BwdParams p, int64_t owners, Split sp, hipStream_t stream, const More&... more) {
    static_assert(lds_dkv_fused<HD, NW>() <= 160 * 1024, "LDS budget");
    const fa2::LdsBytes lds = bwd_pass_lds<NW, FORM>(lds_dkv_fused<HD, NW>(), p);
    if (lds.launch > 160 * 1024) return FA2_ERR_BAD_SHAPE;      // unreachable, as above
    p.nblk = (p.Nkv + NW * 32 - 1) / (NW * 32);
    const int64_t grid = apply_split(p, sp, owners * p.nblk);
    if (int rc = fa2::launch<fa2::bwd_dkv_kernel<HD, kBF16, CAUSAL, true, NW, true, HD, FORM, KSN, DTN>>(dim3((unsigned)grid), dim3(NW * 64), lds, stream, p, more...))
        return rc;
    return merge_if_split<HD>(p, sp, 2, stream);
}

// a dV sweep, then a dK sweep
template <int HD, bool CAUSAL, int NW, int FORM = 0, int KSN = HD / 16, int DTN = HD / 32, class... More>
int launch_dv_dk(fa2::BwdParams p, int64_t owners, hipStream_t stream, const More&... more) {
    p.nblk = (p.Nkv + NW * 32 - 1) / (NW * 32);
    const dim3 grid((unsigned)(owners * p.nblk));
    const fa2::LdsBytes lds_v = bwd_pass_lds<NW, FORM>(lds_dv<HD, NW>(), p), lds_k = bwd_pass_lds<NW, FORM>(lds_dk<HD, NW>(), p);
    if (lds_v.launch > 160 * 1024) return FA2_ERR_BAD_SHAPE;      // unreachable, as above
    if (int rc = fa2::launch<fa2::bwd_dkv_kernel<HD, kBF16, CAUSAL, false, NW, false, HD, FORM, KSN, DTN>>(grid, dim3(NW * 64), lds_v, stream, p, more...)) return rc;
    if (lds_k.launch > 160 * 1024) return FA2_ERR_BAD_SHAPE;
    return fa2::launch<fa2::bwd_dkv_kernel<HD, kBF16, CAUSAL, true, NW, false, HD, FORM, KSN, DTN>>(grid, dim3(NW * 64), lds_k, stream, p, more...);
}

// D in 65..128: dK and dV in one sweep by wave pairs (bwd_dkv_pair_kernel): 128 KV rows per workgroup of 8 waves, S and P formed once
template <int HD, bool CAUSAL, int KSN = HD / 16, int DTN = HD / 32, class... More>
int launch_dkv_pair(fa2::BwdParams p, int64_t owners, hipStream_t stream, const More&... more) {
    p.nblk = (p.Nkv + 127) / 128;
    return fa2::launch<fa2::bwd_dkv_pair_kernel<HD, kBF16, CAUSAL, KSN, DTN>>(dim3((unsigned)(owners * p.nblk)), dim3(512), lds_dkv_pair<HD>(), stream, p, more...);
}

// Head dims above 256 (kernel head dim 512, the SD VAE attention block): 4-wave workgroups of 128 rows, one wave per SIMD with the 512-register
// budget, single LDS stage; every workgroup produces a 128-column slab of its output (grid.y: only the slabs that hold real columns) and recomputes
// S (and dP) over the whole head dim.  Three launches: dQ (+ delta), dV, dK.  A correct path for a rare shape, not a tuned one.
// parts: bit 0 = dQ, bit 1 = dV and dK.  KSN (trimmed instantiations): ceil(D / 16) k-steps of the products contracted over the head dim.
template <bool CAUSAL, int KSN = 32, class... More>
int launch_bwd_slabs(fa2::BwdParams p, int parts, int64_t owners, hipStream_t stream, const More&... more) {
    constexpr int HD = 512, HDV = 128, NW = 4, kRows = NW * 32;
    const unsigned slabs = (unsigned)((p.D + HDV - 1) / HDV);
    if (parts & 1) {
        p.nblk = (p.Nq + kRows - 1) / kRows;
        if (int rc = fa2::launch<fa2::bwd_dq_kernel<HD, kBF16, CAUSAL, NW, HDV, 0, KSN, HDV / 32>>(dim3((unsigned)((int64_t)p.B * p.H * p.nblk), slabs), dim3(NW * 64),
                                                                                                 lds_slab_dq<HD, HDV, NW>(), stream, p, more...))
            return rc;
    }
    if (!(parts & 2)) return 0;
    p.nblk = (p.Nkv + kRows - 1) / kRows;
    const dim3 grid((unsigned)(owners * p.nblk), slabs);
    if (int rc = fa2::launch<fa2::bwd_dkv_kernel<HD, kBF16, CAUSAL, false, NW, false, HDV, 0, KSN, HDV / 32>>(grid, dim3(NW * 64), lds_slab_dv<HD, HDV, NW>(), stream, p, more...))
        return rc;
    return fa2::launch<fa2::bwd_dkv_kernel<HD, kBF16, CAUSAL, true, NW, false, HDV, 0, KSN, HDV / 32>>(grid, dim3(NW * 64), lds_slab_dk<HD, HDV, NW>(), stream, p, more...);
}

}  // namespace
