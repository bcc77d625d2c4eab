// bwd_bias_hip.cpp — backward through a biased / masked forward (fa2_bwd_bias) for ONE dtype: the BIAS instantiations of the
// compiler-scheduled passes (fa2_bwd_kernel.hip.h): dQ, then dK and dV in one sweep at head dims <= 64, dV and dK above.  build.py compiles this file twice (-DFA2_TU_BF16=0 / 1).
// The passes themselves are fa2_pass_launch.h's (the BIAS forms add the bias images to a pass's LDS size); this file picks the FORM and the dK / dV shape.
// The reference has no counterpart: its `mask` argument is accepted and ignored (FlashAttn.py:49, :74; README.md:45 "to do").
#include "fa2_pass_launch.h"

namespace {

// the split passes' parts are summed by bwd_hip.cpp's kernel
template <int HD>
int merge_split_parts(const fa2::BwdParams& p, int which, hipStream_t stream) { return fa2::FA2_DT(launch_bwd_merge)(HD, p, which, stream); }

// The passes (fa2_pass_launch.h) of one bias FORM: dQ, then dK and dV in one sweep at head dims <= 64, a dV and a dK sweep above (also at head dim 128)
template <int HD, bool CAUSAL, int FORM>
int launch_form(const fa2::BwdParams& p0, hipStream_t stream) {
    constexpr int NW = bwd_waves(HD);          // D = 256: one wave per SIMD (512 registers), single LDS stage
    fa2::BwdParams p = p0;
    p.nsplit = 0;
    // split of a partly filled last round / of an underfilled KV-owner grid (fa2_bwd_bias_ws: scratch memory from the caller), as in bwd_hip.cpp
    fa2::SplitPlan sp_dq, sp_dkv;
    if constexpr (!CAUSAL && NW == 8) bwd_split_plans(HD, p, CAUSAL, &sp_dq, &sp_dkv);
    const int64_t owners = (int64_t)p.B * p.H;
    if (int rc = launch_dq<HD, CAUSAL, NW, FORM == 3 ? 1 : FORM>(p, sp_dq, stream)) return rc;      // (the dQ pass has no per-row form: one load per score)
    // both accumulators fit one wave: dK and dV in ONE sweep (S, the bias and P formed once), like the unmasked backward
    // (with one load per score, FORM 1, the fused pass spills: two sweeps as above 64)
    if constexpr (HD <= 64 && FORM != 1) return launch_dkv_fused<HD, CAUSAL, NW, FORM>(p, owners, sp_dkv, stream);
    else return launch_dv_dk<HD, CAUSAL, NW, FORM>(p, owners, stream);
}

// FORM 2: bias tiles by LDS-DMA where the geometry allows and the images fit the LDS; FORM 1: one guarded load per score; FORM 3: one per KV row
template <int HD, bool CAUSAL>
int launch_t(fa2::BwdParams p, hipStream_t stream) {
    constexpr int NW = bwd_waves(HD);
    // bias tiles staged by LDS-DMA (p.bias_tile, host.cpp): NW wave-private images above the stages, where the largest pass fits the 160 KiB with them
    if (p.bias_tile && (HD <= 64 ? lds_dkv_fused<HD, NW>() : lds_dk<HD, NW>()) + NW * p.bias_img <= 160 * 1024) return launch_form<HD, CAUSAL, 2>(p, stream);
    p.bias_tile = 0;
    // a bias broadcast over the Q rows (a [B, 1, 1, Nkv] key-padding mask): the dK / dV pass loads its lanes' values once (FORM 3)
    if constexpr (HD <= 128) {
        if (p.bs[2] == 0) return launch_form<HD, CAUSAL, 3>(p, stream);
    }
    return launch_form<HD, CAUSAL, 1>(p, stream);
}

template <int HD>
int launch_hd(const fa2::BwdParams& p, bool causal, hipStream_t stream) {
    return causal ? launch_t<HD, true>(p, stream) : launch_t<HD, false>(p, stream);
}

}  // namespace

namespace fa2 {

int FA2_DT(launch_bwd_bias_hip)(int HD, const BwdParams& p, bool causal, hipStream_t stream) {
    switch (HD) {
        case 64: return launch_hd<64>(p, causal, stream);
        case 128: return launch_hd<128>(p, causal, stream);
        case 256: return launch_hd<256>(p, causal, stream);
        default: return FA2_ERR_HEAD_DIM;       // (the slab kernels of head dims above 256 have no bias form)
    }
}

}  // namespace fa2
