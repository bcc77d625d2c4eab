// fa2_family_unit.h — the body of a kernel-family unit for ONE dtype.  A family is a form of the compiler-scheduled forward kernel (fa2_fwd_kernel.hip.h)
// and backward passes (fa2_bwd_kernel.hip.h), compiled under names of its own next to the plain instantiations:
//     window_hip.cpp  FA2_WIN                 varlen_hip.cpp          + FA2_VARLEN
//     dropout_hip.cpp FA2_WIN + FA2_DROP      varlen_dropout_hip.cpp  + FA2_VARLEN
//     scoremod_hip.cpp FA2_WIN + FA2_SMOD     varlen_scoremod_hip.cpp + FA2_VARLEN
// Each of those files sets its form macros and FA2_FAMILY (window, varlen, ...) and includes this one; build.py compiles it twice (-DFA2_TU_BF16=0 / 1).
// The kernel headers compile their blocks under the form macros (preprocessor blocks: every other translation unit sees the text it always saw, so its
// code cannot change).  From FA2_FAMILY come the kernels' names — fwd_<family>_kernel, bwd_<family>_dq_kernel, bwd_<family>_dkv_kernel,
// bwd_<family>_dkv_pair_kernel, so that they never collide with the plain instantiations — and the exported launch_fwd_<family>_<dt> / launch_bwd_<family>_<dt>.
// The families' kernels are non-causal instantiations: host.cpp folds the causal flag into the window (right = 0) before it gets here; the packed forms
// are launched exactly like the dense ones (the host passes the stated maximum lengths as Nq / Nkv, which size the grids).
// No trimmed instantiations, no KV-split, no hand-scheduled bodies: every head dim runs the full kernel of its padded head dim.
// FA2_FAMILY_FWD_ONLY = 1 (prefill_hip.cpp, prefill_scoremod_hip.cpp: an inference call has no backward): the unit compiles and exports the forward alone.
// FA2_FAMILY_MAX_HD (prefill_fp8_hip.cpp, prefill_fp8_scoremod_hip.cpp): the largest kernel head dim the unit instantiates; above it the launcher answers
// FA2_ERR_HEAD_DIM (an instantiation that would need scratch memory is not compiled).  Default: all four.
#ifndef FA2_FAMILY
#error "define FA2_FAMILY (and the family's form macros) before including fa2_family_unit.h"
#endif
#define FA2_FAMILY_NAME_(a, f, b) a##f##b
#define FA2_FAMILY_NAME(a, f, b) FA2_FAMILY_NAME_(a, f, b)
#define fwd_kernel FA2_FAMILY_NAME(fwd_, FA2_FAMILY, _kernel)
#define bwd_dq_kernel FA2_FAMILY_NAME(bwd_, FA2_FAMILY, _dq_kernel)
#define bwd_dkv_kernel FA2_FAMILY_NAME(bwd_, FA2_FAMILY, _dkv_kernel)
#define bwd_dkv_pair_kernel FA2_FAMILY_NAME(bwd_, FA2_FAMILY, _dkv_pair_kernel)
#include "fa2_pass_launch.h"

#ifndef FA2_FAMILY_FWD_ONLY
#define FA2_FAMILY_FWD_ONLY 0
#endif
#ifndef FA2_FAMILY_MAX_HD
#define FA2_FAMILY_MAX_HD 512
#endif

// The FA2_PAGED kernels take one further argument, the PagedKv block (fa2_prefill.h), the FA2_KV8 kernels the KvDescale block behind it, and the FA2_SMOD
// kernels the ScoreMod block (fa2_scoremod.h), in this order; the launchers pass them through.  Elsewhere the macros are empty.
#if FA2_PAGED
#define FA2_FAMILY_PAGED_PARAMS , const fa2::PagedKv& pg
#define FA2_FAMILY_PAGED_ARGS , pg
#else
#define FA2_FAMILY_PAGED_PARAMS
#define FA2_FAMILY_PAGED_ARGS
#endif
#if FA2_KV8
#define FA2_FAMILY_KV8_PARAMS , const fa2::KvDescale& kvd
#define FA2_FAMILY_KV8_ARGS , kvd
#else
#define FA2_FAMILY_KV8_PARAMS
#define FA2_FAMILY_KV8_ARGS
#endif
#if FA2_SMOD
#define FA2_FAMILY_SMOD_PARAMS , const fa2::ScoreMod& sm
#define FA2_FAMILY_SMOD_ARGS , sm
#else
#define FA2_FAMILY_SMOD_PARAMS
#define FA2_FAMILY_SMOD_ARGS
#endif
#define FA2_FAMILY_MORE_PARAMS FA2_FAMILY_PAGED_PARAMS FA2_FAMILY_KV8_PARAMS FA2_FAMILY_SMOD_PARAMS
#define FA2_FAMILY_MORE_ARGS FA2_FAMILY_PAGED_ARGS FA2_FAMILY_KV8_ARGS FA2_FAMILY_SMOD_ARGS

namespace {

template <int HD>
int launch_fwd_hd(const fa2::FwdParams& p0, int rows, hipStream_t stream FA2_FAMILY_MORE_PARAMS) {
    fa2::FwdParams p = p0;
    p.nsplit = 0;
    // (FA2_PAGED: 128-row workgroups at every head dim above 128 — the 256-row instantiation of head dim 256 spills to scratch memory, the 128-row one does not)
    if constexpr (HD > (FA2_PAGED ? 128 : 256)) return launch_fwd_shape<HD, false, 4>(p, stream FA2_FAMILY_MORE_ARGS);
    else return rows == 128 ? launch_fwd_shape<HD, false, 4>(p, stream FA2_FAMILY_MORE_ARGS) : launch_fwd_shape<HD, false, 8>(p, stream FA2_FAMILY_MORE_ARGS);
}

#if !FA2_FAMILY_FWD_ONLY
// The backward: dQ pass, then dK and dV — fused at head dims <= 64, wave pairs at 128, separate sweeps at 256, slabs at 512 (bwd_hip.cpp has the
// reasons for each shape).  kv_group == 1: the operator expands grouped K / V and sums the gradients per group.
template <int HD>
int launch_bwd_hd(const fa2::BwdParams& p0, hipStream_t stream FA2_FAMILY_MORE_PARAMS) {
    constexpr int NW = bwd_waves(HD);
    fa2::BwdParams p = p0;
    p.nsplit = 0;
    const int64_t owners = (int64_t)p.B * p.H;
    if (owners * ((p.Nq + 127) / 128) > 0x7fffffffLL || owners * ((p.Nkv + 127) / 128) > 0x7fffffffLL) return FA2_ERR_GRID;
    if constexpr (HD > 256) {
        return launch_bwd_slabs<false>(p, 3, owners, stream FA2_FAMILY_MORE_ARGS);
    } else {
        if (int rc = launch_dq<HD, false, NW>(p, NoSplit(), stream FA2_FAMILY_MORE_ARGS)) return rc;
        if constexpr (HD <= 64) return launch_dkv_fused<HD, false, NW>(p, owners, NoSplit(), stream FA2_FAMILY_MORE_ARGS);
        else if constexpr (HD == 128) return launch_dkv_pair<HD, false>(p, owners, stream FA2_FAMILY_MORE_ARGS);
        else return launch_dv_dk<HD, false, NW>(p, owners, stream FA2_FAMILY_MORE_ARGS);
    }
}
#endif

}  // namespace

namespace fa2 {

int FA2_DT(FA2_FAMILY_NAME(launch_fwd_, FA2_FAMILY, ))(int HD, const FwdParams& p, int rows, hipStream_t stream FA2_FAMILY_MORE_PARAMS) {
    switch (HD) {
        case 64: return launch_fwd_hd<64>(p, rows, stream FA2_FAMILY_MORE_ARGS);
        case 128: return launch_fwd_hd<128>(p, rows, stream FA2_FAMILY_MORE_ARGS);
#if FA2_FAMILY_MAX_HD >= 256
        case 256: return launch_fwd_hd<256>(p, rows, stream FA2_FAMILY_MORE_ARGS);
#endif
#if FA2_FAMILY_MAX_HD >= 512
        case 512: return launch_fwd_hd<512>(p, rows, stream FA2_FAMILY_MORE_ARGS);
#endif
        default: return FA2_ERR_HEAD_DIM;
    }
}

#if !FA2_FAMILY_FWD_ONLY
int FA2_DT(FA2_FAMILY_NAME(launch_bwd_, FA2_FAMILY, ))(int HD, const BwdParams& p, hipStream_t stream FA2_FAMILY_MORE_PARAMS) {
    switch (HD) {
        case 64: return launch_bwd_hd<64>(p, stream FA2_FAMILY_MORE_ARGS);
        case 128: return launch_bwd_hd<128>(p, stream FA2_FAMILY_MORE_ARGS);
        case 256: return launch_bwd_hd<256>(p, stream FA2_FAMILY_MORE_ARGS);
        case 512: return launch_bwd_hd<512>(p, stream FA2_FAMILY_MORE_ARGS);
        default: return FA2_ERR_HEAD_DIM;
    }
}
#endif

}  // namespace fa2
