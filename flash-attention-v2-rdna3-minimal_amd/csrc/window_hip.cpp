// window_hip.cpp — sliding-window (local) attention for ONE dtype: the FA2_WIN forms of the compiler-scheduled forward kernel
// (fa2_fwd_kernel.hip.h) and backward passes (fa2_bwd_kernel.hip.h), and their launchers.  build.py compiles this file twice
// (-DFA2_TU_BF16=0 / 1), in parallel with the other translation units.  The range arithmetic is fa2_window.h's.
// The windowed kernels are non-causal instantiations: host.cpp folds the causal flag into the window (right = 0) before it gets here.
// No trimmed instantiations, no KV-split, no hand-scheduled bodies: every head dim runs the full kernel of its padded head dim.
// The kernel headers compile their sliding-window blocks under FA2_WIN (preprocessor blocks: every other translation unit sees the text it always
// saw, so its code cannot change), and the kernels get names of their own here so that they never collide with the plain instantiations.
// varlen_hip.cpp includes this file under FA2_VARLEN with kernel and launcher names of its own: the packed forms are launched exactly like these (the
// host passes the stated maximum lengths as Nq / Nkv, which size the grids).
#ifndef FA2_VARLEN
#define FA2_WIN 1
#define fwd_kernel fwd_window_kernel
#define bwd_dq_kernel bwd_window_dq_kernel
#define bwd_dkv_kernel bwd_window_dkv_kernel
#define bwd_dkv_pair_kernel bwd_window_dkv_pair_kernel
#define FA2_WIN_LAUNCH(pass, dt) launch_##pass##_window_##dt
#endif
#include "fa2_launch.h"

#include "fa2_gfx950.h"

#ifndef FA2_TU_BF16
#error "compile with -DFA2_TU_BF16=0 or 1"
#endif

// scoremod_hip.cpp / varlen_scoremod_hip.cpp include this file under FA2_SMOD: their kernels take one further argument (fa2_scoremod.h), which the
// launchers pass through.  Everywhere else both macros are empty.
#if FA2_SMOD
#define FA2_WIN_MORE_PARAMS , const fa2::ScoreMod& sm
#define FA2_WIN_MORE_ARGS , sm
#else
#define FA2_WIN_MORE_PARAMS
#define FA2_WIN_MORE_ARGS
#endif

namespace {

constexpr bool kBF16 = FA2_TU_BF16 != 0;

template <int HD, int NW>
int launch_fwd_shape(const fa2::FwdParams& p0, hipStream_t stream FA2_WIN_MORE_PARAMS) {
    constexpr int HDV = HD > 128 ? 128 : HD;                     // D = 256 / 512: 128-column slabs of O (grid.y), as the plain kernels
    constexpr int lds_kv = 2 * fa2::Geo<HD, NW>::TILEB + 2 * fa2::Geo<HDV, NW>::TILEB;
    constexpr int lds_epi = FA2_EPI_LDS ? NW * 32 * (HDV * 2 + 16) : 0;
    constexpr int lds = lds_kv > lds_epi ? lds_kv : lds_epi;
    static_assert(lds <= 160 * 1024, "LDS budget");
    fa2::FwdParams p = p0;
    p.nqblk = (p.Nq + NW * 32 - 1) / (NW * 32);
    p.nsplit = 0;
    const int64_t nblk = (int64_t)p.nbh * p.nqblk;
    if (nblk > 0x7fffffffLL) return FA2_ERR_GRID;
    const dim3 grid((unsigned)nblk, (p.D + HDV - 1) / HDV);
    constexpr auto kern = fa2::fwd_kernel<HD, HDV, kBF16, false, NW, 1, 0, HD / 16, HDV / 32, false>;
    if (int rc = fa2::set_lds<kern>(lds)) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(NW * 64), lds, stream, p FA2_WIN_MORE_ARGS);
    return (int)hipGetLastError();
}

template <int HD>
int launch_fwd_hd(const fa2::FwdParams& p, int rows, hipStream_t stream FA2_WIN_MORE_PARAMS) {
    if constexpr (HD > 256) return launch_fwd_shape<HD, 4>(p, stream FA2_WIN_MORE_ARGS);
    else return rows == 128 ? launch_fwd_shape<HD, 4>(p, stream FA2_WIN_MORE_ARGS) : launch_fwd_shape<HD, 8>(p, stream FA2_WIN_MORE_ARGS);
}

// The backward: dQ pass, then dK and dV — fused at head dims <= 64, wave pairs at 128, separate sweeps at 256, slabs at 512 (bwd_hip.cpp has the
// unwindowed twins and the reasons for each shape).  kv_group == 1: the operator expands grouped K / V and sums the gradients per group.
template <int HD>
int launch_bwd_hd(fa2::BwdParams p, hipStream_t stream FA2_WIN_MORE_PARAMS) {
    constexpr int NW = HD > 128 ? 4 : 8;
    constexpr int kRows = NW * 32, kStages = NW == 8 ? 2 : 1;
    constexpr int TILEB = fa2::Geo<HD, NW>::TILEB;
    int rc;
    p.nsplit = 0;
    if ((int64_t)p.B * p.H * ((p.Nq + 127) / 128) > 0x7fffffffLL || (int64_t)p.B * p.H * ((p.Nkv + 127) / 128) > 0x7fffffffLL) return FA2_ERR_GRID;
    if constexpr (HD <= 256) {
        constexpr int lds = kStages * 3 * TILEB;
        constexpr auto kern = fa2::bwd_dq_kernel<HD, kBF16, false, NW, HD, 0, HD / 16, HD / 32>;
        if ((rc = fa2::set_lds<kern>(lds))) return rc;
        p.nblk = (p.Nq + kRows - 1) / kRows;
        hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)p.B * p.H * p.nblk)), dim3(NW * 64), lds, stream, p FA2_WIN_MORE_ARGS);
        if ((rc = (int)hipGetLastError())) return rc;
    }
    if constexpr (HD <= 64) {
        p.nblk = (p.Nkv + kRows - 1) / kRows;
        constexpr int lds = kStages * (4 * TILEB + 512);
        constexpr auto kern = fa2::bwd_dkv_kernel<HD, kBF16, false, true, NW, true, HD, 0, HD / 16, HD / 32>;
        if ((rc = fa2::set_lds<kern>(lds))) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)p.B * p.H * p.nblk)), dim3(NW * 64), lds, stream, p FA2_WIN_MORE_ARGS);
        return (int)hipGetLastError();
    } else if constexpr (HD == 128) {
        p.nblk = (p.Nkv + 127) / 128;
        constexpr int lds = 2 * (4 * TILEB + 512) + 4 * 4096;
        constexpr auto kern = fa2::bwd_dkv_pair_kernel<HD, kBF16, false, HD / 16, HD / 32>;
        if ((rc = fa2::set_lds<kern>(lds))) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)p.B * p.H * p.nblk)), dim3(512), lds, stream, p FA2_WIN_MORE_ARGS);
        return (int)hipGetLastError();
    } else if constexpr (HD == 256) {
        p.nblk = (p.Nkv + kRows - 1) / kRows;
        {
            constexpr int lds = kStages * (2 * TILEB + 512);
            constexpr auto kern = fa2::bwd_dkv_kernel<HD, kBF16, false, false, NW, false, HD, 0, HD / 16, HD / 32>;
            if ((rc = fa2::set_lds<kern>(lds))) return rc;
            hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)p.B * p.H * p.nblk)), dim3(NW * 64), lds, stream, p FA2_WIN_MORE_ARGS);
            if ((rc = (int)hipGetLastError())) return rc;
        }
        {
            constexpr int lds = kStages * (3 * TILEB + 512);
            constexpr auto kern = fa2::bwd_dkv_kernel<HD, kBF16, false, true, NW, false, HD, 0, HD / 16, HD / 32>;
            if ((rc = fa2::set_lds<kern>(lds))) return rc;
            hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)p.B * p.H * p.nblk)), dim3(NW * 64), lds, stream, p FA2_WIN_MORE_ARGS);
            if ((rc = (int)hipGetLastError())) return rc;
        }
        return 0;
    } else {
        // head dims above 256: 128-column slabs of dQ / dV / dK per 128-row workgroup (grid.y), S and dP contracted over the whole head dim
        constexpr int HDV = 128;
        constexpr int TILEBV = fa2::Geo<HDV, NW>::TILEB;
        const unsigned slabs = (unsigned)((p.D + HDV - 1) / HDV);
        {
            constexpr int lds = 2 * TILEB + TILEBV;
            constexpr auto kern = fa2::bwd_dq_kernel<HD, kBF16, false, NW, HDV, 0, HD / 16, HDV / 32>;
            if ((rc = fa2::set_lds<kern>(lds))) return rc;
            p.nblk = (p.Nq + kRows - 1) / kRows;
            hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)p.B * p.H * p.nblk), slabs), dim3(NW * 64), lds, stream, p FA2_WIN_MORE_ARGS);
            if ((rc = (int)hipGetLastError())) return rc;
        }
        p.nblk = (p.Nkv + kRows - 1) / kRows;
        {
            constexpr int lds = TILEB + TILEBV + 512;
            constexpr auto kern = fa2::bwd_dkv_kernel<HD, kBF16, false, false, NW, false, HDV, 0, HD / 16, HDV / 32>;
            if ((rc = fa2::set_lds<kern>(lds))) return rc;
            hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)p.B * p.H * p.nblk), slabs), dim3(NW * 64), lds, stream, p FA2_WIN_MORE_ARGS);
            if ((rc = (int)hipGetLastError())) return rc;
        }
        {
            constexpr int lds = 2 * TILEB + TILEBV + 512;
            constexpr auto kern = fa2::bwd_dkv_kernel<HD, kBF16, false, true, NW, false, HDV, 0, HD / 16, HDV / 32>;
            if ((rc = fa2::set_lds<kern>(lds))) return rc;
            hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)p.B * p.H * p.nblk), slabs), dim3(NW * 64), lds, stream, p FA2_WIN_MORE_ARGS);
            if ((rc = (int)hipGetLastError())) return rc;
        }
        return 0;
    }
}

}  // namespace

namespace fa2 {

#if FA2_TU_BF16
int FA2_WIN_LAUNCH(fwd, bf16)(int HD, const FwdParams& p, int rows, hipStream_t stream FA2_WIN_MORE_PARAMS) {
#else
int FA2_WIN_LAUNCH(fwd, f16)(int HD, const FwdParams& p, int rows, hipStream_t stream FA2_WIN_MORE_PARAMS) {
#endif
    switch (HD) {
        case 64: return launch_fwd_hd<64>(p, rows, stream FA2_WIN_MORE_ARGS);
        case 128: return launch_fwd_hd<128>(p, rows, stream FA2_WIN_MORE_ARGS);
        case 256: return launch_fwd_hd<256>(p, rows, stream FA2_WIN_MORE_ARGS);
        case 512: return launch_fwd_hd<512>(p, rows, stream FA2_WIN_MORE_ARGS);
        default: return FA2_ERR_HEAD_DIM;
    }
}

#if FA2_TU_BF16
int FA2_WIN_LAUNCH(bwd, bf16)(int HD, const BwdParams& p, hipStream_t stream FA2_WIN_MORE_PARAMS) {
#else
int FA2_WIN_LAUNCH(bwd, f16)(int HD, const BwdParams& p, hipStream_t stream FA2_WIN_MORE_PARAMS) {
#endif
    switch (HD) {
        case 64: return launch_bwd_hd<64>(p, stream FA2_WIN_MORE_ARGS);
        case 128: return launch_bwd_hd<128>(p, stream FA2_WIN_MORE_ARGS);
        case 256: return launch_bwd_hd<256>(p, stream FA2_WIN_MORE_ARGS);
        case 512: return launch_bwd_hd<512>(p, stream FA2_WIN_MORE_ARGS);
        default: return FA2_ERR_HEAD_DIM;
    }
}

}  // namespace fa2
