// varlen_dv_hip.cpp — packed attention with V narrower than K for ONE dtype (fa2_fwd_varlen_dv: the non-absorbed MLA prefill, head dims 192 / 128): the
// FA2_DV form of the packed forward kernel (FA2_VARLEN, varlen_hip.cpp).  Forward only, so the unit names its one kernel and its launches itself instead
// of going through fa2_family_unit.h, which would instantiate every head dim and the backward passes.
// Served pairs: D a multiple of 8 in 136 .. 256, Dv a multiple of 8 in 8 .. 128 (host.cpp checks them).  Every one runs the kernel of head dim 256 with
// HDV = 128 as ONE column slab: the K image keeps its 256-column geometry (granules at or beyond D are never fetched), Q.K^T runs KSQ = 12 k-steps for
// D <= 192 and 16 above, and the O column blocks are the run-time ceil(Dv / 32) (RTD).  Against the padded route — V zero-padded to D through
// fa2_fwd_varlen, two 128-column slabs of 16 k-steps each — that is 24 + 16 = 40 MFMAs per (32 rows x 64 keys) at 192 / 128 instead of 96.
// Workgroup shapes: 128 rows (4 waves, one per SIMD with the 512-register budget) and 256 rows (8 waves); neither uses scratch memory
// (tests/test_varlen_dv.py reads the private segment sizes off the compiler).
#define FA2_WIN 1
#define FA2_VARLEN 1
#define FA2_DV 1
#define fwd_kernel fwd_varlen_dv_kernel
#include "fa2_pass_launch.h"

namespace {

template <int NW, int KSQ>
int launch_dv_shape(const fa2::FwdParams& p0, int Dv, hipStream_t stream) {
    constexpr int HD = 256, HDV = 128;
    constexpr int lds_kv = 2 * fa2::Geo<HD, NW>::TILEB + 2 * fa2::Geo<HDV, NW>::TILEB;      // 96 KiB: one workgroup per CU
    constexpr int lds_epi = FA2_EPI_LDS ? NW * 32 * (HDV * 2 + 16) : 0;                    // epilogue image (reuses the K / V space)
    constexpr int lds = lds_kv > lds_epi ? lds_kv : lds_epi;
    static_assert(lds <= 160 * 1024, "LDS budget");
    fa2::FwdParams p = p0;
    p.nsplit = 0;
    p.nqblk = (p.Nq + NW * 32 - 1) / (NW * 32);
    const int64_t nblk = (int64_t)p.nbh * p.nqblk;
    if (nblk > 0x7fffffffLL) return FA2_ERR_GRID;
    return fa2::launch<fa2::fwd_kernel<HD, HDV, kBF16, false, NW, 1, 0, KSQ, HDV / 32, true>>(dim3((unsigned)nblk, 1), dim3(NW * 64), lds, stream, p, Dv);
}

}  // namespace

namespace fa2 {

int FA2_DT(launch_fwd_varlen_dv)(const FwdParams& p, int Dv, int rows, hipStream_t stream) {
    if (p.D > 256 || Dv < 1 || Dv > 128) return FA2_ERR_HEAD_DIM;
    if (rows == 128) return p.D <= 192 ? launch_dv_shape<4, 12>(p, Dv, stream) : launch_dv_shape<4, 16>(p, Dv, stream);
    return p.D <= 192 ? launch_dv_shape<8, 12>(p, Dv, stream) : launch_dv_shape<8, 16>(p, Dv, stream);
}

}  // namespace fa2
