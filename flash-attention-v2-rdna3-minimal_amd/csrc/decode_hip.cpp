// decode_hip.cpp — KV-cache decode attention (fa2_fwd_decode): the instantiations of csrc/fa2_decode.hip.h for one dtype (build.py compiles the unit
// twice, -DFA2_TU_BF16=0 and =1) and their launchers.  host.cpp validates the call and makes the plan (decode_plan); this unit executes it.
#include "fa2_launch.h"

#include "fa2_gfx950.h"

namespace fa2 {
namespace {

constexpr bool kBF16 = FA2_TU_BF16 != 0;

template <int HD>
int launch_decode_hd(const DecodeParams& p, int row_tiles, hipStream_t stream) {
    const dim3 grid((unsigned)p.nsplit, (unsigned)p.Hkv, (unsigned)p.B), block(kDecodeWaves * 64);
    int rc;
    switch (row_tiles) {
        case 1: rc = launch<decode_kernel<HD, kBF16, 1>>(grid, block, 0, stream, p); break;
        case 2: rc = launch<decode_kernel<HD, kBF16, 2>>(grid, block, 0, stream, p); break;
        default: rc = launch<decode_kernel<HD, kBF16, 4>>(grid, block, 0, stream, p); break;      // three row tiles run the four-tile kernel
    }
    if (rc || p.nsplit <= 1) return rc;
    const int64_t threads = (int64_t)p.B * p.Hkv * p.rows * (HD / 8);
    return launch<decode_combine_kernel<HD, kBF16>>(dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, p);
}

}  // namespace

int FA2_DT(launch_decode)(int HD, const DecodeParams& p, int row_tiles, hipStream_t stream) {
    return HD == 64 ? launch_decode_hd<64>(p, row_tiles, stream) : launch_decode_hd<128>(p, row_tiles, stream);
}

}  // namespace fa2
