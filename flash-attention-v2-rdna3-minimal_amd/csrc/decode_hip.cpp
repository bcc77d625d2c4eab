// decode_hip.cpp — KV-cache decode attention (fa2_fwd_decode, fa2_fwd_decode_fp8, fa2_fwd_decode_window): the instantiations of csrc/fa2_decode.hip.h for
// one dtype and one cache format (build.py compiles the unit four times, -DFA2_TU_BF16=0 and =1, each with and without -DFA2_TU_FP8=1) and their
// launchers.  host.cpp validates the call and makes the plan (decode_plan); this unit executes it.
#include "fa2_launch.h"

#include "fa2_gfx950.h"

#ifndef FA2_TU_FP8
#define FA2_TU_FP8 0
#endif

namespace fa2 {
namespace {

constexpr bool kBF16 = FA2_TU_BF16 != 0;
constexpr bool kFP8 = FA2_TU_FP8 != 0;      // the caches hold e4m3 bytes (the I/O dtype stays kBF16's)

// BAND: the kernels with a sliding window, soft-capping and ALiBi slopes (fa2_fwd_decode_window); the plain ones are the instantiations they were
template <int HD, bool BAND>
int launch_decode_hd(const DecodeParams& p, int row_tiles, hipStream_t stream) {
    const dim3 grid((unsigned)p.nsplit, (unsigned)p.Hkv, (unsigned)p.B), block(kDecodeWaves * 64);
    int rc;
    switch (row_tiles) {
        case 1: rc = launch<decode_kernel<HD, kBF16, 1, kFP8, BAND>>(grid, block, 0, stream, p); break;
        case 2: rc = launch<decode_kernel<HD, kBF16, 2, kFP8, BAND>>(grid, block, 0, stream, p); break;
        default: rc = launch<decode_kernel<HD, kBF16, 4, kFP8, BAND>>(grid, block, 0, stream, p); break;      // three row tiles run the four-tile kernel
    }
    if (rc || p.nsplit <= 1) return rc;
    return FA2_DT(launch_decode_combine)(HD, p, stream);      // the parts are f32 rows whatever the cache held: ONE combine kernel, in the 16-bit unit
}

}  // namespace

#if FA2_TU_FP8
int FA2_DT(launch_decode_fp8)(int HD, const DecodeParams& p, int row_tiles, hipStream_t stream) {
    return HD == 64 ? launch_decode_hd<64, false>(p, row_tiles, stream) : launch_decode_hd<128, false>(p, row_tiles, stream);
}
int FA2_DT(launch_decode_band_fp8)(int HD, const DecodeParams& p, int row_tiles, hipStream_t stream) {
    return HD == 64 ? launch_decode_hd<64, true>(p, row_tiles, stream) : launch_decode_hd<128, true>(p, row_tiles, stream);
}
#else
int FA2_DT(launch_decode)(int HD, const DecodeParams& p, int row_tiles, hipStream_t stream) {
    return HD == 64 ? launch_decode_hd<64, false>(p, row_tiles, stream) : launch_decode_hd<128, false>(p, row_tiles, stream);
}
int FA2_DT(launch_decode_band)(int HD, const DecodeParams& p, int row_tiles, hipStream_t stream) {
    return HD == 64 ? launch_decode_hd<64, true>(p, row_tiles, stream) : launch_decode_hd<128, true>(p, row_tiles, stream);
}

int FA2_DT(launch_decode_combine)(int HD, const DecodeParams& p, hipStream_t stream) {
    const int64_t threads = (int64_t)p.B * p.Hkv * p.rows * (HD / 8);
    const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
    return HD == 64 ? launch<decode_combine_kernel<64, kBF16>>(grid, block, 0, stream, p) : launch<decode_combine_kernel<128, kBF16>>(grid, block, 0, stream, p);
}
#endif

}  // namespace fa2
