// decode_wide_hip.cpp — KV-cache decode attention at head dim 256 (fa2_fwd_decode_wide): the instantiations of csrc/fa2_decode_wide.hip.h for one dtype and
// one cache format (build.py compiles the unit four times, like decode_hip.cpp) and their launcher; the 16-bit units also hold the 256-wide instance of
// decode's combine kernel.  host.cpp validates the call and makes the plan (decode_plan); this unit executes it.
#include "fa2_launch.h"

#include "fa2_decode_wide.hip.h"
#include "fa2_gfx950.h"

#ifndef FA2_TU_FP8
#define FA2_TU_FP8 0
#endif

namespace fa2 {
namespace {

constexpr bool kBF16 = FA2_TU_BF16 != 0;
constexpr bool kFP8 = FA2_TU_FP8 != 0;

// grid: (row block, part) x K / V head x sequence; row_tiles: the tiles of ONE workgroup (1 or 2)
template <int RT, bool BAND>
int launch_wide_rt(const DecodeParams& p, hipStream_t stream) {
    const dim3 grid((unsigned)(p.nsplit * decode_wide_row_blocks(p.rows)), (unsigned)p.Hkv, (unsigned)p.B), block(kDecodeWaves * 64);
    return launch<decode_wide_kernel<kBF16, RT, kFP8, BAND>>(grid, block, decode_wide_lds_bytes(RT), stream, p);
}

int launch_wide(const DecodeParams& p, int row_tiles, bool band, hipStream_t stream) {
    if (row_tiles == 1) return band ? launch_wide_rt<1, true>(p, stream) : launch_wide_rt<1, false>(p, stream);
    return band ? launch_wide_rt<2, true>(p, stream) : launch_wide_rt<2, false>(p, stream);
}

}  // namespace

#if FA2_TU_FP8
int FA2_DT(launch_decode_wide_fp8)(const DecodeParams& p, int row_tiles, bool band, hipStream_t stream) {
    if (int rc = launch_wide(p, row_tiles, band, stream)) return rc;
    return p.nsplit > 1 ? FA2_DT(launch_decode_wide_combine)(p, stream) : 0;      // the parts are f32 rows whatever the cache held
}
#else
int FA2_DT(launch_decode_wide)(const DecodeParams& p, int row_tiles, bool band, hipStream_t stream) {
    if (int rc = launch_wide(p, row_tiles, band, stream)) return rc;
    return p.nsplit > 1 ? FA2_DT(launch_decode_wide_combine)(p, stream) : 0;
}

int FA2_DT(launch_decode_wide_combine)(const DecodeParams& p, hipStream_t stream) {
    const int64_t threads = (int64_t)p.B * p.Hkv * p.rows * (kDecodeWideHD / 8);
    const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
    return launch<decode_combine_kernel<kDecodeWideHD, kBF16>>(grid, block, 0, stream, p);
}
#endif

}  // namespace fa2
