// decode_mla_hip.cpp — decode attention on a latent (MLA) KV cache (fa2_fwd_decode_mla): the instantiations of csrc/fa2_decode_mla.hip.h for one dtype
// (build.py compiles the unit twice, -DFA2_TU_BF16=0 and =1), the 512-wide instantiation of decode_combine_kernel, and their launcher.  host.cpp
// validates the call and makes the plan (decode_mla_plan); this unit executes it.
#include "fa2_decode_mla.hip.h"

#include "fa2_gfx950.h"

namespace fa2 {
namespace {
constexpr bool kBF16 = FA2_TU_BF16 != 0;
}  // namespace

int FA2_DT(launch_decode_mla)(const DecodeParams& p, hipStream_t stream) {
    const dim3 grid((unsigned)p.nsplit, (unsigned)mla_row_blocks(p.rows), (unsigned)p.B), block(kDecodeWaves * 64);
    if (int rc = launch<decode_mla_kernel<kBF16>>(grid, block, kMlaLdsBytes, stream, p)) return rc;
    if (p.nsplit <= 1) return 0;
    const int64_t threads = (int64_t)p.B * p.rows * (kMlaDv / 8);
    return launch<decode_combine_kernel<kMlaDv, kBF16>>(dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, p);
}

}  // namespace fa2
