// kvappend_varlen_hip.cpp — the packed (ragged) KV-cache append (fa2_kvcache_append_varlen): the instantiation of kvappend_varlen_kernel
// (csrc/fa2_kvappend.hip.h) for one I/O dtype and one cache format, and its launcher.  build.py compiles the unit four times with the flags of
// kvappend_hip.cpp (NaNs honoured: the e4m3 clamp lets a NaN through to the convert).  host.cpp validates the call and fills KvAppendVarlenParams.
#include "fa2_launch.h"

#include "fa2_gfx950.h"

#ifndef FA2_TU_FP8
#define FA2_TU_FP8 0
#endif

namespace fa2 {

// grid: x = the packed token, y = slices of the token's R * UR units
#if FA2_TU_FP8
int FA2_DT(launch_kvappend_varlen_fp8)(const KvAppendVarlenParams& p, int64_t total, hipStream_t stream) {
#else
int FA2_DT(launch_kvappend_varlen)(const KvAppendVarlenParams& p, int64_t total, hipStream_t stream) {
#endif
    const int units = p.R * p.UR, threads = append_threads(units);
    const dim3 grid((unsigned)total, (unsigned)((units + threads - 1) / threads)), block(threads);
    return launch<kvappend_varlen_kernel<FA2_TU_BF16 != 0, FA2_TU_FP8 != 0>>(grid, block, 0, stream, p);
}

}  // namespace fa2
