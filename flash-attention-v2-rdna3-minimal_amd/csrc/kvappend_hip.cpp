// kvappend_hip.cpp — KV-cache append with rotary embedding and e4m3 quantisation (fa2_kvcache_append): the instantiation of csrc/fa2_kvappend.hip.h for one
// I/O dtype and one cache format (build.py compiles the unit four times, like decode_hip.cpp, and with NaNs honoured: the e4m3 clamp lets a NaN through
// to the convert) and its launcher.  host.cpp validates the call and fills KvAppendParams; this unit executes it.
#include "fa2_launch.h"

#include "fa2_gfx950.h"

#ifndef FA2_TU_FP8
#define FA2_TU_FP8 0
#endif

namespace fa2 {

// grid: x = the (sequence, token) group, y = slices of the group's R * UR units
#if FA2_TU_FP8
int FA2_DT(launch_kvappend_fp8)(const KvAppendParams& p, hipStream_t stream) {
#else
int FA2_DT(launch_kvappend)(const KvAppendParams& p, hipStream_t stream) {
#endif
    const int units = p.R * p.UR, threads = append_threads(units);
    const dim3 grid((unsigned)((int64_t)p.B * p.Nnew), (unsigned)((units + threads - 1) / threads)), block(threads);
    return launch<kvappend_kernel<FA2_TU_BF16 != 0, FA2_TU_FP8 != 0>>(grid, block, 0, stream, p);
}

}  // namespace fa2
