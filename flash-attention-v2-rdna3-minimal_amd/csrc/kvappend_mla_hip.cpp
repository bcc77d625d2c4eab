// kvappend_mla_hip.cpp — the append for a latent (MLA) KV cache (fa2_kvcache_append_mla, fa2_kvcache_append_mla_varlen): the instantiations of the two
// kernels of csrc/fa2_kvappend_mla.hip.h for one I/O dtype, and their launcher.  build.py compiles the unit twice, with NaNs honoured like the other
// append units (a NaN in k_pe goes through the rotation as a NaN).  host.cpp validates the call and fills KvAppendMlaParams; this unit executes it.
#include "fa2_kvappend_mla.hip.h"

#include "fa2_gfx950.h"

namespace fa2 {

// grid: x = the (sequence, token) group or the packed token, y = slices of the group's R * 36 units
int FA2_DT(launch_kvappend_mla)(const KvAppendMlaParams& p, int64_t groups, bool packed, hipStream_t stream) {
    constexpr bool kBF16 = FA2_TU_BF16 != 0;
    const int units = p.R * kMlaUnits, threads = append_threads(units);
    const dim3 grid((unsigned)groups, (unsigned)((units + threads - 1) / threads)), block(threads);
    if (packed) return launch<kvappend_mla_varlen_kernel<kBF16>>(grid, block, 0, stream, p);
    return launch<kvappend_mla_kernel<kBF16>>(grid, block, 0, stream, p);
}

}  // namespace fa2
