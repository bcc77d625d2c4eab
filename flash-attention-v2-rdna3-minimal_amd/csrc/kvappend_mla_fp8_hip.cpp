// kvappend_mla_fp8_hip.cpp — the quantising append for an e4m3 latent (MLA) KV cache (fa2_kvcache_append_mla_fp8, fa2_kvcache_append_mla_varlen_fp8):
// the instantiations of the two kernels of csrc/fa2_kvappend_mla_fp8.hip.h for one I/O dtype, and their launcher.  build.py compiles the unit twice, with
// NaNs honoured like the other append units (a NaN in kv_c falls through the e4m3 clamp to the convert; a NaN in k_pe goes through the rotation as a
// NaN).  host.cpp validates the call and fills KvAppendMlaParams — kv_cache the byte cache, ks in bytes; this unit executes it.
#include "fa2_kvappend_mla_fp8.hip.h"

#include "fa2_gfx950.h"

namespace fa2 {

// grid: x = the (sequence, token) group or the packed token, y = slices of the group's R * 36 units — the 16-bit launcher's, whose q units the kernels
// keep; at least 64 lanes per workgroup, so the wave that quantises the latent row is whole
int FA2_DT(launch_kvappend_mla_fp8)(const KvAppendMlaParams& p, int64_t groups, bool packed, hipStream_t stream) {
    constexpr bool kBF16 = FA2_TU_BF16 != 0;
    const int units = p.R * kMlaUnits, threads = append_threads(units);
    const dim3 grid((unsigned)groups, (unsigned)((units + threads - 1) / threads)), block(threads);
    if (packed) return launch<kvappend_mla_varlen_fp8_kernel<kBF16>>(grid, block, 0, stream, p);
    return launch<kvappend_mla_fp8_kernel<kBF16>>(grid, block, 0, stream, p);
}

}  // namespace fa2
