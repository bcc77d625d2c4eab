// prefill_mla_sparse_fp8_hip.cpp — sparse (top-k indexed) attention for packed tokens on an e4m3 latent (MLA) KV cache of 656-byte rows
// (fa2_fwd_prefill_mla_sparse_fp8): the FP8 instantiation of csrc/fa2_prefill_mla_sparse.hip.h for one I/O dtype (build.py compiles the unit twice,
// -DFA2_TU_BF16=0 and =1) and its launcher.  host.cpp validates the call; this unit executes it.
#include "fa2_prefill_mla_sparse.hip.h"

#include "fa2_gfx950.h"

namespace fa2 {
namespace {
constexpr bool kBF16 = FA2_TU_BF16 != 0;
}  // namespace

int FA2_DT(launch_prefill_mla_sparse_fp8)(const PrefillMlaSparseParams& p, uint32_t items, hipStream_t stream) {
    return launch<prefill_mla_sparse_fp8_kernel<kBF16>>(dim3(items), dim3(kDecodeWaves * 64), kMlaLdsBytes, stream, p);
}

}  // namespace fa2
