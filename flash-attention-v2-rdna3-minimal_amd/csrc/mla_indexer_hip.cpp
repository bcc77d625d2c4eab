// mla_indexer_hip.cpp — the lightning indexer's logits (fa2_mla_indexer_logits): the instantiations of csrc/fa2_mla_indexer.hip.h for one dtype
// (build.py compiles the unit twice, -DFA2_TU_BF16=0 and =1), one per served head count, and their launcher.  host.cpp validates the call; this unit
// executes it.
#include "fa2_mla_indexer.hip.h"

#include "fa2_gfx950.h"

namespace fa2 {
namespace {
constexpr bool kBF16 = FA2_TU_BF16 != 0;
}  // namespace

int FA2_DT(launch_mla_indexer_logits)(const MlaIndexerParams& p, hipStream_t stream) {
    const dim3 grid((unsigned)mla_indexer_chunks(p.capacity_keys), (unsigned)p.Nq, (unsigned)p.B), block(kIdxWaves * 64);
    switch (p.H / 16) {
        case 1: return launch<mla_indexer_logits_kernel<kBF16, 1>>(grid, block, 0, stream, p);
        case 2: return launch<mla_indexer_logits_kernel<kBF16, 2>>(grid, block, 0, stream, p);
        case 3: return launch<mla_indexer_logits_kernel<kBF16, 3>>(grid, block, 0, stream, p);
        case 4: return launch<mla_indexer_logits_kernel<kBF16, 4>>(grid, block, 0, stream, p);
    }
    return FA2_ERR_HEAD_DIM;      // a head count without a kernel is an error, never another path
}

}  // namespace fa2
