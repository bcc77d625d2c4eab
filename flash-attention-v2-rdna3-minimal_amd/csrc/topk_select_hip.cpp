// topk_select_hip.cpp — the top-k selection over the indexer's logits (fa2_topk_indices, fa2_topk_indices_varlen): the kernel of csrc/fa2_topk_select.hip.h in
// its uniform and its packed row geometry, and their launchers.
// One unit: the kernel reads float32 logits whatever the I/O dtype of the indexer was.  host.cpp validates the call; this unit executes it.
#include "fa2_topk_select.hip.h"

#include "fa2_gfx950.h"

namespace fa2 {

int launch_topk_select(const TopkParams& p, hipStream_t stream) {
    return launch<topk_select_kernel<kTopkThreads>>(dim3((unsigned)((int64_t)p.B * p.Nq)), dim3(kTopkThreads), 0, stream, p);
}

int launch_topk_select_varlen(const TopkParams& p, hipStream_t stream) {
    return launch<topk_select_kernel<kTopkThreads, true>>(dim3((unsigned)p.Nq), dim3(kTopkThreads), 0, stream, p);
}

}  // namespace fa2
