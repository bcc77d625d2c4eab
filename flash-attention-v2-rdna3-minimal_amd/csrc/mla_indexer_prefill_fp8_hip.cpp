// mla_indexer_prefill_fp8_hip.cpp — the lightning indexer's logits for packed query tokens over an e4m3 index-key cache
// (fa2_mla_indexer_logits_varlen_fp8): the instantiations of csrc/fa2_mla_indexer_prefill_fp8.hip.h — one per q form (e4m3, fp16, bf16) and served head
// count — and their launcher.  One unit: the cache has no I/O dtype.  host.cpp validates the call; this unit executes it.
#include "fa2_mla_indexer_prefill_fp8.hip.h"

#include "fa2_gfx950.h"

namespace fa2 {
namespace {

template <int QF>
int launch_form(const MlaIndexerPrefillParams& p, hipStream_t stream) {
    const dim3 grid((unsigned)mla_indexer_prefill_chunks(p.capacity_keys), (unsigned)mla_indexer_prefill_blocks(p.total_q)), block(kIdxPfThreads);
    const int lds = mla_indexer_prefill_lds(p.H, QF);
    switch (p.H / 16) {
        case 1: return launch<mla_indexer_prefill_fp8_kernel<QF, 1>>(grid, block, lds, stream, p);
        case 2: return launch<mla_indexer_prefill_fp8_kernel<QF, 2>>(grid, block, lds, stream, p);
        case 3: return launch<mla_indexer_prefill_fp8_kernel<QF, 3>>(grid, block, lds, stream, p);
        case 4: return launch<mla_indexer_prefill_fp8_kernel<QF, 4>>(grid, block, lds, stream, p);
    }
    return FA2_ERR_HEAD_DIM;      // a head count without a kernel is an error, never another path
}

}  // namespace

int launch_mla_indexer_prefill_fp8(int q_form, const MlaIndexerPrefillParams& p, hipStream_t stream) {
    switch (q_form) {
        case kIdxQE4M3: return launch_form<kIdxQE4M3>(p, stream);
        case kIdxQF16: return launch_form<kIdxQF16>(p, stream);
        case kIdxQBF16: return launch_form<kIdxQBF16>(p, stream);
    }
    return FA2_ERR_DTYPE;
}

}  // namespace fa2
