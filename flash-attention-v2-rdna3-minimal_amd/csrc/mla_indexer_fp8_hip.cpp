// mla_indexer_fp8_hip.cpp — the lightning indexer's logits over an e4m3 index-key cache (fa2_mla_indexer_logits_fp8) and the quantising append that
// writes that cache (fa2_kvcache_append_mla_index_fp8): the instantiations of csrc/fa2_mla_indexer_fp8.hip.h — one per q form (e4m3, fp16, bf16) and
// served head count — and of csrc/fa2_kvappend_mla_index_fp8.hip.h, and their launchers.  One unit: the cache has no I/O dtype.  host.cpp validates the
// calls; this unit executes them.
#include "fa2_mla_indexer_fp8.hip.h"
#include "fa2_kvappend_mla_index_fp8.hip.h"

#include "fa2_gfx950.h"

namespace fa2 {
namespace {

template <int QF>
int launch_form(const MlaIndexerFp8Params& p, hipStream_t stream) {
    const dim3 grid((unsigned)mla_indexer_chunks(p.capacity_keys), (unsigned)p.Nq, (unsigned)p.B), block(kIdxWaves * 64);
    switch (p.H / 16) {
        case 1: return launch<mla_indexer_logits_fp8_kernel<QF, 1>>(grid, block, 0, stream, p);
        case 2: return launch<mla_indexer_logits_fp8_kernel<QF, 2>>(grid, block, 0, stream, p);
        case 3: return launch<mla_indexer_logits_fp8_kernel<QF, 3>>(grid, block, 0, stream, p);
        case 4: return launch<mla_indexer_logits_fp8_kernel<QF, 4>>(grid, block, 0, stream, p);
    }
    return FA2_ERR_HEAD_DIM;      // a head count without a kernel is an error, never another path
}

}  // namespace

int launch_mla_indexer_logits_fp8(int q_form, const MlaIndexerFp8Params& p, hipStream_t stream) {
    switch (q_form) {
        case kIdxQE4M3: return launch_form<kIdxQE4M3>(p, stream);
        case kIdxQF16: return launch_form<kIdxQF16>(p, stream);
        case kIdxQBF16: return launch_form<kIdxQBF16>(p, stream);
    }
    return FA2_ERR_DTYPE;
}

int launch_kvappend_mla_index_fp8(bool bf16, const KvAppendMlaIndexParams& p, hipStream_t stream) {
    const dim3 grid((unsigned)((p.tokens + kIdxAppendTokens - 1) / kIdxAppendTokens)), block(kIdxAppendThreads);
    return bf16 ? launch<kvappend_mla_index_fp8_kernel<true>>(grid, block, 0, stream, p) : launch<kvappend_mla_index_fp8_kernel<false>>(grid, block, 0, stream, p);
}

}  // namespace fa2
