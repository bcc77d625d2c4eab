// prefill_hip.cpp — chunked prefill against a KV cache for ONE dtype (fa2_fwd_prefill): the FA2_PAGED form of the compiler-scheduled forward kernel.
// It is the packed form (FA2_VARLEN, varlen_hip.cpp) with a sequence's key count taken from cache_seqlens and every 64-key K / V tile staged through a
// buffer descriptor built for that tile — from the block table's page id in a paged cache, from the sequence's own slab in a contiguous one (paged_enter,
// PagedCursor in fa2_fwd_kernel.hip.h; fa2_prefill.h has the tile arithmetic).  Everything after the staging is the packed kernel's, instruction for
// instruction, so a call's results equal fa2_fwd_varlen's on the gathered keys bit for bit.
// An inference call: forward only.  No KV-split, as in every family.
#define FA2_WIN 1
#define FA2_VARLEN 1
#define FA2_PAGED 1
#define FA2_FAMILY_FWD_ONLY 1
#define FA2_FAMILY prefill
#include "fa2_family_unit.h"
