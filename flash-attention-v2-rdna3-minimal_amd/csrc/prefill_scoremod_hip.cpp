// prefill_scoremod_hip.cpp — logit soft-capping and ALiBi slopes on chunked prefill against a KV cache for ONE dtype (fa2_fwd_prefill with softcap > 0 or
// slopes): the FA2_PAGED + FA2_SMOD form of the forward kernel — prefill_hip.cpp's with the transform of fa2_scoremod.h; the slope vector is chosen by the
// sequence index, the positions are those of the cache (row i of a chunk sits at cache_seqlens[s] - Nq_s + i).  Forward only.
#define FA2_WIN 1
#define FA2_VARLEN 1
#define FA2_PAGED 1
#define FA2_SMOD 1
#define FA2_FAMILY_FWD_ONLY 1
#define FA2_FAMILY prefill_scoremod
#include "fa2_family_unit.h"
