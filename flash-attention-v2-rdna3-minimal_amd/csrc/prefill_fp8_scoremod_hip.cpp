// prefill_fp8_scoremod_hip.cpp — logit soft-capping and ALiBi slopes on chunked prefill against an e4m3 KV cache for ONE I/O dtype (fa2_fwd_prefill_fp8 with
// softcap > 0 or slopes): the FA2_KV8 form of prefill_scoremod_hip.cpp's kernel.  k_descale multiplies the scale of the modifier's natural units, so the
// cap sees the descaled score.  Forward only; head dims up to 256, as in prefill_fp8_hip.cpp.
#define FA2_WIN 1
#define FA2_VARLEN 1
#define FA2_PAGED 1
#define FA2_KV8 1
#define FA2_SMOD 1
#define FA2_FAMILY_FWD_ONLY 1
#define FA2_FAMILY_MAX_HD 256
#define FA2_FAMILY prefill_fp8_scoremod
#include "fa2_family_unit.h"
