// prefill_fp8_hip.cpp — chunked prefill against an e4m3 KV cache for ONE I/O dtype (fa2_fwd_prefill_fp8): the FA2_KV8 form of prefill_hip.cpp's kernel.
// K / V tiles are fetched as e4m3 bytes, 8 per LDS granule, converted to the I/O dtype in registers (exact) and written to the LDS image the 16-bit kernel
// builds — the register form of the staging at every head dim — and the per (sequence, K / V head) descales ride in the score factor and in the epilogue's
// row factor.  Everything after the LDS image is prefill_hip.cpp's, so with power-of-two descales a call equals fa2_fwd_prefill on the dequantised cache
// bit for bit.  Head dims up to 256: the head-dim-512 instantiation needs scratch memory with the staging registers and is not compiled.
#define FA2_WIN 1
#define FA2_VARLEN 1
#define FA2_PAGED 1
#define FA2_KV8 1
#define FA2_FAMILY_FWD_ONLY 1
#define FA2_FAMILY_MAX_HD 256
#define FA2_FAMILY prefill_fp8
#include "fa2_family_unit.h"
