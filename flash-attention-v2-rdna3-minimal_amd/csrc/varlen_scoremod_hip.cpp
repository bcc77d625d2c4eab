// varlen_scoremod_hip.cpp — logit soft-capping and ALiBi slopes on packed, variable-length batches for ONE dtype (fa2_fwd_varlen_scoremod /
// fa2_bwd_varlen_scoremod): the FA2_VARLEN + FA2_SMOD forms of the kernels — varlen_hip.cpp's with the transform of fa2_scoremod.h; the slope vector is
// chosen by the sequence index, the positions count inside the sequence.
#define FA2_WIN 1
#define FA2_VARLEN 1
#define FA2_SMOD 1
#define FA2_FAMILY varlen_scoremod
#include "fa2_family_unit.h"
