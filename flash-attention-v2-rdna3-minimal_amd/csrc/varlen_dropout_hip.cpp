// varlen_dropout_hip.cpp — attention dropout on packed, variable-length batches for ONE dtype (fa2_fwd_varlen_dropout / fa2_bwd_varlen_dropout): the
// FA2_VARLEN + FA2_DROP forms of the kernels — varlen_hip.cpp's with the keep mask of fa2_dropout.h, keyed by the sequence index and the positions
// inside the sequence.
#define FA2_WIN 1
#define FA2_VARLEN 1
#define FA2_DROP 1
#define FA2_FAMILY varlen_dropout
#include "fa2_family_unit.h"
