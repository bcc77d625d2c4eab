// varlen_dropout_hip.cpp — attention dropout on packed, variable-length batches for ONE dtype (fa2_fwd_varlen_dropout / fa2_bwd_varlen_dropout): the
// FA2_VARLEN + FA2_DROP forms of the kernels — varlen_hip.cpp's with the keep mask of fa2_dropout.h, keyed by the sequence index and the positions
// inside the sequence.  build.py compiles this file twice (-DFA2_TU_BF16=0 / 1).
#define FA2_VARLEN 1
#define FA2_WIN 1
#define fwd_kernel fwd_varlen_dropout_kernel
#define bwd_dq_kernel bwd_varlen_dropout_dq_kernel
#define bwd_dkv_kernel bwd_varlen_dropout_dkv_kernel
#define bwd_dkv_pair_kernel bwd_varlen_dropout_dkv_pair_kernel
#define FA2_WIN_LAUNCH(pass, dt) launch_##pass##_varlen_dropout_##dt
#include "dropout_hip.cpp"
