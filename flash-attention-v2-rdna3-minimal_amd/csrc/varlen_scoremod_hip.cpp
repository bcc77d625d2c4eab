// varlen_scoremod_hip.cpp — logit soft-capping and ALiBi slopes on packed, variable-length batches for ONE dtype (fa2_fwd_varlen_scoremod /
// fa2_bwd_varlen_scoremod): the FA2_VARLEN + FA2_SMOD forms of the kernels — varlen_hip.cpp's with the transform of fa2_scoremod.h; the slope vector is
// chosen by the sequence index, the positions count inside the sequence.  build.py compiles this file twice (-DFA2_TU_BF16=0 / 1).
#define FA2_VARLEN 1
#define FA2_WIN 1
#define fwd_kernel fwd_varlen_scoremod_kernel
#define bwd_dq_kernel bwd_varlen_scoremod_dq_kernel
#define bwd_dkv_kernel bwd_varlen_scoremod_dkv_kernel
#define bwd_dkv_pair_kernel bwd_varlen_scoremod_dkv_pair_kernel
#define FA2_WIN_LAUNCH(pass, dt) launch_##pass##_varlen_scoremod_##dt
#include "scoremod_hip.cpp"
