// scoremod_hip.cpp — logit soft-capping and ALiBi slopes for ONE dtype (fa2_fwd_scoremod / fa2_bwd_scoremod): the FA2_SMOD forms of the compiler-scheduled
// forward kernel and backward passes.  They are the sliding-window forms (FA2_WIN, window_hip.cpp) with the transform of fa2_scoremod.h applied to the
// scores between Q.K^T and the softmax, before the band's masks, so one kernel family serves plain (window = (-1, -1)), causal, windowed, offset and
// grouped calls.  build.py compiles this file twice (-DFA2_TU_BF16=0 / 1).  The launchers are window_hip.cpp's, compiled here under names of their own and
// with one further parameter: the ScoreMod block (softcap, the slope pointer and its stride), which the kernels take as a further argument.
// varlen_scoremod_hip.cpp includes this file under FA2_VARLEN for the packed forms.
#define FA2_SMOD 1
#ifndef FA2_VARLEN
#define FA2_WIN 1
#define FA2_VARLEN 0
#define fwd_kernel fwd_scoremod_kernel
#define bwd_dq_kernel bwd_scoremod_dq_kernel
#define bwd_dkv_kernel bwd_scoremod_dkv_kernel
#define bwd_dkv_pair_kernel bwd_scoremod_dkv_pair_kernel
#define FA2_WIN_LAUNCH(pass, dt) launch_##pass##_scoremod_##dt
#endif
#include "window_hip.cpp"
