// dropout_hip.cpp — attention dropout for ONE dtype (fa2_fwd_dropout / fa2_bwd_dropout): the FA2_DROP forms of the compiler-scheduled forward kernel and
// backward passes.  They are the sliding-window forms (FA2_WIN, window_hip.cpp) with the Philox keep mask of fa2_dropout.h applied to the probabilities
// after the softmax, so one kernel family serves plain (window = (-1, -1)), causal, windowed, offset and grouped dropout calls.  build.py compiles this
// file twice (-DFA2_TU_BF16=0 / 1).  The launchers are window_hip.cpp's, compiled here under names of their own; the host puts the seed and the threshold
// into the parameter block (set_dropout) before it calls them.  varlen_dropout_hip.cpp includes this file under FA2_VARLEN for the packed forms.
#define FA2_DROP 1
#ifndef FA2_VARLEN
#define FA2_WIN 1
#define FA2_VARLEN 0
#define fwd_kernel fwd_dropout_kernel
#define bwd_dq_kernel bwd_dropout_dq_kernel
#define bwd_dkv_kernel bwd_dropout_dkv_kernel
#define bwd_dkv_pair_kernel bwd_dropout_dkv_pair_kernel
#define FA2_WIN_LAUNCH(pass, dt) launch_##pass##_dropout_##dt
#endif
#include "window_hip.cpp"
