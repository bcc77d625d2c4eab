// varlen_hip.cpp — packed, variable-length attention for ONE dtype (fa2_fwd_varlen / fa2_bwd_varlen): the FA2_VARLEN forms of the compiler-scheduled
// forward kernel and backward passes.  They are the sliding-window forms (FA2_WIN, window_hip.cpp) with the lengths, the base rows and the band's offset
// taken per sequence from cu_seqlens (varlen_enter in the kernel headers), so one kernel family serves plain, causal (top-left or bottom-right), windowed
// and grouped packed calls, and a band that masks nothing runs the unmasked steady-state loop.  build.py compiles this file twice (-DFA2_TU_BF16=0 / 1).
// The launchers are window_hip.cpp's, compiled here under names of their own: the host hands them the stated maximum lengths as Nq / Nkv, which size
// the grids B * H * ceil(max_seqlen / rows); a workgroup whose block starts beyond its sequence's length returns at once.
// No hand-scheduled bodies, no KV-split, no longest-first order, no host-built work list (DESIGN has them as next steps).
#define FA2_VARLEN 1
#define FA2_WIN 1
#define fwd_kernel fwd_varlen_kernel
#define bwd_dq_kernel bwd_varlen_dq_kernel
#define bwd_dkv_kernel bwd_varlen_dkv_kernel
#define bwd_dkv_pair_kernel bwd_varlen_dkv_pair_kernel
#define FA2_WIN_LAUNCH(pass, dt) launch_##pass##_varlen_##dt
#include "window_hip.cpp"
