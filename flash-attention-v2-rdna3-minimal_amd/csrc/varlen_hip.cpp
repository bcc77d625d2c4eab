// varlen_hip.cpp — packed, variable-length attention for ONE dtype (fa2_fwd_varlen / fa2_bwd_varlen): the FA2_VARLEN forms of the compiler-scheduled
// forward kernel and backward passes.  They are the sliding-window forms (FA2_WIN, window_hip.cpp) with the lengths, the base rows and the band's offset
// taken per sequence from cu_seqlens (varlen_enter in the kernel headers), so one kernel family serves plain, causal (top-left or bottom-right), windowed
// and grouped packed calls, and a band that masks nothing runs the unmasked steady-state loop.
// The launchers (fa2_family_unit.h) get the stated maximum lengths as Nq / Nkv, which size the grids B * H * ceil(max_seqlen / rows); a workgroup whose
// block starts beyond its sequence's length returns at once.
// No hand-scheduled bodies, no KV-split, no longest-first order, no host-built work list (DESIGN has them as next steps).
#define FA2_WIN 1
#define FA2_VARLEN 1
#define FA2_FAMILY varlen
#include "fa2_family_unit.h"
