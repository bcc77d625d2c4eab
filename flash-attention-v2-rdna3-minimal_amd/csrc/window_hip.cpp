// window_hip.cpp — sliding-window (local) attention for ONE dtype (fa2_fwd_window / fa2_bwd_window): the FA2_WIN forms of the compiler-scheduled forward
// kernel and backward passes.  The window, causal flag already folded in, travels in the parameter block (set_window / get_window); the range arithmetic is
// fa2_window.h's.  fa2_family_unit.h has the launchers, which every family shares.
#define FA2_WIN 1
#define FA2_FAMILY window
#include "fa2_family_unit.h"
