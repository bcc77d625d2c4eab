// dropout_hip.cpp — attention dropout for ONE dtype (fa2_fwd_dropout / fa2_bwd_dropout): the FA2_DROP forms of the compiler-scheduled forward kernel and
// backward passes.  They are the sliding-window forms (FA2_WIN, window_hip.cpp) with the Philox keep mask of fa2_dropout.h applied to the probabilities
// after the softmax, so one kernel family serves plain (window = (-1, -1)), causal, windowed, offset and grouped dropout calls.  The host puts the seed
// and the threshold into the parameter block (set_dropout) before it calls the launchers (fa2_family_unit.h).
#define FA2_WIN 1
#define FA2_DROP 1
#define FA2_FAMILY dropout
#include "fa2_family_unit.h"
