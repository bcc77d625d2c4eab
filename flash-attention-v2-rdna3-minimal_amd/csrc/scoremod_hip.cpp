// scoremod_hip.cpp — logit soft-capping and ALiBi slopes for ONE dtype (fa2_fwd_scoremod / fa2_bwd_scoremod): the FA2_SMOD forms of the compiler-scheduled
// forward kernel and backward passes.  They are the sliding-window forms (FA2_WIN, window_hip.cpp) with the transform of fa2_scoremod.h applied to the
// scores between Q.K^T and the softmax, before the band's masks, so one kernel family serves plain (window = (-1, -1)), causal, windowed, offset and
// grouped calls.  The launchers (fa2_family_unit.h) take one further parameter here: the ScoreMod block (softcap, the slope pointer and its stride),
// which the kernels take as a further argument.
#define FA2_WIN 1
#define FA2_SMOD 1
#define FA2_FAMILY scoremod
#include "fa2_family_unit.h"
