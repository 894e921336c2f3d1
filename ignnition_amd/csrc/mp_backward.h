// mp_backward.h — the backward of one message-passing (MP) instance, mp_step.h's mirror: for
// ign_backward_mp (train.cpp), which picks the instance's record and flips the destination's
// gradient buffer afterwards.
#pragma once
#include "train_state.h"

namespace ign {

// MP instance rec of the last forward: dLoss/d(its output version), in the destination's current
// gradient buffer, into dLoss/d(its input version) in the other one; the message gradients added to
// its sources' buffers, the parameter gradients to t->grads (or parked in the deferred slots).
int mp_backward(ign_plan* p, ign_batch* b, TrainState* t, const MPRec& rec);

}  // namespace ign
