// cell_options.cpp — the GRU cell options behind the C ABI (ign_plan_set_cell_options).  The reference
// builds every update cell as getattr(tf.keras.layers, type + "Cell")(**parameters) (AUX:748-749); of
// GRUCell's keys the engine lowers activation, recurrent_activation, use_bias and reset_after.  The
// options enter the model in plan_lower.cpp's set_cell_options; the kernels are gru_cell.hip.
#include "engine_internal.h"

namespace ign {

// Like a LayerNormalization layer, the options change the parameter layout (the cell's bias tensor)
// and what a batch's training buffers are sized from.
int plan_set_cell_options(ign_plan* p, int cell, const ign_cell_options* o) {
  if (!p) return fail(IGN_ERR_INVALID, "null plan");
  if (p->batch_made)
    return fail(IGN_ERR_INVALID, "ign_plan_set_cell_options after a batch of the plan was created (its parameter and "
                "training buffers are sized from the cell options)");
  if (p->params_set || p->d_params)
    return fail(IGN_ERR_INVALID, "ign_plan_set_cell_options after the plan's parameters were set or placed on the device "
                "(the options decide the cell's bias tensor)");
  return set_cell_options(p, cell, o);
}

}  // namespace ign

extern "C" int ign_plan_set_cell_options(ign_plan* plan, int32_t cell, const ign_cell_options* options) {
  return plan_set_cell_options(plan, cell, options);
}
