// layernorm.cpp — LayerNormalization layers of the readout's Dense stacks behind the C ABI
// (ign_plan_add_layernorm).  The reference builds every layer with getattr(tf.keras.layers,
// type_layer) (AUX:869-1003); a LayerNormalization keeps no moving statistics, so ign_forward and the
// training forward run the same arithmetic.  The site list and the layouts are plan_lower.cpp's
// add_layernorm, the kernels layernorm_kernels.hip; dense_stack.cpp and the inference readout run them.
#include "engine_internal.h"

namespace ign {

int plan_add_layernorm(ign_plan* p, int stack, int before_layer, float epsilon, int center, int scale) {
  if (!p) return fail(IGN_ERR_INVALID, "null plan");
  if (p->batch_made)
    return fail(IGN_ERR_INVALID, "ign_plan_add_layernorm after a batch of the plan was created (its buffers are sized "
                "from the plan's layers)");
  if (p->params_set || p->d_params)
    return fail(IGN_ERR_INVALID, "ign_plan_add_layernorm after the plan's parameters were set or placed on the device "
                "(the layer adds tensors to the parameter layout)");
  return add_layernorm(p, stack, before_layer, epsilon, center, scale);
}

}  // namespace ign

extern "C" int ign_plan_add_layernorm(ign_plan* plan, int32_t stack, int32_t before_layer, float epsilon, int32_t center,
                                      int32_t scale) {
  return plan_add_layernorm(plan, stack, before_layer, epsilon, center, scale);
}
