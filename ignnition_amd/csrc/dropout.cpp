// dropout.cpp — Dropout layers of the readout's Dense stacks behind the C ABI: the plan's site list
// (ign_plan_add_dropout; the list itself is plan_lower.cpp's add_dropout), a batch's mask stream (ign_batch_set_dropout) and the mask on the host
// (ign_dropout_keep).  The reference builds every layer with getattr(tf.keras.layers, type_layer)
// (AUX:869-1003) and calls the readout networks with training=(mode == TRAIN) (GM:612-629): a
// Dropout is tf.nn.dropout in training and the identity otherwise.  The kernels are
// dropout_kernels.hip; dense_stack.cpp runs them.
#include <cmath>

#include "dropout_rng.h"
#include "engine_internal.h"

namespace ign {

int plan_add_dropout(ign_plan* p, int stack, int before_layer, float rate, uint64_t layer_seed) {
  if (!p) return fail(IGN_ERR_INVALID, "null plan");
  if (p->batch_made)
    return fail(IGN_ERR_INVALID, "ign_plan_add_dropout after a batch of the plan was created (its training buffers "
                "are sized from the plan's sites)");
  return add_dropout(p, stack, before_layer, rate, layer_seed);
}

}  // namespace ign

extern "C" {

int ign_plan_add_dropout(ign_plan* plan, int32_t stack, int32_t before_layer, float rate, uint64_t layer_seed) {
  return plan_add_dropout(plan, stack, before_layer, rate, layer_seed);
}

int ign_batch_set_dropout(ign_batch* batch, uint64_t seed, uint32_t step) {
  if (!batch) return fail(IGN_ERR_INVALID, "null batch");
  batch->drop_seed = seed;
  batch->drop_step = step;
  return IGN_OK;
}

int ign_dropout_keep(uint64_t seed, int32_t site, uint32_t step, int64_t rows, int64_t units, float rate, uint8_t* out) {
  if (rows < 0 || units < 0 || site < 0 || (rows * units > 0 && !out)) return fail(IGN_ERR_INVALID, "ign_dropout_keep: bad argument");
  if (!(rate >= 0.f && rate < 1.f)) return fail(IGN_ERR_INVALID, "Dropout rate must be in [0, 1), got %g", (double)rate);
  const uint64_t n = (uint64_t)rows * (uint64_t)units;
  for (uint64_t g = 0; g * 4 < n; ++g) {
    const Philox4 r = dropout_words(seed, (uint32_t)site, step, g);
    for (uint64_t j = 0; j < 4 && g * 4 + j < n; ++j) out[g * 4 + j] = dropout_keep_word(r.w[j], rate) ? 1 : 0;
  }
  return IGN_OK;
}

}  // extern "C"
