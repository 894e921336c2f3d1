// dropout.cpp — Dropout layers of the readout's Dense stacks behind the C ABI: the plan's site list
// (ign_plan_add_dropout), a batch's mask stream (ign_batch_set_dropout) and the mask on the host
// (ign_dropout_keep).  The reference builds every layer with getattr(tf.keras.layers, type_layer)
// (AUX:869-1003) and calls the readout networks with training=(mode == TRAIN) (GM:612-629): a
// Dropout is tf.nn.dropout in training and the identity otherwise.  The kernels are
// dropout_kernels.hip; dense_stack.cpp runs them.
#include <climits>
#include <cmath>

#include "dropout_rng.h"
#include "engine_internal.h"

namespace ign {

int plan_add_dropout(ign_plan* p, int stack, int before_layer, float rate, uint64_t layer_seed) {
  if (!p) return fail(IGN_ERR_INVALID, "null plan");
  if (p->batch_made)
    return fail(IGN_ERR_INVALID, "ign_plan_add_dropout after a batch of the plan was created (its training buffers "
                "are sized from the plan's sites)");
  int layers;
  if (stack == -1) {
    layers = (int)p->dense.size();
  } else {
    if (stack < 0 || stack >= (int)p->ro_ops.size() || p->ro_ops[stack].type != IGN_RO_NEURAL_NETWORK)
      return fail(IGN_ERR_INVALID, "ign_plan_add_dropout: stack %d is neither -1 (predict) nor a readout "
                  "neural_network operation", stack);
    layers = (int)p->ro_ops[stack].layers.size();
  }
  if (before_layer < 0 || before_layer > layers)
    return fail(IGN_ERR_INVALID, "ign_plan_add_dropout: before_layer %d outside 0..%d", before_layer, layers);
  if (!(rate >= 0.f && rate < 1.f))   // tf.nn.dropout raises ValueError
    return fail(IGN_ERR_INVALID, "Dropout rate must be in [0, 1), got %g", (double)rate);
  if (rate == 0.f) return IGN_OK;   // tf.nn.dropout returns x: no layer, no site
  DropSite d;
  d.stack = stack;
  d.before = before_layer;
  d.rate = rate;
  d.scale = dropout_scale(rate);
  d.seed = layer_seed;
  d.order = sites_in_front(p, stack, before_layer);
  auto key = [](const DropSite& s) { return std::make_pair(s.stack < 0 ? INT_MAX : s.stack, s.before); };
  size_t at = 0;
  while (at < p->drops.size() && key(p->drops[at]) <= key(d)) ++at;
  p->drops.insert(p->drops.begin() + at, d);
  return IGN_OK;
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
