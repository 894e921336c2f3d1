// learn.cpp — loss, regularizer and optimizer update behind the C ABI: what model_fn's TRAIN branch
// (code/utils/generate_model.py:697-830 = GM) does around tf.gradients.
//
//   ign_loss            the Keras losses a description may name (GM:716-753), by kind, over the
//                       batch's flat predictions; ign_mse_loss is its kind 0
//   ign_l2_loss         the Dense l2 kernel regularizers (AUX:833-834)
//   ign_optimizer_step  the Keras optimizers (Adam, SGD, RMSprop, Adagrad, Adadelta, Adamax), by
//                       desc, with the host-evaluated rate (GM:797-818); ign_adam_step is its kind 0
//                       with loose hyper-parameters
//   ign_loss_kind / ign_optimizer_kind   the one name table (no GPU)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "learn_kernels.h"

namespace {

constexpr int kRedMax = 1024;   // partial sums a reduction may leave in d_red

// the plan's reduction buffer, allocated on first use
int red_buffer(ign_plan* p, double** out) {
  if (!p->d_red) HIP_TRY(hipMalloc(&p->d_red, kRedMax * sizeof(double)));
  *out = p->d_red;
  return IGN_OK;
}

// the sum of the nb partials a kernel on the plan's stream left in d_red, in index order (waits)
int red_sum(ign_plan* p, int nb, double* sum) {
  double h[kRedMax];
  HIP_TRY(hipMemcpyAsync(h, p->d_red, nb * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  double s = 0;
  for (int i = 0; i < nb; ++i) s += h[i];
  *sum = s;
  return IGN_OK;
}

// the one name table of the lowered Keras losses / optimizers (index = kind)
const char* const kLossNames[] = {"MeanSquaredError", "MeanAbsoluteError", "MeanAbsolutePercentageError",
                                  "MeanSquaredLogarithmicError", "Huber", "LogCosh", "BinaryCrossentropy",
                                  "Poisson"};
const char* const kOptimizerNames[] = {"Adam", "SGD", "RMSprop", "Adagrad", "Adadelta", "Adamax"};

int kind_of(const char* what, const char* const* names, size_t N, const char* name, int32_t* kind) {
  if (!name || !kind) return fail(IGN_ERR_INVALID, "null argument");
  std::string all;
  for (size_t i = 0; i < N; ++i) {
    if (!std::strcmp(name, names[i])) {
      *kind = (int32_t)i;
      return IGN_OK;
    }
    all += (i ? ", " : "") + std::string(names[i]);
  }
  return fail(IGN_ERR_UNSUPPORTED, "%s \"%s\" is not lowered (%s)", what, name, all.c_str());
}

}  // namespace

extern "C" {

int ign_loss_kind(const char* name, int32_t* kind) {
  return kind_of("loss", kLossNames, sizeof(kLossNames) / sizeof(kLossNames[0]), name, kind);
}

int ign_optimizer_kind(const char* name, int32_t* kind) {
  return kind_of("optimizer", kOptimizerNames, sizeof(kOptimizerNames) / sizeof(kOptimizerNames[0]), name, kind);
}

int ign_loss(ign_plan* p, int32_t kind, const float* pred, const float* labels, int64_t n, float* dpred, double* loss) {
  if (!p || !pred || !labels || !dpred) return fail(IGN_ERR_INVALID, "null argument");
  if (kind < 0 || kind > IGN_LOSS_POISSON) return fail(IGN_ERR_INVALID, "loss kind %d out of range", (int)kind);
  if (n <= 0) return fail(IGN_ERR_INVALID, "empty prediction vector");
  int rc = ensure_device(p);
  if (rc) return rc;
  constexpr int NB = 256;
  double* red;
  if ((rc = red_buffer(p, &red))) return rc;
  HIP_TRY(launch_loss(kind, pred, labels, n, dpred, red, NB, p->stream));
  if (loss) {
    double s;
    if ((rc = red_sum(p, NB, &s))) return rc;
    *loss = s / (double)n;
  }
  return IGN_OK;
}

int ign_mse_loss(ign_plan* p, const float* pred, const float* labels, int64_t n, float* dpred, double* loss) {
  return ign_loss(p, IGN_LOSS_MEAN_SQUARED_ERROR, pred, labels, n, dpred, loss);
}

int ign_l2_loss(ign_plan* p, double* loss) {
  if (!p || !loss) return fail(IGN_ERR_INVALID, "null argument");
  if (!p->params_set) return fail(IGN_ERR_INVALID, "parameters not set (ign_plan_set_params)");
  int rc = ensure_device(p);
  if (rc) return rc;
  constexpr int NB = 64;
  double* red;
  if ((rc = red_buffer(p, &red))) return rc;
  double total = 0;
  std::vector<const DenseP*> layers;   // readout and message-network Dense layers (model.losses)
  for (auto& d : p->dense) layers.push_back(&d);
  for (auto& mp : p->mps)
    for (auto& nn : mp.nn)
      for (auto& d : nn.layers) layers.push_back(&d);
  for (const DenseP* dl : layers) {
    const DenseP& d = *dl;
    if (d.l2 == 0.f) continue;
    HIP_TRY(launch_sumsq(p->d_params + d.off_w, (int64_t)d.in * d.out, red, NB, p->stream));
    double s;
    if ((rc = red_sum(p, NB, &s))) return rc;
    total += (double)d.l2 * s;
  }
  *loss = total;
  return IGN_OK;
}

int ign_optimizer_num_slots(const ign_optimizer_desc* d, int32_t* n, float* init_value) {
  if (!d || !n) return fail(IGN_ERR_INVALID, "null argument");
  float init = 0.f;
  switch (d->kind) {
    case IGN_OPT_ADAM: *n = 2; break;
    case IGN_OPT_SGD: *n = d->momentum > 0.f ? 1 : 0; break;
    case IGN_OPT_RMSPROP: *n = 1 + (d->centered ? 1 : 0) + (d->momentum > 0.f ? 1 : 0); break;
    case IGN_OPT_ADAGRAD:
      *n = 1;
      init = d->initial_accumulator_value;
      break;
    case IGN_OPT_ADADELTA: *n = 2; break;
    case IGN_OPT_ADAMAX: *n = 2; break;
    default: return fail(IGN_ERR_INVALID, "optimizer kind %d out of range", (int)d->kind);
  }
  if (init_value) *init_value = init;
  return IGN_OK;
}

int ign_optimizer_step(ign_plan* p, const ign_optimizer_desc* d, const float* grads, float* const* slots,
                       int32_t n_slots, int64_t iteration, float lr) {
  if (!p || !d || !grads) return fail(IGN_ERR_INVALID, "null argument");
  int32_t need = 0;
  int rc = ign_optimizer_num_slots(d, &need, nullptr);
  if (rc) return rc;
  if (d->reserved != 0) return fail(IGN_ERR_INVALID, "ign_optimizer_desc.reserved must be 0");
  if (n_slots != need) return fail(IGN_ERR_INVALID, "optimizer takes %d slot buffer(s), %d given", (int)need, (int)n_slots);
  if (need && !slots) return fail(IGN_ERR_INVALID, "null argument");
  for (int i = 0; i < need; ++i)
    if (!slots[i]) return fail(IGN_ERR_INVALID, "slot buffer %d is null", i);
  if (!p->params_set) return fail(IGN_ERR_INVALID, "parameters not set (ign_plan_set_params)");
  if (iteration < 0) return fail(IGN_ERR_INVALID, "negative iteration");
  rc = ensure_device(p);
  if (rc) return rc;
  OptimizerLaunch o{};
  o.kind = d->kind;
  o.w = p->d_params;
  o.g = grads;
  o.n = p->n_params;
  o.lr = lr;
  o.momentum = d->momentum;
  o.rho = d->rho;
  o.b1 = d->beta_1;
  o.b2 = d->beta_2;
  o.eps = d->epsilon;
  o.nesterov = d->nesterov != 0;
  o.centered = d->centered != 0;
  if (d->kind == IGN_OPT_RMSPROP) {   // the kernel's positions: rms, mg, mom
    int k = 0;
    o.slots[0] = slots[k++];
    if (d->centered) o.slots[1] = slots[k++];
    if (d->momentum > 0.f) o.slots[2] = slots[k++];
  } else {
    for (int i = 0; i < need; ++i) o.slots[i] = slots[i];
  }
  // the bias corrections depend on the step only: host, double
  const double tstep = (double)iteration + 1.0;
  if (d->kind == IGN_OPT_ADAM)
    o.lr = (float)((double)lr * std::sqrt(1.0 - std::pow((double)d->beta_2, tstep)) / (1.0 - std::pow((double)d->beta_1, tstep)));
  else if (d->kind == IGN_OPT_ADAMAX)
    o.lr = (float)((double)lr / (1.0 - std::pow((double)d->beta_1, tstep)));
  HIP_TRY(launch_optimizer(o, p->stream));
  return repack(p);
}

int ign_nonfinite_count(ign_plan* p, const float* dev, int64_t n, uint32_t* dev_count) {
  if (!p || !dev || !dev_count) return fail(IGN_ERR_INVALID, "null argument");
  if (n < 0) return fail(IGN_ERR_INVALID, "negative element count");
  if (((uintptr_t)dev & 3) || ((uintptr_t)dev_count & 3))
    return fail(IGN_ERR_INVALID, "ign_nonfinite_count: pointers must be 4-byte aligned");
  if (n == 0) return IGN_OK;
  int rc = ensure_device(p);
  if (rc) return rc;
  HIP_TRY(launch_nonfinite_count(dev, n, dev_count, p->stream));
  return IGN_OK;
}

int ign_adam_step(ign_plan* p, const float* grads, float* m, float* v, int64_t iteration, float lr, float beta1,
                  float beta2, float epsilon) {
  if (!p || !grads || !m || !v) return fail(IGN_ERR_INVALID, "null argument");
  ign_optimizer_desc d{};
  d.kind = IGN_OPT_ADAM;
  d.beta_1 = beta1;
  d.beta_2 = beta2;
  d.epsilon = epsilon;
  float* const slots[2] = {m, v};
  return ign_optimizer_step(p, &d, grads, slots, 2, iteration, lr);
}

}  // extern "C"
