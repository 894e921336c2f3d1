// learn_kernels.h — launchers of the loss, l2 and optimizer kernels (element-wise over the flat
// predictions / the flat parameter buffer).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the loss and optimizer kinds of the C ABI (enum ign_loss, enum ign_optimizer in ignmp.h)
#define IGN_K_LOSS_MSE 0
#define IGN_K_LOSS_MAE 1
#define IGN_K_LOSS_MAPE 2
#define IGN_K_LOSS_MSLE 3
#define IGN_K_LOSS_HUBER 4
#define IGN_K_LOSS_LOGCOSH 5
#define IGN_K_LOSS_BCE 6
#define IGN_K_LOSS_POISSON 7
#define IGN_K_OPT_ADAM 0
#define IGN_K_OPT_SGD 1
#define IGN_K_OPT_RMSPROP 2
#define IGN_K_OPT_ADAGRAD 3
#define IGN_K_OPT_ADADELTA 4
#define IGN_K_OPT_ADAMAX 5
// dpred = d(mean of the kind's element terms)/dpred ; part[b] = partial sums of the terms
// (MeanSquaredError: dpred = 2 (pred - label) / n, terms (pred - label)^2)
hipError_t launch_loss(int kind, const float* pred, const float* label, int64_t n, float* dpred, double* part,
                       int nblk, hipStream_t st);
// one element-wise update of w[n] from g[n]; slots: the kernel's three slot positions (see
// optimizer_kernel), nullptr where the configuration has none;
// lr: the rate with the step's bias correction folded in by the host
struct OptimizerLaunch {
  int kind;
  float* w;
  const float* g;
  float* slots[3];
  int64_t n;
  float lr, momentum, rho, b1, b2, eps;
  int nesterov, centered;
};
hipError_t launch_optimizer(const OptimizerLaunch& o, hipStream_t st);
// *count += the number of NaN / +-Inf among x[0..n) (x 4-byte aligned, n == 0: no launch)
hipError_t launch_nonfinite_count(const float* x, int64_t n, uint32_t* count, hipStream_t st);
// part[b] = partial sums of x^2
hipError_t launch_sumsq(const float* x, int64_t n, double* part, int nblk, hipStream_t st);
