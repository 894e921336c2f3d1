// learn_kernels.hip — gfx950 kernels of the loss, the l2 regularizer and the optimizer update:
// element-wise over the flat predictions / the flat parameter buffer, no MFMA, no LDS tiles.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "learn_kernels.h"

namespace {

// the block's sum of s (256 threads) in a fixed tree order, into part[blockIdx.x]
__device__ __forceinline__ void block_sum_to_part(double s, double* __restrict__ part) {
  __shared__ double red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ void sumsq_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ part) {
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    s += (double)x[i] * (double)x[i];
  block_sum_to_part(s, part);
}

// ---------------------------------------------------------------------------------------------
// The Keras losses (default constructor arguments, eps = 1e-7), each the mean over the n flat
// predictions of an element term; p = prediction, y = label, d = p - y.
// dpred[i] = dterm/dp / n in float32, the terms formed and summed in double
// (LogCosh's |d| + log1p(exp(-2|d|)) - log 2 and MSLE's difference of logarithms cancel in
// float32), one partial per block.  dpred uses the accurate float32 functions, and where the
// table's expression subtracts two nearly equal values it is rearranged so that the only
// subtraction is of the inputs themselves (exact or half an ulp in float32):
//   MSLE     lp - ly = log1p((p' - y') / (1 + y')),  p' = max(p, eps), y' = max(y, eps)
//   BCE      y / a - (1 - y) / b = ((y - q) - eps (1 - 2 y)) / (a b),  a = q + eps, b = 1 - q + eps
//   Poisson  1 - y / (p + eps) = ((p - y) + eps) / (p + eps)
// The comparisons against eps and 1 - eps are made in double: 1 - 1e-7 lies between the two
// largest floats below 1, so the float constant would move p = 1 - 2^-24 across the clip.
// MeanSquaredError squares the float32 difference and keeps its factor 2 in the scale
// (dpred = (2 / n) d), g = d.
template <int KIND>
__device__ __forceinline__ void loss_term(float p, float y, double& term, float& g) {
  constexpr double eps = 1e-7;
  constexpr float epsf = 1e-7f;
  const float d = p - y;
  const double dd = (double)p - (double)y;
  if constexpr (KIND == IGN_K_LOSS_MSE) {
    term = (double)d * (double)d;
    g = d;
  } else if constexpr (KIND == IGN_K_LOSS_MAE) {
    term = fabs(dd);
    g = p > y ? 1.f : p < y ? -1.f : 0.f;
  } else if constexpr (KIND == IGN_K_LOSS_MAPE) {
    term = 100.0 * fabs(dd) / fmax(fabs((double)y), eps);
    const float den = fabs((double)y) > eps ? fabsf(y) : epsf;
    g = p > y ? 100.f / den : p < y ? -100.f / den : 0.f;
  } else if constexpr (KIND == IGN_K_LOSS_MSLE) {
    const double l = log1p(fmax((double)p, eps)) - log1p(fmax((double)y, eps));
    term = l * l;
    if ((double)p > eps) {
      const float ys = (double)y > eps ? y : epsf;
      g = 2.f * log1pf((p - ys) / (1.f + ys)) / (1.f + p);
    } else {
      g = 0.f;
    }
  } else if constexpr (KIND == IGN_K_LOSS_HUBER) {
    const double a = fabs(dd);
    term = a <= 1.0 ? 0.5 * dd * dd : a - 0.5;
    g = fminf(fmaxf(d, -1.f), 1.f);
  } else if constexpr (KIND == IGN_K_LOSS_LOGCOSH) {
    const double a = fabs(dd);
    term = a + log1p(exp(-2.0 * a)) - 0.69314718055994530942;
    g = tanhf(d);
  } else if constexpr (KIND == IGN_K_LOSS_BCE) {
    const double q = fmin(fmax((double)p, eps), 1.0 - eps);
    term = -((double)y * log(q + eps) + (1.0 - (double)y) * log(1.0 - q + eps));
    if ((double)p > eps && (double)p < 1.0 - eps) {
      const float a = p + epsf, b = (1.f - p) + epsf;
      g = -((y - p) - epsf * (1.f - 2.f * y)) / (a * b);
    } else {
      g = 0.f;
    }
  } else {   // IGN_K_LOSS_POISSON
    term = (double)p - (double)y * log((double)p + eps);
    g = (d + epsf) / (p + epsf);
  }
}

template <int KIND>
__global__ void loss_kernel(const float* __restrict__ pred, const float* __restrict__ label, int64_t n,
                            float* __restrict__ dpred, double* __restrict__ part) {
  double s = 0.0;
  const float sc = (KIND == IGN_K_LOSS_MSE ? 2.0f : 1.0f) / (float)n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double term;
    float g;
    loss_term<KIND>(pred[i], label[i], term, g);
    dpred[i] = sc * g;
    s += term;
  }
  block_sum_to_part(s, part);
}

// ---------------------------------------------------------------------------------------------
// The Keras optimizers (optimizer_v2 / training_ops semantics), element-wise over the flat
// parameter buffer; s0 .. s2: the caller's slot buffers in ign_optimizer_num_slots' order.
// Step-dependent factors come from the host (Adam: lr = lr sqrt(1 - beta_2^t) / (1 - beta_1^t),
// Adamax: lr = lr / (1 - beta_1^t)).
//   Adam      s0 = m, s1 = v (training_ops.ApplyAdam).  m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2;
//             w -= lr m / (sqrt(v) + eps)
//   SGD       s0 = v (momentum > 0).  v = momentum v - lr g; w += nesterov ? momentum v - lr g : v
//   RMSprop   s0 = rms, then mg (centered), then mom (momentum > 0).  rms = rho rms + (1 - rho) g^2;
//             den = centered ? max(rms - mg^2, 0) : rms;  momentum 0: w -= lr g / (sqrt(den) + eps),
//             else mom = momentum mom + lr g / sqrt(den + eps), w -= mom (Keras' two epsilons).
//             The clamp at 0 departs from Keras only where rounding makes rms - mg^2 negative
//             and Keras' square root gives NaN.
//   Adagrad   s0 = acc (starts at initial_accumulator_value).  acc += g^2; w -= lr g / (sqrt(acc) + eps)
//   Adadelta  s0 = acc, s1 = accu.  acc = rho acc + (1 - rho) g^2; u = sqrt(accu + eps) / sqrt(acc + eps) g;
//             accu = rho accu + (1 - rho) u^2; w -= lr u
//   Adamax    s0 = m, s1 = u.  m = b1 m + (1 - b1) g; u = max(b2 u, |g|); w -= lr m / (u + eps)
// Each maps g = 0 with fresh slots to an update of +0, so the zero alignment gaps of the buffer stay zero.
struct OptArgs {
  float* w;
  const float* g;
  float* s0;
  float* s1;
  float* s2;
  int64_t n;
  float lr, momentum, rho, b1, b2, eps;
  int nesterov, centered;
};

template <int KIND>
__global__ void optimizer_kernel(OptArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
    const float g = a.g[i];
    if constexpr (KIND == IGN_K_OPT_ADAM) {
      const float m = a.b1 * a.s0[i] + (1.f - a.b1) * g;
      const float v = a.b2 * a.s1[i] + (1.f - a.b2) * g * g;
      a.s0[i] = m;
      a.s1[i] = v;
      a.w[i] -= a.lr * m / (sqrtf(v) + a.eps);
    } else if constexpr (KIND == IGN_K_OPT_SGD) {
      if (a.s0) {
        const float v = a.momentum * a.s0[i] - a.lr * g;
        a.s0[i] = v;
        a.w[i] += a.nesterov ? a.momentum * v - a.lr * g : v;
      } else {
        a.w[i] -= a.lr * g;
      }
    } else if constexpr (KIND == IGN_K_OPT_RMSPROP) {
      const float rms = a.rho * a.s0[i] + (1.f - a.rho) * g * g;
      a.s0[i] = rms;
      float den = rms;
      if (a.centered) {
        const float mg = a.rho * a.s1[i] + (1.f - a.rho) * g;
        a.s1[i] = mg;
        den = fmaxf(rms - mg * mg, 0.f);
      }
      if (a.s2) {
        const float mom = a.momentum * a.s2[i] + a.lr * g / sqrtf(den + a.eps);
        a.s2[i] = mom;
        a.w[i] -= mom;
      } else {
        a.w[i] -= a.lr * g / (sqrtf(den) + a.eps);
      }
    } else if constexpr (KIND == IGN_K_OPT_ADAGRAD) {
      const float acc = a.s0[i] + g * g;
      a.s0[i] = acc;
      a.w[i] -= a.lr * g / (sqrtf(acc) + a.eps);
    } else if constexpr (KIND == IGN_K_OPT_ADADELTA) {
      const float acc = a.rho * a.s0[i] + (1.f - a.rho) * g * g;
      a.s0[i] = acc;
      const float accu = a.s1[i];
      const float u = sqrtf(accu + a.eps) / sqrtf(acc + a.eps) * g;
      a.s1[i] = a.rho * accu + (1.f - a.rho) * u * u;
      a.w[i] -= a.lr * u;
    } else {   // IGN_K_OPT_ADAMAX
      const float m = a.b1 * a.s0[i] + (1.f - a.b1) * g;
      const float u = fmaxf(a.b2 * a.s1[i], fabsf(g));
      a.s0[i] = m;
      a.s1[i] = u;
      a.w[i] -= a.lr * m / (u + a.eps);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The non-finite guard: *count += the number of NaN / +-Inf among x[0..n).  A value is non-finite
// when its exponent field is all ones; the test is on the bit pattern, so no floating-point
// option of the compiler can fold it.  x + head is 16-byte aligned: the nvec float4 of the body
// are read as such (grid-stride), the head scalars before it and the tail (< 4) scalars after it
// by the first head + tail threads of the grid.  Each wave sums its lanes' counts, the block its
// four waves', and a block that found any adds its sum with one atomic: an integer sum, the same
// in any order.
__device__ __forceinline__ uint32_t nonfinite_bits(float v) {
  return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u ? 1u : 0u;
}

__global__ void nonfinite_kernel(const float* __restrict__ x, int64_t head, int64_t nvec, int64_t tail,
                                 uint32_t* __restrict__ count) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float4* __restrict__ body = reinterpret_cast<const float4*>(x + head);
  uint32_t c = 0;
  for (int64_t i = tid; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 q = body[i];
    c += nonfinite_bits(q.x) + nonfinite_bits(q.y) + nonfinite_bits(q.z) + nonfinite_bits(q.w);
  }
  if (tid < head)
    c += nonfinite_bits(x[tid]);
  else if (tid < head + tail)
    c += nonfinite_bits(x[head + 4 * nvec + (tid - head)]);
  for (int o = warpSize / 2; o > 0; o >>= 1) c += __shfl_down(c, o);
  __shared__ uint32_t wave_sum[256 / 64];
  if ((threadIdx.x & (warpSize - 1)) == 0) wave_sum[threadIdx.x / warpSize] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < (int)(blockDim.x / warpSize); ++w) s += wave_sum[w];
    if (s) atomicAdd(count, s);
  }
}

}  // namespace

hipError_t launch_nonfinite_count(const float* x, int64_t n, uint32_t* count, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  // scalars up to the first 16-byte boundary (x is 4-byte aligned), then whole float4, then the rest
  const int64_t head = std::min<int64_t>(n, (int64_t)(((16 - ((uintptr_t)x & 15)) & 15) / 4));
  const int64_t nvec = (n - head) / 4;
  const int64_t tail = n - head - 4 * nvec;
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((nvec + 255) / 256, 256)));
  hipLaunchKernelGGL(nonfinite_kernel, grid, dim3(256), 0, st, x, head, nvec, tail, count);
  return hipGetLastError();
}

hipError_t launch_loss(int kind, const float* pred, const float* label, int64_t n, float* dpred, double* part,
                       int nblk, hipStream_t st) {
  switch (kind) {
#define LOSS_CASE(K) \
    case K: hipLaunchKernelGGL(loss_kernel<K>, dim3(nblk), dim3(256), 0, st, pred, label, n, dpred, part); break;
    LOSS_CASE(IGN_K_LOSS_MSE)
    LOSS_CASE(IGN_K_LOSS_MAE)
    LOSS_CASE(IGN_K_LOSS_MAPE)
    LOSS_CASE(IGN_K_LOSS_MSLE)
    LOSS_CASE(IGN_K_LOSS_HUBER)
    LOSS_CASE(IGN_K_LOSS_LOGCOSH)
    LOSS_CASE(IGN_K_LOSS_BCE)
    LOSS_CASE(IGN_K_LOSS_POISSON)
#undef LOSS_CASE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_optimizer(const OptimizerLaunch& o, hipStream_t st) {
  if (o.n == 0) return hipSuccess;
  OptArgs a{o.w, o.g, o.slots[0], o.slots[1], o.slots[2], o.n, o.lr, o.momentum, o.rho, o.b1, o.b2, o.eps,
            o.nesterov, o.centered};
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((o.n + 255) / 256, 16384)));
  switch (o.kind) {
#define OPT_CASE(K) \
    case K: hipLaunchKernelGGL(optimizer_kernel<K>, grid, dim3(256), 0, st, a); break;
    OPT_CASE(IGN_K_OPT_ADAM)
    OPT_CASE(IGN_K_OPT_SGD)
    OPT_CASE(IGN_K_OPT_RMSPROP)
    OPT_CASE(IGN_K_OPT_ADAGRAD)
    OPT_CASE(IGN_K_OPT_ADADELTA)
    OPT_CASE(IGN_K_OPT_ADAMAX)
#undef OPT_CASE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_sumsq(const float* x, int64_t n, double* part, int nblk, hipStream_t st) {
  hipLaunchKernelGGL(sumsq_kernel, dim3(nblk), dim3(256), 0, st, x, n, part);
  return hipGetLastError();
}
