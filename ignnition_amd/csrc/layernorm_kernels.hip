// layernorm_kernels.hip — Keras LayerNormalization over the last axis of [rows][units], for the
// readout's Dense stacks: the forward (inference and training), the input gradient and the
// gamma / beta gradients.
//
// Forward and input gradient stream each row once: a row lives in the registers of the TPR lanes
// that share it, EPL elements per lane, and its sums are __shfl_xor butterflies inside those lanes
// (every lane of a row ends with the same sum, formed in the same order on every run).
//   units <= 64    TPR = 16, 32 or 64 lanes per row, one element each: 4, 2 or 1 rows per wave
//   units <= 256   one row per wave, four elements per lane: one float4 where units % 4 == 0, the
//                  row stride is a multiple of 4 and the pointers are 16-byte aligned, else the
//                  columns lane, lane + 64, ...
//   wider          one row per wave, the lanes stride over the row once per sum and once to write
//                  (the row stays in cache between the passes)
// The variance is the mean of the squared centred values, and rstd = 1.0f / sqrtf(var + epsilon).
// A row of equal values centres to exact zeros and reads exactly beta.
//
// The gamma / beta gradients are column sums over every row: stage 1 gives each workgroup a chunk
// of rows and 64 columns and writes its partial sums, stage 2 adds a column's partials in chunk
// order.  No atomics anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "layernorm_kernels.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

struct LnFwdArgs {
  const float* x;
  int ldx;
  int64_t n;
  int units;
  const float *gamma, *beta;
  float eps;
  float* y;
  float* stats;
};

struct LnBwdArgs {
  const float *g, *x, *stats, *gamma;
  int64_t n;
  int units;
  float* dx;
  int acc;
};

// the sum over the TPR lanes of a row (TPR a power of two, rows aligned to it)
template <int TPR>
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = TPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The columns lane lr of a row holds: VEC: 4 lr .. 4 lr + 3 (one float4); else lr + TPR k.
template <int TPR, int EPL, bool VEC>
__device__ __forceinline__ int col_of(int lr, int k) {
  return VEC ? 4 * lr + k : lr + TPR * k;
}

template <int TPR, int EPL, bool VEC>
__device__ __forceinline__ void load_row(const float* p, int lr, int units, bool live, float (&v)[EPL]) {
  if constexpr (VEC) {
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live && 4 * lr < units) t = *reinterpret_cast<const float4*>(p + 4 * lr);
    v[0] = t.x;
    v[1 % EPL] = t.y;
    v[2 % EPL] = t.z;
    v[3 % EPL] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const int c = col_of<TPR, EPL, VEC>(lr, k);
      v[k] = live && c < units ? p[c] : 0.f;
    }
  }
}

template <int TPR, int EPL, bool VEC>
__device__ __forceinline__ void store_row(float* p, int lr, int units, bool live, const float (&v)[EPL], bool acc) {
  if constexpr (VEC) {
    if (live && 4 * lr < units) {
      float4 t = make_float4(v[0], v[1 % EPL], v[2 % EPL], v[3 % EPL]);
      if (acc) {
        const float4 o = *reinterpret_cast<const float4*>(p + 4 * lr);
        t.x += o.x;
        t.y += o.y;
        t.z += o.z;
        t.w += o.w;
      }
      *reinterpret_cast<float4*>(p + 4 * lr) = t;
    }
  } else {
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const int c = col_of<TPR, EPL, VEC>(lr, k);
      if (live && c < units) p[c] = acc ? p[c] + v[k] : v[k];
    }
  }
}

template <int TPR, int EPL, bool VEC>
__global__ __launch_bounds__(kBlock) void layernorm_fwd(LnFwdArgs a) {
  constexpr int RPW = 64 / TPR;
  const int lane = threadIdx.x & 63, lr = lane % TPR;
  const int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int64_t row = wave * RPW + lane / TPR;
  const bool live = row < a.n;   // every lane stays for the shuffles
  const int units = a.units;
  float v[EPL];
  load_row<TPR, EPL, VEC>(a.x + row * a.ldx, lr, units, live, v);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < EPL; ++k) s += v[k];
  const float mean = row_sum<TPR>(s) / (float)units;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < EPL; ++k) {
    v[k] = col_of<TPR, EPL, VEC>(lr, k) < units ? v[k] - mean : 0.f;
    q += v[k] * v[k];
  }
  const float var = row_sum<TPR>(q) / (float)units;
  const float rstd = 1.0f / sqrtf(var + a.eps);
#pragma unroll
  for (int k = 0; k < EPL; ++k) {
    const int c = col_of<TPR, EPL, VEC>(lr, k);
    if (c < units) {
      float y = v[k] * rstd;
      if (a.gamma) y *= a.gamma[c];
      if (a.beta) y += a.beta[c];
      v[k] = y;
    }
  }
  store_row<TPR, EPL, VEC>(a.y + row * units, lr, units, live, v, false);
  if (a.stats && live && lr == 0) {
    a.stats[2 * row] = mean;
    a.stats[2 * row + 1] = rstd;
  }
}

// units > 256: one row per wave, the lanes stride over it
__global__ __launch_bounds__(kBlock) void layernorm_fwd_wide(LnFwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const bool live = row < a.n;
  const int units = a.units;
  const float* x = a.x + row * a.ldx;
  float s = 0.f;
  for (int c = lane; live && c < units; c += 64) s += x[c];
  const float mean = row_sum<64>(s) / (float)units;
  float q = 0.f;
  for (int c = lane; live && c < units; c += 64) {
    const float d = x[c] - mean;
    q += d * d;
  }
  const float var = row_sum<64>(q) / (float)units;
  const float rstd = 1.0f / sqrtf(var + a.eps);
  float* y = a.y + row * units;
  for (int c = lane; live && c < units; c += 64) {
    float o = (x[c] - mean) * rstd;
    if (a.gamma) o *= a.gamma[c];
    if (a.beta) o += a.beta[c];
    y[c] = o;
  }
  if (a.stats && live && lane == 0) {
    a.stats[2 * row] = mean;
    a.stats[2 * row + 1] = rstd;
  }
}

template <int TPR, int EPL, bool VEC>
__global__ __launch_bounds__(kBlock) void layernorm_bwd_dx(LnBwdArgs a) {
  constexpr int RPW = 64 / TPR;
  const int lane = threadIdx.x & 63, lr = lane % TPR;
  const int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int64_t row = wave * RPW + lane / TPR;
  const bool live = row < a.n;
  const int units = a.units;
  float g[EPL], xh[EPL];
  load_row<TPR, EPL, VEC>(a.g + row * units, lr, units, live, g);
  load_row<TPR, EPL, VEC>(a.x + row * units, lr, units, live, xh);
  const float mean = live ? a.stats[2 * row] : 0.f, rstd = live ? a.stats[2 * row + 1] : 0.f;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < EPL; ++k) {
    const int c = col_of<TPR, EPL, VEC>(lr, k);
    const bool in = c < units;
    xh[k] = in ? (xh[k] - mean) * rstd : 0.f;
    g[k] = in ? (a.gamma ? g[k] * a.gamma[c] : g[k]) : 0.f;
    s1 += g[k];
    s2 += g[k] * xh[k];
  }
  const float m1 = row_sum<TPR>(s1) / (float)units, m2 = row_sum<TPR>(s2) / (float)units;
#pragma unroll
  for (int k = 0; k < EPL; ++k) g[k] = rstd * (g[k] - m1 - xh[k] * m2);
  store_row<TPR, EPL, VEC>(a.dx + row * units, lr, units, live, g, a.acc != 0);
}

__global__ __launch_bounds__(kBlock) void layernorm_bwd_dx_wide(LnBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const bool live = row < a.n;
  const int units = a.units;
  const float *g = a.g + row * units, *x = a.x + row * units;
  const float mean = live ? a.stats[2 * row] : 0.f, rstd = live ? a.stats[2 * row + 1] : 0.f;
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; live && c < units; c += 64) {
    const float gg = a.gamma ? g[c] * a.gamma[c] : g[c];
    s1 += gg;
    s2 += gg * ((x[c] - mean) * rstd);
  }
  const float m1 = row_sum<64>(s1) / (float)units, m2 = row_sum<64>(s2) / (float)units;
  float* dx = a.dx + row * units;
  for (int c = lane; live && c < units; c += 64) {   // each element is read before it is written: dx may be g
    const float gg = a.gamma ? g[c] * a.gamma[c] : g[c];
    const float d = rstd * (gg - m1 - (x[c] - mean) * rstd * m2);
    dx[c] = a.acc ? dx[c] + d : d;
  }
}

// stage 1: workgroup (chunk, column tile): thread (ty, tx) sums rows ty, ty + 4, ... of the chunk for
// column tile * 64 + tx; the four ty sums are added in order and written to part[chunk][2][units]
__global__ __launch_bounds__(kBlock) void layernorm_bwd_params_partial(const float* g, const float* x, const float* stats,
                                                                       int64_t n, int units, int64_t chunk_rows,
                                                                       float* part) {
  __shared__ float sg[kWaves][64], sb[kWaves][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + tx;
  const int64_t r0 = (int64_t)blockIdx.x * chunk_rows, r1 = min(n, r0 + chunk_rows);
  float dg = 0.f, db = 0.f;
  if (c < units)
#pragma unroll 4
    for (int64_t r = r0 + ty; r < r1; r += kWaves) {
      const float gv = g[r * units + c];
      dg += gv * ((x[r * units + c] - stats[2 * r]) * stats[2 * r + 1]);
      db += gv;
    }
  sg[ty][tx] = dg;
  sb[ty][tx] = db;
  __syncthreads();
  if (ty == 0 && c < units) {
    float* o = part + (int64_t)blockIdx.x * 2 * units;
    o[c] = ((sg[0][tx] + sg[1][tx]) + sg[2][tx]) + sg[3][tx];
    o[units + c] = ((sb[0][tx] + sb[1][tx]) + sb[2][tx]) + sb[3][tx];
  }
}

// stage 2: thread j < 2 units adds part[0 .. chunks)[j] in chunk order into dgamma (j < units) or dbeta
__global__ __launch_bounds__(kBlock) void layernorm_bwd_params_reduce(const float* part, int64_t chunks, int units,
                                                                      float* dgamma, float* dbeta) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= 2 * units) return;
  float* out = j < units ? dgamma : dbeta;
  if (!out) return;
  float s = 0.f;
  for (int64_t k = 0; k < chunks; ++k) s += part[k * 2 * units + j];
  out[j < units ? j : j - units] += s;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// blocks of kWaves waves, rpw rows per wave
dim3 row_grid(int64_t n, int rpw) { return dim3((unsigned)((n + (int64_t)kWaves * rpw - 1) / ((int64_t)kWaves * rpw))); }

template <typename Kernel, typename Args>
void launch_rows(Kernel kernel, int64_t n, int rpw, const Args& a, hipStream_t st) {
  hipLaunchKernelGGL(kernel, row_grid(n, rpw), dim3(kBlock), 0, st, a);
}

}  // namespace

hipError_t launch_layernorm_fwd(const float* x, int ldx, int64_t n, int units, const float* gamma, const float* beta,
                                float epsilon, float* y, float* stats, hipStream_t st) {
  if (n <= 0 || units <= 0) return hipSuccess;
  if (ldx < units) return hipErrorInvalidValue;
  const LnFwdArgs a{x, ldx, n, units, gamma, beta, epsilon, y, stats};
  if (units <= 16) launch_rows(layernorm_fwd<16, 1, false>, n, 4, a, st);
  else if (units <= 32) launch_rows(layernorm_fwd<32, 1, false>, n, 2, a, st);
  else if (units <= 64) launch_rows(layernorm_fwd<64, 1, false>, n, 1, a, st);
  else if (units > 256) launch_rows(layernorm_fwd_wide, n, 1, a, st);
  else if (units % 4 == 0 && ldx % 4 == 0 && aligned16(x) && aligned16(y)) launch_rows(layernorm_fwd<64, 4, true>, n, 1, a, st);
  else launch_rows(layernorm_fwd<64, 4, false>, n, 1, a, st);
  return hipGetLastError();
}

hipError_t launch_layernorm_bwd_dx(const float* g, const float* x, const float* stats, const float* gamma, int64_t n,
                                   int units, float* dx, int acc, hipStream_t st) {
  if (n <= 0 || units <= 0) return hipSuccess;
  const LnBwdArgs a{g, x, stats, gamma, n, units, dx, acc};
  if (units <= 16) launch_rows(layernorm_bwd_dx<16, 1, false>, n, 4, a, st);
  else if (units <= 32) launch_rows(layernorm_bwd_dx<32, 1, false>, n, 2, a, st);
  else if (units <= 64) launch_rows(layernorm_bwd_dx<64, 1, false>, n, 1, a, st);
  else if (units > 256) launch_rows(layernorm_bwd_dx_wide, n, 1, a, st);
  else if (units % 4 == 0 && aligned16(g) && aligned16(x) && aligned16(dx)) launch_rows(layernorm_bwd_dx<64, 4, true>, n, 1, a, st);
  else launch_rows(layernorm_bwd_dx<64, 4, false>, n, 1, a, st);
  return hipGetLastError();
}

hipError_t launch_layernorm_bwd_params(const float* g, const float* x, const float* stats, int64_t n, int units,
                                       float* part, float* dgamma, float* dbeta, hipStream_t st) {
  if (n <= 0 || units <= 0 || (!dgamma && !dbeta)) return hipSuccess;
  const int64_t chunks = layernorm_chunks(n);
  hipLaunchKernelGGL(layernorm_bwd_params_partial, dim3((unsigned)chunks, (unsigned)((units + 63) / 64)), dim3(kBlock), 0,
                     st, g, x, stats, n, units, layernorm_chunk_rows(n), part);
  hipLaunchKernelGGL(layernorm_bwd_params_reduce, dim3((unsigned)((2 * units + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                     part, chunks, units, dgamma, dbeta);
  return hipGetLastError();
}
