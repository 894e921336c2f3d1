// layernorm_kernels.h — launchers of the LayerNormalization passes (layernorm_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

// y[r][j] = (x[r][j] - mean_r) * rstd_r * gamma[j] + beta[j] over n rows of `units` floats; x rows
// are ldx floats apart, y rows `units`.  mean_r = sum_j x / units, var_r = sum_j (x - mean_r)^2 /
// units (biased, over the centred values), rstd_r = 1.0f / sqrtf(var_r + epsilon).  gamma / beta
// null: 1 / 0.  stats non-null (training): stats[2 r] = mean_r, stats[2 r + 1] = rstd_r.  y must
// not be x.
hipError_t launch_layernorm_fwd(const float* x, int ldx, int64_t n, int units, const float* gamma, const float* beta,
                                float epsilon, float* y, float* stats, hipStream_t st);
// dx[r][j] (+)= rstd_r (g gamma - mean_j(g gamma) - xh mean_j(g gamma xh)), xh = (x - mean_r) rstd_r
// recomputed from x and stats; every row `units` floats apart.  acc 1: added to dx; 0: written (dx
// may be g).
hipError_t launch_layernorm_bwd_dx(const float* g, const float* x, const float* stats, const float* gamma, int64_t n,
                                   int units, float* dx, int acc, hipStream_t st);
// dgamma[j] += sum_r g[r][j] xh[r][j], dbeta[j] += sum_r g[r][j] (either may be null), in two
// fixed-order stages through part (layernorm_partial_floats(n, units) floats): per-workgroup partial
// column sums, then one ordered sum per column.  No atomics: the same bits on every run.
hipError_t launch_layernorm_bwd_params(const float* g, const float* x, const float* stats, int64_t n, int units,
                                       float* part, float* dgamma, float* dbeta, hipStream_t st);

// rows per stage-1 workgroup and the number of them: at most 1024 partial rows per column
inline int64_t layernorm_chunk_rows(int64_t n) { return std::max<int64_t>(256, (n + 1023) / 1024); }
inline int64_t layernorm_chunks(int64_t n) { return n > 0 ? (n + layernorm_chunk_rows(n) - 1) / layernorm_chunk_rows(n) : 0; }
inline int64_t layernorm_partial_floats(int64_t n, int units) { return layernorm_chunks(n) * 2 * units; }
