// dropout_kernels.h — launchers of the Dropout mask passes (dropout_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// z[i] = keep(seed, site, step, i) ? y[i] * scale : 0 over n flat elements of [rows][units]
// (dropout_rng.h: keep = uniform >= rate); z may be y
hipError_t launch_dropout_fwd(const float* y, float* z, int64_t n, float rate, float scale, uint64_t seed, uint32_t site,
                              uint32_t step, hipStream_t st);
// dy[i] = keep(...) ? dz[i] * scale : 0, the same mask; dy may be dz
hipError_t launch_dropout_bwd(const float* dz, float* dy, int64_t n, float rate, float scale, uint64_t seed,
                              uint32_t site, uint32_t step, hipStream_t st);
