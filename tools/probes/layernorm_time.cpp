// layernorm_time.cpp — times the three LayerNormalization launches (csrc/layernorm_kernels.hip) at the
// RouteNet readout's shape, 1 254 400 rows x 256 units by default: device events around 20 launches
// after 3 warm-up launches, and the achieved bytes/s against the bytes each launch must move.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I ignnition_amd/csrc tools/probes/layernorm_time.cpp
//         ignnition_amd/csrc/layernorm_kernels.hip -o tools/probes/layernorm_time
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "layernorm_kernels.h"

#define CHECK(e)                                                                  \
  do {                                                                            \
    hipError_t _e = (e);                                                          \
    if (_e != hipSuccess) {                                                       \
      fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(_e));                     \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

int main(int argc, char** argv) {
  const int64_t n = argc > 1 ? atoll(argv[1]) : 1254400;
  const int units = argc > 2 ? atoi(argv[2]) : 256;
  const int reps = 20;
  const size_t elems = (size_t)n * units;
  std::vector<float> h(elems);
  uint32_t s = 12345u;
  for (auto& v : h) {
    s = s * 1664525u + 1013904223u;
    v = (float)(s >> 8) * (1.0f / 16777216.0f) - 0.5f;
  }
  float *x, *y, *g, *dx, *stats, *gamma, *beta, *part, *dgamma, *dbeta;
  CHECK(hipMalloc(&x, elems * 4));
  CHECK(hipMalloc(&y, elems * 4));
  CHECK(hipMalloc(&g, elems * 4));
  CHECK(hipMalloc(&dx, elems * 4));
  CHECK(hipMalloc(&stats, (size_t)n * 8));
  CHECK(hipMalloc(&gamma, units * 4));
  CHECK(hipMalloc(&beta, units * 4));
  CHECK(hipMalloc(&dgamma, units * 4));
  CHECK(hipMalloc(&dbeta, units * 4));
  CHECK(hipMalloc(&part, (size_t)layernorm_partial_floats(n, units) * 4 + 4));
  CHECK(hipMemcpy(x, h.data(), elems * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(g, h.data(), elems * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(gamma, h.data(), units * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(beta, h.data() + units, units * 4, hipMemcpyHostToDevice));
  CHECK(hipMemset(dgamma, 0, units * 4));
  CHECK(hipMemset(dbeta, 0, units * 4));
  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const double row_bytes = (double)elems * 4;
  struct Case {
    const char* name;
    double bytes;
  } cases[3] = {{"layernorm_fwd (with stats)", 2 * row_bytes + 8.0 * n},
                {"layernorm_bwd_dx", 3 * row_bytes + 8.0 * n},
                {"layernorm_bwd_params (both stages)", 2 * row_bytes + 8.0 * n}};
  for (int c = 0; c < 3; ++c) {
    for (int r = 0; r < 3 + reps; ++r) {
      if (r == 3) CHECK(hipEventRecord(e0, st));
      if (c == 0) CHECK(launch_layernorm_fwd(x, units, n, units, gamma, beta, 1e-3f, y, stats, st));
      if (c == 1) CHECK(launch_layernorm_bwd_dx(g, x, stats, gamma, n, units, dx, 0, st));
      if (c == 2) CHECK(launch_layernorm_bwd_params(g, x, stats, n, units, part, dgamma, dbeta, st));
    }
    CHECK(hipEventRecord(e1, st));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    ms /= reps;
    printf("%-36s %lld x %d: %.4f ms per launch, %.3f GB moved, %.2f TB/s\n", cases[c].name, (long long)n, units, ms,
           cases[c].bytes * 1e-9, cases[c].bytes / (ms * 1e-3) * 1e-12);
  }
  return 0;
}
