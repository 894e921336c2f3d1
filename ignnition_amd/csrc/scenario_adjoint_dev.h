// scenario_adjoint_dev.h — what the scenario adjoint's kernel units share on the device and at launch
// (scenario_adjoint.hip: the input gradients; scenario_wgrad.hip: the parameter gradients,
// §3q): the sweep over launch_pack_a's transposed fragments, the coefficient tile's loads, the persistent grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "device_common.h"
#include "scenario_adjoint.h"

namespace {

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// acc[G][t] += sum over gate G's k range of A[16 t + .][G H + .] v[G][.]: A = pack_a fragments with MT
// row tiles and k over 3H ([MT][3H / 16][64] x f4), v the lane's [3][H / 16] B operand
template <int MT, int H>
__device__ __forceinline__ void sweep_t(const f4* A4, int lane, const f4 (&v)[3][H / 16], f4 (&acc)[3][MT]) {
  constexpr int NT = H / 16, K4 = 3 * NT;
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int G = 0; G < 3; ++G) {
        const f4 w = A4[(t * K4 + G * NT + i) * 64 + lane];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[G][t] = MFMA(w[q], v[G][i][q], acc[G][t]);
      }
}

// the lane's float4s of one coefficient tile: cf[q][i] = block q, row j, units 16 i + 4 g .. (p points at
// block 0, row j, unit 4 g)
template <int H>
__device__ __forceinline__ void load_tile(const float* p, f4 (&cf)[kScenCoef][H / 16]) {
#pragma unroll
  for (int q = 0; q < kScenCoef; ++q)
#pragma unroll
    for (int i = 0; i < H / 16; ++i) cf[q][i] = ld4(p + q * 16 * H + 16 * i);
}

// resident workgroups per CU x CUs, at most the work (a persistent grid), asked once per kernel
template <auto KERNEL>
int waves_grid(int64_t waves) {
  static const int64_t resident = [] {
    int dev = 0, cus = 0, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus <= 0) cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, KERNEL, 256, 0) != hipSuccess || per_cu <= 0) per_cu = 1;
    return (int64_t)per_cu * cus;
  }();
  return (int)std::max<int64_t>(1, std::min<int64_t>(resident, (waves + 3) / 4));
}

template <auto KERNEL, class Args>
hipError_t launch_waves(const Args& a, int64_t waves, hipStream_t st) {
  hipLaunchKernelGGL(KERNEL, dim3(waves_grid<KERNEL>(waves)), dim3(256), 0, st, a);
  return hipGetLastError();
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
