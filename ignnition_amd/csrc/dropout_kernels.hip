// dropout_kernels.hip — the Dropout layers of the readout's Dense stacks in training
// (tf.nn.dropout as Keras calls it with training=True): z = keep ? y / (1 - rate) : 0 and the same
// mask on the gradient.  The mask is dropout_rng.h's pure function of (seed, site, step, element);
// nothing is stored between the forward and the backward.
//
// Both are memory-bound passes over [rows][units] as a flat array: one thread per group of four
// consecutive elements, one Philox call per group, a float4 load and store where both pointers are
// 16-byte aligned and the group is whole, scalar accesses for the tail group (and for unaligned
// pointers).  A dropped element is selected to 0, never multiplied by 0: inf or NaN under the mask
// gives 0.  in and out may be the same buffer (no __restrict__).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dropout_kernels.h"
#include "dropout_rng.h"

namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxBlocks = 1 << 20;

struct DropArgs {
  const float* in;
  float* out;
  int64_t n;          // elements
  float rate, scale;
  uint64_t seed;      // the batch's stream seed xor the layer's own
  uint32_t site, step;
  int vec;            // 1: in and out are 16-byte aligned
};

__device__ __forceinline__ float masked(float v, uint32_t word, float rate, float scale) {
  return ign::dropout_keep_word(word, rate) ? v * scale : 0.0f;
}

__device__ __forceinline__ void dropout_body(const DropArgs& a) {
  const int64_t groups = (a.n + 3) >> 2;
  for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kBlock) {
    const ign::Philox4 r = ign::dropout_words(a.seed, a.site, a.step, (uint64_t)g);
    const int64_t i = g << 2;
    if (a.vec && i + 4 <= a.n) {
      const float4 v = *reinterpret_cast<const float4*>(a.in + i);
      float4 o;
      o.x = masked(v.x, r.w[0], a.rate, a.scale);
      o.y = masked(v.y, r.w[1], a.rate, a.scale);
      o.z = masked(v.z, r.w[2], a.rate, a.scale);
      o.w = masked(v.w, r.w[3], a.rate, a.scale);
      *reinterpret_cast<float4*>(a.out + i) = o;
    } else {
      for (int j = 0; j < 4; ++j)
        if (i + j < a.n) a.out[i + j] = masked(a.in[i + j], r.w[j], a.rate, a.scale);
    }
  }
}

// z = mask(y): the training forward
__global__ __launch_bounds__(kBlock) void dropout_fwd(DropArgs a) { dropout_body(a); }
// dy = mask(dz): the same mask on the gradient
__global__ __launch_bounds__(kBlock) void dropout_bwd(DropArgs a) { dropout_body(a); }

DropArgs make_args(const float* in, float* out, int64_t n, float rate, float scale, uint64_t seed, uint32_t site,
                   uint32_t step) {
  const int vec = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  return DropArgs{in, out, n, rate, scale, seed, site, step, vec};
}

// a grid over the element groups (grid-stride beyond kMaxBlocks blocks)
dim3 grid_for(int64_t n) { return dim3((unsigned)std::min<int64_t>(((n + 3) / 4 + kBlock - 1) / kBlock, kMaxBlocks)); }

}  // namespace

hipError_t launch_dropout_fwd(const float* y, float* z, int64_t n, float rate, float scale, uint64_t seed, uint32_t site,
                              uint32_t step, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(dropout_fwd, grid_for(n), dim3(kBlock), 0, st, make_args(y, z, n, rate, scale, seed, site, step));
  return hipGetLastError();
}

hipError_t launch_dropout_bwd(const float* dz, float* dy, int64_t n, float rate, float scale, uint64_t seed,
                              uint32_t site, uint32_t step, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(dropout_bwd, grid_for(n), dim3(kBlock), 0, st, make_args(dz, dy, n, rate, scale, seed, site, step));
  return hipGetLastError();
}
