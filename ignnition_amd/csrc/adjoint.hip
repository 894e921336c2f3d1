// adjoint.hip — K prediction cotangents through one adjoint sweep of the linearised forward, on f32
// MFMA (v_mfma_f32_16x16x4_f32), behind ign_backward_jacobian.
//
// jacobian.hip's linearising primal leaves per real GRU step the rows (z, P, R, Q, S) of the linear update
//   hd' = z hd + P (ad_z + hd.U_z) + R (ad_r + hd.U_r) + Q ad_h + S (hd.U_h)
// Its transpose, l' the cotangent of the state after the step:
//   abar = [P l' | R l' | Q l']                 cotangent of the step's x.W row (3H)
//   l    = z l' + [P l' | R l' | S l'] . U^T    one contraction, k = 3H -> H
// Layout as §3n with the tile's 16 rows on the COTANGENT axis: a wave owns (order position, cotangent
// block), so every lane of a tile is the same destination: the coefficient rows are broadcast float4s,
// there is no mask and no select, and a lane's four units of P l' .. S l' are already the B operand of the
// sweep over U^T (k(s4, g, q) = 16 s4 + 4 g + q, s4 = gate * H/16 + tile: the accumulator layout).  The
// A operand is launch_pack_a's fragments of the raw U [H][3H]: tiles over the H state units, k over 3H,
// in LDS once per workgroup.  The three gates' k ranges run into three accumulator sets (independent
// MFMA chains), z l' starts the first, and the sets are added in one order.
// Nothing is scattered: a cell kernel stores its step / destination cotangent blocks, and every source
// row then adds the blocks its transposed CSR lists, in the list's order, in src_adj_kernel -- for the
// ordered update through W^T on the way (the [16][3H] sum is again a B operand), so the per-step blocks
// are read once and no [rows][Kp][3H] intermediate exists.
// Every operation is linear in the cotangent and an MFMA column depends on its own B column only: zero
// cotangents give zeros, a power-of-two scale commutes with every rounding, and a cotangent's bits
// depend neither on K, nor on its index, nor on the chunk of blocks a launch covers.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "adjoint.h"
#include "device_common.h"

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

// ---------------------------------------------------------------------------------------------
// Adjoint of the ordered update.  One wave per (order position, cotangent block) for the whole
// sequence, last step first: l in registers, U^T in LDS once per workgroup (48 KB at H = 64), the grid
// persistent.  A step's coefficient rows are asked for one step ahead.
template <int H>
__global__ __launch_bounds__(256) void seq_gru_adj_kernel(SeqAdjArgs a) {
  constexpr int NT = H / 16, W3 = 3 * H, CF = kJacCoef * H;
  __shared__ f4 sut[3 * NT * NT * 64];
  {
    const f4* s4 = reinterpret_cast<const f4*>(a.Ut);
    for (int e = threadIdx.x; e < 3 * NT * NT * 64; e += blockDim.x) sut[e] = s4[e];
  }
  const int lane = threadIdx.x & 63;
  const int wave = uniform(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  __syncthreads();
  const int64_t kc = (int64_t)a.n_blk * 16;   // cotangents of the chunk
  const int64_t n_work = a.n_dst * a.n_blk;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < n_work; w += (int64_t)gridDim.x * 4) {
    const int64_t pos = w / a.n_blk;
    const int64_t c = (w - pos * a.n_blk) * 16 + j;   // this lane's cotangent in the chunk
    const int row = uniform(a.order[pos]);
    const int L = uniform(a.len[pos]);
    const int s0 = uniform(a.step_ptr[pos]);
    const int64_t hofs = scen_offset(row, (int64_t)a.blk0 * 16 + c, a.kp, H) + 4 * g;
    f4 lam[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) lam[t] = ld4(a.lam_in + hofs + 16 * t);
    if (L > 0) {
      const float* cfp = a.coef + (int64_t)s0 * CF + 4 * g;
      float* ab = a.abar + ((int64_t)s0 * kc + c) * W3 + 4 * g;
      f4 cf[kJacCoef][NT];
#pragma unroll
      for (int q = 0; q < kJacCoef; ++q)
#pragma unroll
        for (int i = 0; i < NT; ++i) cf[q][i] = ld4(cfp + (int64_t)(L - 1) * CF + q * H + 16 * i);
      for (int t = L - 1; t >= 0; --t) {
        // the step before this one: its rows leave now and land behind this step's MFMAs (step 0 asks
        // for its own again: no branch, no read in front of the sequence)
        const float* nq = cfp + (int64_t)std::max(t - 1, 0) * CF;
        f4 cn[kJacCoef][NT];
#pragma unroll
        for (int q = 0; q < kJacCoef; ++q)
#pragma unroll
          for (int i = 0; i < NT; ++i) cn[q][i] = ld4(nq + q * H + 16 * i);
        f4 v[3][NT], acc[3][NT];
        float* o = ab + (int64_t)t * kc * W3;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          v[0][i] = cf[1][i] * lam[i];
          v[1][i] = cf[2][i] * lam[i];
          v[2][i] = cf[4][i] * lam[i];
          st4(o + 16 * i, v[0][i]);
          st4(o + H + 16 * i, v[1][i]);
          st4(o + 2 * H + 16 * i, cf[3][i] * lam[i]);
          acc[0][i] = cf[0][i] * lam[i];
          acc[1][i] = acc[2][i] = f4{0, 0, 0, 0};
        }
        sweep_t<NT, H>(sut, lane, v, acc);
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          lam[i] = (acc[0][i] + acc[1][i]) + acc[2][i];
#pragma unroll
          for (int q = 0; q < kJacCoef; ++q) cf[q][i] = cn[q][i];
        }
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) st4(a.lam_out + hofs + 16 * t, lam[t]);
  }
}

// ---------------------------------------------------------------------------------------------
// Adjoint of the sum update.  One wave per (order position, cotangent block): the coefficient rows
// once, l = z l' + [P l'|R l'|S l'].U^T into the destination's cotangent, xbar = [P l'|R l'|Q l'].W^T
// by destination row for the messages' sources; U^T and W^T in LDS once per workgroup, the grid persistent.
template <int DIN, int H>
__global__ __launch_bounds__(256) void sum_gru_adj_kernel(SumAdjArgs a) {
  constexpr int NC = DIN / 16, NT = H / 16, CF = kJacCoef * H;
  constexpr int WF = 3 * NT * NC * 64, UF = 3 * NT * NT * 64;   // float4 fragments
  __shared__ f4 swt[WF];
  __shared__ f4 sut[UF];
  {
    const f4* gW = reinterpret_cast<const f4*>(a.Wt);
    const f4* gU = reinterpret_cast<const f4*>(a.Ut);
    for (int i = threadIdx.x; i < WF; i += blockDim.x) swt[i] = gW[i];
    for (int i = threadIdx.x; i < UF; i += blockDim.x) sut[i] = gU[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = uniform(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const int64_t kc = (int64_t)a.n_blk * 16;
  const int64_t n_work = a.n_dst * a.n_blk;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < n_work; w += (int64_t)gridDim.x * 4) {
    const int64_t pos = w / a.n_blk;
    const int64_t c = (w - pos * a.n_blk) * 16 + j;
    const int row = uniform(a.order[pos]);
    const float* cfp = a.coef + pos * CF + 4 * g;
    const int64_t hofs = scen_offset(row, (int64_t)a.blk0 * 16 + c, a.kp, H) + 4 * g;
    // (an opaque lane offset keeps the loop-invariant fragment reads inside the work loop)
    int wofs = lane;
    asm volatile("" : "+v"(wofs));
    f4 v[3][NT], acc[3][NT], ql[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const f4 lam = ld4(a.lam_in + hofs + 16 * i);
      v[0][i] = ld4(cfp + 1 * H + 16 * i) * lam;
      v[1][i] = ld4(cfp + 2 * H + 16 * i) * lam;
      v[2][i] = ld4(cfp + 4 * H + 16 * i) * lam;
      ql[i] = ld4(cfp + 3 * H + 16 * i) * lam;
      acc[0][i] = ld4(cfp + 16 * i) * lam;
      acc[1][i] = acc[2][i] = f4{0, 0, 0, 0};
    }
    sweep_t<NT, H>(sut, wofs, v, acc);
#pragma unroll
    for (int i = 0; i < NT; ++i) st4(a.lam_out + hofs + 16 * i, (acc[0][i] + acc[1][i]) + acc[2][i]);
    f4 xa[3][NC];
#pragma unroll
    for (int i = 0; i < NT; ++i) v[2][i] = ql[i];
#pragma unroll
    for (int t = 0; t < NC; ++t) xa[0][t] = xa[1][t] = xa[2][t] = f4{0, 0, 0, 0};
    sweep_t<NC, H>(swt, wofs, v, xa);
    float* xo = a.xbar + ((int64_t)row * kc + c) * DIN + 4 * g;
#pragma unroll
    for (int t = 0; t < NC; ++t) st4(xo + 16 * t, (xa[0][t] + xa[1][t]) + xa[2][t]);
  }
}

// ---------------------------------------------------------------------------------------------
// Source rows gather their readers' blocks.  One wave per (source row, cotangent block): the blocks
// idx[ptr[r] .. ptr[r + 1]) lists are added one by one in that order, four in flight; GEMM: the [16][3H]
// sum then runs through W^T (LDS, once per workgroup) to [16][DIN]; the result is added to the row's
// cotangent state.  A row nobody read is left alone.
template <int DIN, int H, bool GEMM>
__global__ __launch_bounds__(256) void src_adj_kernel(SrcAdjArgs a) {
  constexpr int NC = DIN / 16, NT = H / 16;
  constexpr int W = GEMM ? 3 * H : DIN, NV = W / 16;
  constexpr int WF = GEMM ? 3 * NT * NC * 64 : 1;
  __shared__ f4 swt[WF];
  if constexpr (GEMM) {
    const f4* gW = reinterpret_cast<const f4*>(a.Wt);
    for (int i = threadIdx.x; i < WF; i += blockDim.x) swt[i] = gW[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int wave = uniform(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const int64_t kc = (int64_t)a.n_blk * 16;
  const int64_t n_work = a.rows * a.n_blk;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < n_work; w += (int64_t)gridDim.x * 4) {
    const int64_t r = w / a.n_blk;
    const int64_t c = (w - r * a.n_blk) * 16 + j;
    const int e0 = uniform(a.ptr[r]), e1 = uniform(a.ptr[r + 1]);
    if (e0 == e1) continue;
    const float* base = a.blocks + c * W + 4 * g;
    auto blk = [&](int e) { return base + (int64_t)uniform(a.idx[e]) * kc * W; };
    f4 v[NV];
#pragma unroll
    for (int s = 0; s < NV; ++s) v[s] = f4{0, 0, 0, 0};
    int e = e0;
    for (; e + 4 <= e1; e += 4) {
      const float *p0 = blk(e), *p1 = blk(e + 1), *p2 = blk(e + 2), *p3 = blk(e + 3);
      f4 v0[NV], v1[NV], v2[NV], v3[NV];
#pragma unroll
      for (int s = 0; s < NV; ++s) {
        v0[s] = ld4(p0 + 16 * s);
        v1[s] = ld4(p1 + 16 * s);
        v2[s] = ld4(p2 + 16 * s);
        v3[s] = ld4(p3 + 16 * s);
      }
#pragma unroll
      for (int s = 0; s < NV; ++s) v[s] = (((v[s] + v0[s]) + v1[s]) + v2[s]) + v3[s];
    }
    for (; e < e1; ++e) {
      const float* p = blk(e);
#pragma unroll
      for (int s = 0; s < NV; ++s) v[s] += ld4(p + 16 * s);
    }
    float* out = a.lam + scen_offset(r, (int64_t)a.blk0 * 16 + c, a.kp, DIN) + 4 * g;
    if constexpr (GEMM) {
      int wofs = lane;
      asm volatile("" : "+v"(wofs));
      f4 b[3][NT], xa[3][NC];
#pragma unroll
      for (int G = 0; G < 3; ++G)
#pragma unroll
        for (int i = 0; i < NT; ++i) b[G][i] = v[G * NT + i];
#pragma unroll
      for (int t = 0; t < NC; ++t) xa[0][t] = xa[1][t] = xa[2][t] = f4{0, 0, 0, 0};
      sweep_t<NC, H>(swt, wofs, b, xa);
#pragma unroll
      for (int t = 0; t < NC; ++t) st4(out + 16 * t, ld4(out + 16 * t) + ((xa[0][t] + xa[1][t]) + xa[2][t]));
    } else {
#pragma unroll
      for (int t = 0; t < NC; ++t) st4(out + 16 * t, ld4(out + 16 * t) + v[t]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
__global__ void cot_transpose_kernel(const float* __restrict__ cot, int64_t n_pred, int64_t n_cot, int64_t kp, int units,
                                     float* __restrict__ g) {
  const int64_t total = n_pred * kp * units;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pk = i / units;
    const int u = (int)(i - pk * units);
    const int64_t p = pk / kp, k = pk - p * kp;
    g[i] = k < n_cot ? cot[(k * n_pred + p) * units + u] : 0.0f;
  }
}

__global__ void feature_rows_adj_kernel(const float* __restrict__ lam, int64_t rows, int64_t n_cot, int64_t kp, int H, int F,
                                        float* __restrict__ out) {
  const int64_t total = n_cot * rows * F;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t kr = i / F;
    const int f = (int)(i - kr * F);
    const int64_t k = kr / rows, r = kr - k * rows;
    out[i] = lam[scen_offset(r, k, kp, H) + f];
  }
}

int blocks_for(int64_t threads, int64_t cap) { return (int)std::max<int64_t>(1, std::min<int64_t>((threads + 255) / 256, cap)); }

// resident workgroups per CU x CUs, at most the work (a persistent grid), asked once per kernel
template <auto KERNEL, int BLOCK>
int persistent_grid(int64_t n_blocks_of_work) {
  static const int64_t resident = [] {
    int dev = 0, cus = 0, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus <= 0) cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, KERNEL, BLOCK, 0) != hipSuccess || per_cu <= 0) per_cu = 1;
    return (int64_t)per_cu * cus;
  }();
  return (int)std::max<int64_t>(1, std::min<int64_t>(resident, n_blocks_of_work));
}

template <auto KERNEL, class Args>
hipError_t launch_waves(const Args& a, int64_t waves, hipStream_t st) {
  hipLaunchKernelGGL(KERNEL, dim3(persistent_grid<KERNEL, 256>((waves + 3) / 4)), dim3(256), 0, st, a);
  return hipGetLastError();
}

bool chunk_ok(int32_t kp, int32_t blk0, int32_t n_blk) {
  return kp >= 16 && kp % 16 == 0 && blk0 >= 0 && n_blk >= 1 && (int64_t)(blk0 + n_blk) * 16 <= kp;
}

}  // namespace

hipError_t launch_seq_gru_adj(const SeqAdjArgs& a, int h, hipStream_t st) {
  if (!jacobian_shape_supported(h, h) || !chunk_ok(a.kp, a.blk0, a.n_blk)) return hipErrorInvalidValue;
  if (!a.lam_in || !a.lam_out || a.lam_in == a.lam_out || !a.coef || !a.abar || !a.Ut) return hipErrorInvalidValue;
  if (a.n_dst == 0) return hipSuccess;
  const int64_t waves = a.n_dst * a.n_blk;
  switch (h) {
    case 16: return launch_waves<seq_gru_adj_kernel<16>>(a, waves, st);
    case 32: return launch_waves<seq_gru_adj_kernel<32>>(a, waves, st);
    default: return launch_waves<seq_gru_adj_kernel<64>>(a, waves, st);
  }
}

hipError_t launch_sum_gru_adj(const SumAdjArgs& a, int din, int h, hipStream_t st) {
  if (!jacobian_shape_supported(din, h) || !chunk_ok(a.kp, a.blk0, a.n_blk)) return hipErrorInvalidValue;
  if (!a.lam_in || !a.lam_out || a.lam_in == a.lam_out || !a.coef || !a.xbar || !a.Wt || !a.Ut) return hipErrorInvalidValue;
  if (a.n_dst == 0) return hipSuccess;
  const int64_t waves = a.n_dst * a.n_blk;
  if (din == 32 && h == 32) return launch_waves<sum_gru_adj_kernel<32, 32>>(a, waves, st);
  if (din == 16 && h == 16) return launch_waves<sum_gru_adj_kernel<16, 16>>(a, waves, st);
  if (din == 16 && h == 32) return launch_waves<sum_gru_adj_kernel<16, 32>>(a, waves, st);
  if (din == 32 && h == 16) return launch_waves<sum_gru_adj_kernel<32, 16>>(a, waves, st);
  return launch_waves<sum_gru_adj_kernel<64, 64>>(a, waves, st);
}

hipError_t launch_src_adj(const SrcAdjArgs& a, int din, int h, hipStream_t st) {
  if (!jacobian_shape_supported(din, h) || !chunk_ok(a.kp, a.blk0, a.n_blk)) return hipErrorInvalidValue;
  if (!a.lam || !a.blocks || !a.ptr || !a.idx) return hipErrorInvalidValue;
  if (a.rows == 0) return hipSuccess;
  const int64_t waves = a.rows * a.n_blk;
  if (!a.Wt) {
    switch (din) {
      case 16: return launch_waves<src_adj_kernel<16, 16, false>>(a, waves, st);
      case 32: return launch_waves<src_adj_kernel<32, 32, false>>(a, waves, st);
      default: return launch_waves<src_adj_kernel<64, 64, false>>(a, waves, st);
    }
  }
  if (din == 32 && h == 32) return launch_waves<src_adj_kernel<32, 32, true>>(a, waves, st);
  if (din == 16 && h == 16) return launch_waves<src_adj_kernel<16, 16, true>>(a, waves, st);
  if (din == 16 && h == 32) return launch_waves<src_adj_kernel<16, 32, true>>(a, waves, st);
  if (din == 32 && h == 16) return launch_waves<src_adj_kernel<32, 16, true>>(a, waves, st);
  return launch_waves<src_adj_kernel<64, 64, true>>(a, waves, st);
}

hipError_t launch_cot_transpose(const float* cot, int64_t n_pred, int64_t n_cot, int units, float* g, hipStream_t st) {
  if (!cot || !g || n_cot < 1 || units < 1) return hipErrorInvalidValue;
  if (n_pred == 0) return hipSuccess;
  const int64_t kp = scen_padded(n_cot);
  hipLaunchKernelGGL(cot_transpose_kernel, dim3(blocks_for(n_pred * kp * units, 8192)), dim3(256), 0, st, cot, n_pred, n_cot,
                     kp, units, g);
  return hipGetLastError();
}

hipError_t launch_feature_rows_adj(const float* lam, int64_t rows, int64_t n_cot, int H, int F, float* out, hipStream_t st) {
  if (!lam || !out || n_cot < 1 || F < 1 || F > H) return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(feature_rows_adj_kernel, dim3(blocks_for(n_cot * rows * F, 8192)), dim3(256), 0, st, lam, rows, n_cot,
                     scen_padded(n_cot), H, F, out);
  return hipGetLastError();
}
