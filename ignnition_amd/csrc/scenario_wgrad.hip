// scenario_wgrad.hip — the kernels ign_backward_scenarios_params adds to the scenario adjoint
// (DESIGN.md §3q): d(sum_s cot_s . pred_s) / d(parameters) for S feature sets on one topology.
//
// The hot path is the ordered adjoint: seq_gru_sadj's reverse sweep (scenario_adjoint.hip), a wave per
// (order position, scenario block), with the recurrent weight gradient formed where the products are.  Per
// tile-step the wave holds ubar = [P l'|R l'|S l'] in the accumulator layout (row = scenario j = lane & 15,
// four consecutive units per lane).  dU [H][3H] += h_prev^T . ubar contracts over the tile's 16 SCENARIOS, so
// both operands need the scenario on the MFMA k axis (lane >> 4):
//   A  h_prev: the primal kept the tile transposed [H][16], so lane (j, g) loads units 16 mt + j, scenarios
//      4 g .. 4 g + 3 as ONE float4 per row tile -- MFMA q of the four takes scenario 4 g + q;
//   B  ubar: one transpose per step through a per-wave LDS tile [3H][16 + 4]: a lane stores its four units
//      of scenario j as scalars (lanes j consecutive: conflict-free), and reads columns 16 nt + j, scenarios
//      4 g .. 4 g + 3 as float4s -- a row stride of 20 floats puts eight consecutive rows on all 32 banks.
// abar is never read back.  dU lives in registers for the wave's whole persistent walk (48 per lane at
// H = 32, 12 at 16) beside the lane's own running sums of ubar and of abar's third block (the bias
// gradients), and goes once per wave to a partial tile [H + 2][3H] in launch_seq_bwd_reduce's layout.  The
// wave-to-work assignment is the static stride of the persistent grid and the tiles are reduced in slot
// order, so the bits repeat from run to run.  At H = 64 the partial would be 192 registers on top of the
// sweep's: there (and with the A/B switch) the kernel stores ubar beside abar and launch_tsgemm_add contracts
// the flat rows.  A padding scenario's cotangent is zero, so its l, abar and ubar are zeros and its finite
// h_prev contributes nothing.

#include "scenario_adjoint_dev.h"
#include "scenario_wgrad.h"
#include "train_kernels.h"

namespace {

constexpr int kLd = 20;   // floats between the rows of the transposed ubar tile

template <int H, bool FUSED>
__global__ __launch_bounds__(256) void seq_gru_swg_kernel(SeqSWgArgs wa) {
  const SeqSAdjArgs& a = wa.adj;
  constexpr int NT = H / 16, W3 = 3 * H;
  constexpr int64_t TILE = (int64_t)kScenCoef * 16 * H;
  __shared__ f4 sut[3 * NT * NT * 64];
  __shared__ __attribute__((aligned(16))) float stp[FUSED ? 4 * W3 * kLd : 4];
  {
    const f4* s4 = reinterpret_cast<const f4*>(a.Ut);
    for (int e = threadIdx.x; e < 3 * NT * NT * 64; e += blockDim.x) sut[e] = s4[e];
  }
  const int lane = threadIdx.x & 63;
  const int wave = uniform(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  float* tp = stp + (FUSED ? wave * W3 * kLd : 0);
  f4 dU[NT][3 * NT], su[3][NT], sq[NT];   // FUSED: the wave's partial, the lane's column sums of ubar / Q l'
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    sq[i] = su[0][i] = su[1][i] = su[2][i] = f4{0, 0, 0, 0};
#pragma unroll
    for (int n = 0; n < 3 * NT; ++n) dU[i][n] = f4{0, 0, 0, 0};
  }
  __syncthreads();
  const int64_t sp = (int64_t)a.n_blk * 16;
  const int64_t n_work = a.n_dst * a.n_blk;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < n_work; w += (int64_t)gridDim.x * 4) {
    const int64_t pos = w / a.n_blk, blk = w - pos * a.n_blk;
    const int64_t s = blk * 16 + j;   // this lane's scenario
    const int row = uniform(a.order[pos]);
    const int L = uniform(a.len[pos]);
    const int s0 = uniform(a.step_ptr[pos]);
    const int64_t hofs = scen_offset(row, s, sp, H) + 4 * g;
    f4 lam[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) lam[t] = ld4(a.lam_in + hofs + 16 * t);
    if (L > 0) {
      const float* cfp = a.coef + ((int64_t)s0 * a.n_blk + blk) * TILE + j * H + 4 * g;
      const int64_t step_stride = (int64_t)a.n_blk * TILE;
      const int64_t ofs = ((int64_t)s0 * sp + s) * W3 + 4 * g;
      // the step's transposed h_prev tile, row tile mt: units 16 mt + j, scenarios 4 g ..
      const float* hp = wa.hprev + ((int64_t)s0 * a.n_blk + blk) * 16 * H + j * 16 + 4 * g;
      const int64_t h_stride = (int64_t)a.n_blk * 16 * H;
      f4 cf[kScenCoef][NT], ha[NT];
      load_tile<H>(cfp + (int64_t)(L - 1) * step_stride, cf);
      if constexpr (FUSED) {
#pragma unroll
        for (int mt = 0; mt < NT; ++mt) ha[mt] = ld4(hp + (int64_t)(L - 1) * h_stride + mt * 256);
      }
      for (int t = L - 1; t >= 0; --t) {
        f4 v[3][NT], acc[3][NT], ql[NT];
        float* o = a.abar + ofs + (int64_t)t * sp * W3;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          v[0][i] = cf[1][i] * lam[i];
          v[1][i] = cf[2][i] * lam[i];
          v[2][i] = cf[4][i] * lam[i];
          ql[i] = cf[3][i] * lam[i];
          st4(o + 16 * i, v[0][i]);
          st4(o + H + 16 * i, v[1][i]);
          st4(o + 2 * H + 16 * i, ql[i]);
          acc[0][i] = cf[0][i] * lam[i];
          acc[1][i] = acc[2][i] = f4{0, 0, 0, 0};
        }
        if constexpr (!FUSED) {
          float* u = wa.ubar + ofs + (int64_t)t * sp * W3;
#pragma unroll
          for (int G = 0; G < 3; ++G)
#pragma unroll
            for (int i = 0; i < NT; ++i) st4(u + G * H + 16 * i, v[G][i]);
        }
        // the step in front of this one (step 0 asks for its own again), as seq_gru_sadj does
        load_tile<H>(cfp + (int64_t)std::max(t - 1, 0) * step_stride, cf);
        if constexpr (FUSED) {
#pragma unroll
          for (int G = 0; G < 3; ++G)
#pragma unroll
            for (int i = 0; i < NT; ++i) {
              su[G][i] += v[G][i];
#pragma unroll
              for (int q = 0; q < 4; ++q) tp[(G * H + 16 * i + 4 * g + q) * kLd + j] = v[G][i][q];
            }
#pragma unroll
          for (int i = 0; i < NT; ++i) sq[i] += ql[i];
          // the tile is the wave's own: its LDS operations complete in order, the compiler must keep them so
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          f4 bt[3 * NT];
#pragma unroll
          for (int n = 0; n < 3 * NT; ++n) bt[n] = *reinterpret_cast<const f4*>(tp + (16 * n + j) * kLd + 4 * g);
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int mt = 0; mt < NT; ++mt)
#pragma unroll
              for (int n = 0; n < 3 * NT; ++n) dU[mt][n] = MFMA(ha[mt][q], bt[n][q], dU[mt][n]);
#pragma unroll
          for (int mt = 0; mt < NT; ++mt) ha[mt] = ld4(hp + (int64_t)std::max(t - 1, 0) * h_stride + mt * 256);
        }
        sweep_t<NT, H>(sut, lane, v, acc);
#pragma unroll
        for (int i = 0; i < NT; ++i) lam[i] = (acc[0][i] + acc[1][i]) + acc[2][i];
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) st4(a.lam_out + hofs + 16 * t, lam[t]);
  }
  if constexpr (FUSED) {
    // the wave's tile: rows 0 .. H - 1 dU, row H the column sums of abar, row H + 1 those of ubar; a lane's
    // sums are its scenario's, so the 16 lanes of a unit group add up first (one order)
    float* P = wa.part + ((int64_t)blockIdx.x * 4 + wave) * (H + 2) * W3;
#pragma unroll
    for (int mt = 0; mt < NT; ++mt)
#pragma unroll
      for (int n = 0; n < 3 * NT; ++n)
#pragma unroll
        for (int q = 0; q < 4; ++q) P[(16 * mt + 4 * g + q) * W3 + 16 * n + j] = dU[mt][n][q];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      f4 c[4] = {su[0][i], su[1][i], su[2][i], sq[i]};
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int d = 1; d < 16; d <<= 1) c[k][q] += __shfl_xor(c[k][q], d, 16);
      if (j == 0) {
#pragma unroll
        for (int G = 0; G < 3; ++G) {
          st4(P + (H + 1) * W3 + G * H + 16 * i + 4 * g, c[G]);
          st4(P + H * W3 + G * H + 16 * i + 4 * g, G == 2 ? c[3] : c[G]);
        }
      }
    }
  }
}

// one thread per float4 of a (position, scenario) row
template <int H>
__global__ void sum_products_scen_kernel(SumProductsArgs a) {
  constexpr int HQ = H / 4, W3 = 3 * H;
  const int64_t sp = (int64_t)a.n_blk * 16, total = a.n_dst * sp * HQ;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t ps = i / HQ;
    const int c = 4 * (int)(i - ps * HQ);
    const int64_t pos = ps / sp, s = ps - pos * sp;
    const int64_t rofs = scen_offset(a.order[pos], s, sp, H) + c;
    const float* cf = a.coef + (((pos * a.n_blk + s / 16) * kScenCoef) * 16 + (s & 15)) * H + c;
    const f4 lam = ld4(a.lam_in + rofs);
    const f4 pl = ld4(cf + 16 * H) * lam, rl = ld4(cf + 2 * 16 * H) * lam;
    st4(a.abar + ps * W3 + c, pl);
    st4(a.abar + ps * W3 + H + c, rl);
    st4(a.abar + ps * W3 + 2 * H + c, ld4(cf + 3 * 16 * H) * lam);
    st4(a.ubar + ps * W3 + c, pl);
    st4(a.ubar + ps * W3 + H + c, rl);
    st4(a.ubar + ps * W3 + 2 * H + c, ld4(cf + 4 * 16 * H) * lam);
    st4(a.hpos + ps * H + c, ld4(a.h_in + rofs));
  }
}

// one thread per float4 of a (source row, scenario) row
__global__ void gather_blocks_scen_kernel(float* __restrict__ out, const float* __restrict__ blocks,
                                          const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx, int64_t rows,
                                          int64_t sp, int W) {
  const int64_t q = W / 4, total = rows * sp * q;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t rs = i / q, r = rs / sp;
    const int64_t in_row = (rs - r * sp) * W + (i - rs * q) * 4;
    f4 acc = f4{0, 0, 0, 0};
    for (int e = ptr[r]; e < ptr[r + 1]; ++e) acc += ld4(blocks + (int64_t)idx[e] * sp * W + in_row);
    st4(out + i * 4, acc);
  }
}

int blocks_for(int64_t threads) { return (int)std::max<int64_t>(1, std::min<int64_t>((threads + 255) / 256, 16384)); }

// a fused launch's grid: the persistent grid, within the partial slots a reduction takes
template <int H>
int fused_grid(int64_t waves) {
  return std::min(waves_grid<seq_gru_swg_kernel<H, true>>(waves), kBwdPartialWaves / 4);
}

template <int H, bool FUSED>
hipError_t seq_swg_launch(const SeqSWgArgs& a, int64_t waves, hipStream_t st) {
  if constexpr (FUSED) {
    hipLaunchKernelGGL((seq_gru_swg_kernel<H, true>), dim3(fused_grid<H>(waves)), dim3(256), 0, st, a);
    return hipGetLastError();
  } else {
    return launch_waves<seq_gru_swg_kernel<H, false>>(a, waves, st);
  }
}

}  // namespace

int64_t seq_swg_slots(int64_t n_dst, int32_t n_blk, int h) {
  if (n_dst <= 0 || n_blk < 1) return 0;
  return 4 * (int64_t)(h == 16 ? fused_grid<16>(n_dst * n_blk) : fused_grid<32>(n_dst * n_blk));
}

hipError_t launch_seq_gru_swg(const SeqSWgArgs& wa, int h, bool fused, hipStream_t st) {
  const SeqSAdjArgs& a = wa.adj;
  if (!scen_adj_supported(h, h) || a.n_blk < 1 || (fused && !scen_wgrad_fused_supported(h))) return hipErrorInvalidValue;
  if (!a.lam_in || !a.lam_out || a.lam_in == a.lam_out || !a.coef || !a.abar || !a.Ut || !wa.hprev || !(fused ? wa.part : wa.ubar))
    return hipErrorInvalidValue;
  if (!aligned16(a.lam_in) || !aligned16(a.lam_out) || !aligned16(a.coef) || !aligned16(a.abar) || !aligned16(a.Ut) ||
      !aligned16(wa.hprev) || !aligned16(wa.ubar) || !aligned16(wa.part))
    return hipErrorInvalidValue;
  if (a.n_dst == 0) return hipSuccess;
  const int64_t waves = a.n_dst * a.n_blk;
  if (fused) return h == 16 ? seq_swg_launch<16, true>(wa, waves, st) : seq_swg_launch<32, true>(wa, waves, st);
  switch (h) {
    case 16: return seq_swg_launch<16, false>(wa, waves, st);
    case 32: return seq_swg_launch<32, false>(wa, waves, st);
    default: return seq_swg_launch<64, false>(wa, waves, st);
  }
}

hipError_t launch_sum_products_scen(const SumProductsArgs& a, int h, hipStream_t st) {
  if (!scen_seq_supported(h) || a.n_blk < 1 || !a.coef || !a.lam_in || !a.h_in || !a.order || !a.abar || !a.ubar || !a.hpos)
    return hipErrorInvalidValue;
  if (!aligned16(a.coef) || !aligned16(a.lam_in) || !aligned16(a.h_in) || !aligned16(a.abar) || !aligned16(a.ubar) ||
      !aligned16(a.hpos))
    return hipErrorInvalidValue;
  if (a.n_dst == 0) return hipSuccess;
  const dim3 grid(blocks_for(a.n_dst * a.n_blk * 16 * (h / 4)));
  if (h == 16) hipLaunchKernelGGL(sum_products_scen_kernel<16>, grid, dim3(256), 0, st, a);
  else if (h == 32) hipLaunchKernelGGL(sum_products_scen_kernel<32>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(sum_products_scen_kernel<64>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_gather_blocks_scen(float* out, const float* blocks, const int32_t* ptr, const int32_t* idx, int64_t rows,
                                     int64_t sp, int W, hipStream_t st) {
  if (!out || !blocks || !ptr || !idx || W % 4 || sp < 16 || !aligned16(out) || !aligned16(blocks)) return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(gather_blocks_scen_kernel, dim3(blocks_for(rows * sp * (W / 4))), dim3(256), 0, st, out, blocks, ptr, idx,
                     rows, sp, W);
  return hipGetLastError();
}
