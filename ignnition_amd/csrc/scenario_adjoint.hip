// scenario_adjoint.hip — the reverse sweep of ign_backward_scenarios on f32 MFMA
// (v_mfma_f32_16x16x4_f32): d(sum cot_s . pred_s) / d(features of scenario s) for S feature sets on one
// topology.
//
// scenario.hip's linearising primal leaves per real GRU step and per scenario the rows (z, P, R, Q, S) of
//   hd' = z hd + P (ad_z + hd.U_z) + R (ad_r + hd.U_r) + Q ad_h + S (hd.U_h)
// as tiles [item][block][5][16][H].  The transpose of a step, l' the cotangent of the state after it:
//   abar = [P l' | R l' | Q l']                 cotangent of the step's x.W row (3H)
//   l    = z l' + [P l' | R l' | S l'] . U^T    one contraction, k = 3H -> H
// Layout as §3m: a wave owns (order position, scenario block), the 16 rows of its tile are 16 scenarios of
// one destination, so one length and one step range per wave -- but every row has its own primal, so
// where adjoint.hip broadcasts a step's coefficient rows, a lane here loads its own float4 of each: the
// accumulator layout (row j = lane & 15, units 16 t + 4 g ..) is the coefficient tile's, the loads are 16
// bytes, and the products P l' .. S l' a lane forms are already the B operand of the sweep over U^T
// (k(s4, g, q) = 16 s4 + 4 g + q).  The A operand is launch_pack_a's fragments of the raw U [H][3H] in LDS
// once per workgroup; the three gates' k ranges run into three accumulator sets (independent MFMA chains),
// z l' starts the first, and the sets are added in one order.  No exp, no tanh, no mask, no step code.
// The step / destination blocks are adjoint.hip's, and its src_adj_kernel gathers them for the sources.
// Every operation is linear in the cotangent and an MFMA column depends on its own B column only: zero
// cotangents give zeros, and a scenario's bits depend neither on S, nor on its index, nor on the chunk of
// blocks a launch covers.

#include "scenario_adjoint_dev.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Adjoint of the ordered update.  One wave per (order position, scenario block) for the whole sequence,
// last step first: l in registers, U^T in LDS once per workgroup (48 KB at H = 64), the grid persistent.
// A step's products leave its coefficient registers dead before its sweep starts, so the tile of the step
// in front is asked for into the same registers right there and lands behind the MFMAs: one tile of
// coefficients (80 registers at H = 64) is live, not two.
template <int H>
__global__ __launch_bounds__(256) void seq_gru_sadj_kernel(SeqSAdjArgs a) {
  constexpr int NT = H / 16, W3 = 3 * H;
  constexpr int64_t TILE = (int64_t)kScenCoef * 16 * H;
  __shared__ f4 sut[3 * NT * NT * 64];
  {
    const f4* s4 = reinterpret_cast<const f4*>(a.Ut);
    for (int e = threadIdx.x; e < 3 * NT * NT * 64; e += blockDim.x) sut[e] = s4[e];
  }
  const int lane = threadIdx.x & 63;
  const int wave = uniform(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
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
      // step t's tile: cfp + t * step_stride; its cotangent block: ab + t * sp * W3
      const float* cfp = a.coef + ((int64_t)s0 * a.n_blk + blk) * TILE + j * H + 4 * g;
      const int64_t step_stride = (int64_t)a.n_blk * TILE;
      float* ab = a.abar + ((int64_t)s0 * sp + s) * W3 + 4 * g;
      f4 cf[kScenCoef][NT];
      load_tile<H>(cfp + (int64_t)(L - 1) * step_stride, cf);
      for (int t = L - 1; t >= 0; --t) {
        f4 v[3][NT], acc[3][NT];
        float* o = ab + (int64_t)t * sp * W3;
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
        // the step in front of this one (step 0 asks for its own again: no branch, no read in front of
        // the sequence)
        load_tile<H>(cfp + (int64_t)std::max(t - 1, 0) * step_stride, cf);
        sweep_t<NT, H>(sut, lane, v, acc);
#pragma unroll
        for (int i = 0; i < NT; ++i) lam[i] = (acc[0][i] + acc[1][i]) + acc[2][i];
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) st4(a.lam_out + hofs + 16 * t, lam[t]);
  }
}

// ---------------------------------------------------------------------------------------------
// Adjoint of the sum update.  One wave per (order position, scenario block): the tile's coefficient rows
// once, l = z l' + [P l'|R l'|S l'].U^T into the destination's cotangent, xbar = [P l'|R l'|Q l'].W^T by
// destination row for the messages' sources; U^T and W^T in LDS once per workgroup, the grid persistent.
template <int DIN, int H>
__global__ __launch_bounds__(256) void sum_gru_sadj_kernel(SumSAdjArgs a) {
  constexpr int NC = DIN / 16, NT = H / 16;
  constexpr int64_t TILE = (int64_t)kScenCoef * 16 * H;
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
  const int64_t sp = (int64_t)a.n_blk * 16;
  const int64_t n_work = a.n_dst * a.n_blk;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < n_work; w += (int64_t)gridDim.x * 4) {
    const int64_t pos = w / a.n_blk;
    const int64_t s = (w - pos * a.n_blk) * 16 + j;
    const int row = uniform(a.order[pos]);
    const int64_t hofs = scen_offset(row, s, sp, H) + 4 * g;
    // (an opaque lane offset keeps the loop-invariant fragment reads inside the work loop)
    int wofs = lane;
    asm volatile("" : "+v"(wofs));
    f4 cf[kScenCoef][NT];
    load_tile<H>(a.coef + w * TILE + j * H + 4 * g, cf);
    f4 v[3][NT], acc[3][NT], ql[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const f4 lam = ld4(a.lam_in + hofs + 16 * i);
      v[0][i] = cf[1][i] * lam;
      v[1][i] = cf[2][i] * lam;
      v[2][i] = cf[4][i] * lam;
      ql[i] = cf[3][i] * lam;
      acc[0][i] = cf[0][i] * lam;
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
    float* xo = a.xbar + ((int64_t)row * sp + s) * DIN + 4 * g;
#pragma unroll
    for (int t = 0; t < NC; ++t) st4(xo + 16 * t, (xa[0][t] + xa[1][t]) + xa[2][t]);
  }
}

}  // namespace

hipError_t launch_seq_gru_sadj(const SeqSAdjArgs& a, int h, hipStream_t st) {
  if (!scen_adj_supported(h, h) || a.n_blk < 1) return hipErrorInvalidValue;
  if (!a.lam_in || !a.lam_out || a.lam_in == a.lam_out || !a.coef || !a.abar || !a.Ut) return hipErrorInvalidValue;
  if (!aligned16(a.lam_in) || !aligned16(a.lam_out) || !aligned16(a.coef) || !aligned16(a.abar) || !aligned16(a.Ut))
    return hipErrorInvalidValue;
  if (a.n_dst == 0) return hipSuccess;
  const int64_t waves = a.n_dst * a.n_blk;
  switch (h) {
    case 16: return launch_waves<seq_gru_sadj_kernel<16>>(a, waves, st);
    case 32: return launch_waves<seq_gru_sadj_kernel<32>>(a, waves, st);
    default: return launch_waves<seq_gru_sadj_kernel<64>>(a, waves, st);
  }
}

hipError_t launch_sum_gru_sadj(const SumSAdjArgs& a, int din, int h, hipStream_t st) {
  if (!scen_adj_supported(din, h) || a.n_blk < 1) return hipErrorInvalidValue;
  if (!a.lam_in || !a.lam_out || a.lam_in == a.lam_out || !a.coef || !a.xbar || !a.Wt || !a.Ut) return hipErrorInvalidValue;
  if (!aligned16(a.lam_in) || !aligned16(a.lam_out) || !aligned16(a.coef) || !aligned16(a.xbar) || !aligned16(a.Wt) ||
      !aligned16(a.Ut))
    return hipErrorInvalidValue;
  if (a.n_dst == 0) return hipSuccess;
  const int64_t waves = a.n_dst * a.n_blk;
  if (din == 32 && h == 32) return launch_waves<sum_gru_sadj_kernel<32, 32>>(a, waves, st);
  if (din == 16 && h == 16) return launch_waves<sum_gru_sadj_kernel<16, 16>>(a, waves, st);
  if (din == 16 && h == 32) return launch_waves<sum_gru_sadj_kernel<16, 32>>(a, waves, st);
  if (din == 32 && h == 16) return launch_waves<sum_gru_sadj_kernel<32, 16>>(a, waves, st);
  return launch_waves<sum_gru_sadj_kernel<64, 64>>(a, waves, st);
}
