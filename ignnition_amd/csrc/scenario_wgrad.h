// scenario_wgrad.h — launchers of the kernels ign_backward_scenarios_params adds to the scenario adjoint
// (scenario_wgrad.hip, scenario_adjoint.cpp): d(sum_s cot_s . pred_s) / d(parameters), summed over S feature
// sets on one topology, in one pass.  The ordered adjoint already forms, per tile-step, the
// step cotangents abar = [P l'|R l'|Q l'] and the recurrent-side products ubar = [P l'|R l'|S l']; what a
// weight gradient adds is their contraction with the primal's states:
//   dU += h_prev^T . ubar      db_rec += sum ubar      db_in += sum abar      (over steps x scenarios)
// fused into the sweep (H 16 / 32: dU in registers for a wave's whole walk, k over the tile's 16 scenarios)
// or left to launch_tsgemm_add over the flat rows step * Sp + s of the stored h_prev and ubar (H 64, and the
// A/B switch).  Everything row-count-sized goes through launch_tsgemm_add on flat rows x Sp.
#pragma once
#include "scenario_adjoint.h"

inline bool scen_wgrad_fused_supported(int h) { return h == 16 || h == 32; }

// seq_gru_sadj's sweep with the recurrent weight gradient.
struct SeqSWgArgs {
  SeqSAdjArgs adj;
  const float* hprev;   // launch_seq_gru_scen's keep: fused the transposed tiles [step][block][H][16], else flat rows
  float* ubar;          // unfused: [n_steps][Sp][3H] the recurrent-side products, written
  float* part;          // fused: seq_swg_slots(..) tiles [H + 2][3H] in launch_seq_bwd_reduce's layout (dU, the
                        // column sums of abar, those of ubar), every one written
};
// the partial tiles a fused launch writes: one per wave of its persistent grid, the same from call to call
int64_t seq_swg_slots(int64_t n_dst, int32_t n_blk, int h);
// scen_adj_supported(h, h); fused: scen_wgrad_fused_supported(h)
hipError_t launch_seq_gru_swg(const SeqSWgArgs& a, int h, bool fused, hipStream_t st);

// The sum update's products by order position, as flat rows pos * Sp + s: abar [..][3H], ubar [..][3H] from
// the destination's coefficient tile and the cotangent of its state after the MP, and hpos [..][H], its state
// before the MP (h_in [rows][Sp][H]) in the same row order.
struct SumProductsArgs {
  const float* coef;    // [n_dst][n_blk][kScenCoef][16][H]
  const float* lam_in;  // [rows][Sp][H]
  const float* h_in;
  const int32_t* order;
  float *abar, *ubar, *hpos;
  int64_t n_dst;
  int32_t n_blk;
};
hipError_t launch_sum_products_scen(const SumProductsArgs& a, int h, hipStream_t st);

// out[r][s][:W] = the sum of blocks[idx[e]][s][:W] over e in [ptr[r], ptr[r + 1]), in the list's order (zeros
// for a row nobody read): the cotangent of an ordered MP's projected source rows, launch_src_adj's gathered
// block in front of its W^T contraction.  W % 4 == 0
hipError_t launch_gather_blocks_scen(float* out, const float* blocks, const int32_t* ptr, const int32_t* idx, int64_t rows,
                                     int64_t sp, int W, hipStream_t st);
