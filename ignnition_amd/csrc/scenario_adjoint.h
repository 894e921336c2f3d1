// scenario_adjoint.h — launchers of the kernels behind ign_backward_scenarios (scenario_adjoint.hip,
// scenario_adjoint.cpp): the input gradients of S feature sets on one topology in one pass.
// The layout is §3m's: Sp = S rounded up to 16, states and cotangent states [row][Sp][H], a tile the 16
// scenarios of one destination.  scenario.h's linearising primal leaves per real GRU step and PER SCENARIO
// the coefficient rows (z, P, R, Q, S) of
//   hd' = z hd + P (ad_z + hd.U_z) + R (ad_r + hd.U_r) + Q ad_h + S (hd.U_h)
// as tiles [item][n_blk][kScenCoef][16][H]; the transpose of a step, l' the cotangent of the state after it:
//   abar = [P l' | R l' | Q l']                  (3H: the cotangent of the step's x.W row)
//   l    = z l' + [P l' | R l' | S l'] . U^T     (one contraction, k = 3H -> H)
// §3o's adjoint with every row of a tile on its own primal: the coefficients are a lane's own 16-byte loads
// where §3o broadcasts them.  The blocks the cell kernels leave are adjoint.h's ([item][Sp][width]), so
// launch_src_adj gathers them for the source rows unchanged (kp = Sp, blk0 = 0, n_blk = Sp / 16).
#pragma once
#include "adjoint.h"
#include "scenario.h"

// Adjoint of the ordered update: every sequence's steps from last to first.
struct SeqSAdjArgs {
  const float* lam_in;         // [rows][Sp][H] cotangent of the states after the MP
  float* lam_out;              // [rows][Sp][H] cotangent of the states before it (the cell's part), written
  const float* coef;           // [n_steps][n_blk][kScenCoef][16][H]
  float* abar;                 // [n_steps][Sp][3H] the step cotangents, written
  const int32_t* order;
  const int32_t* len;
  const int32_t* step_ptr;
  const float* Ut;             // launch_pack_a's fragments of the raw U [H][3H]
  int64_t n_dst;
  int32_t n_blk;               // Sp / 16
};
// scen_adj_supported(h, h)
hipError_t launch_seq_gru_sadj(const SeqSAdjArgs& a, int h, hipStream_t st);

// Adjoint of the sum update: one step per destination.
struct SumSAdjArgs {
  const float* lam_in;
  float* lam_out;
  const float* coef;           // [n_dst][n_blk][kScenCoef][16][H] per order position
  float* xbar;                 // [rows][Sp][DIN] by destination ROW: the cotangent of the summed messages, written
  const int32_t* order;
  const float* Wt;             // launch_pack_a's fragments of the raw W [DIN][3H]
  const float* Ut;
  int64_t n_dst;
  int32_t n_blk;
};
// scen_adj_supported(din, h)
hipError_t launch_sum_gru_sadj(const SumSAdjArgs& a, int din, int h, hipStream_t st);
