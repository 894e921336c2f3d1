// adjoint.h — launchers of the kernels behind ign_backward_jacobian (adjoint.hip, adjoint.cpp): K
// prediction cotangents through ONE adjoint sweep of the linearised forward.  The
// linearising primal of jacobian.h leaves per real GRU step the coefficient rows (z, P, R, Q, S) of
//   hd' = z hd + P (ad_z + hd.U_z) + R (ad_r + hd.U_r) + Q ad_h + S (hd.U_h)
// and the transpose of that step, with l' the cotangent of the state after it, is
//   abar = [P l' | R l' | Q l']                  (3H: the cotangent of the step's x.W row)
//   l    = z l' + [P l' | R l' | S l'] . U^T     (one contraction, k = 3H -> H)
// The layout is §3m / §3n's with the 16 rows of an MFMA tile on the COTANGENT axis: Kp = K rounded up to
// 16, cotangent states [row][Kp][H].  The per-step / per-destination blocks a cell kernel leaves for its
// sources are written for one CHUNK of cotangent blocks [blk0, blk0 + n_blk): [item][n_blk * 16][width].
// U^T / W^T are launch_pack_a's fragments of the raw U [H][3H] / W [DIN][3H] (tiles over the rows, k
// over 3H).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jacobian.h"

// Adjoint of the ordered update: every sequence's steps from last to first.
struct SeqAdjArgs {
  const float* lam_in;         // [rows][Kp][H] cotangent of the states after the MP
  float* lam_out;              // [rows][Kp][H] cotangent of the states before it (the cell's part), written
  const float* coef;           // [n_steps][kJacCoef][H]
  float* abar;                 // [n_steps][n_blk * 16][3H] this chunk's step cotangents, written
  const int32_t* order;
  const int32_t* len;
  const int32_t* step_ptr;
  const float* Ut;
  int64_t n_dst;
  int32_t kp, blk0, n_blk;
};
hipError_t launch_seq_gru_adj(const SeqAdjArgs& a, int h, hipStream_t st);

// Adjoint of the sum update: one step per destination.
struct SumAdjArgs {
  const float* lam_in;
  float* lam_out;
  const float* coef;           // [n_dst][kJacCoef][H] per order position
  float* xbar;                 // [rows][n_blk * 16][DIN] by destination ROW: this chunk's cotangent of the summed messages
  const int32_t* order;
  const float* Wt;
  const float* Ut;
  int64_t n_dst;
  int32_t kp, blk0, n_blk;
};
hipError_t launch_sum_gru_adj(const SumAdjArgs& a, int din, int h, hipStream_t st);

// Step / destination cotangents to source cotangents, without a scatter: source row r adds the blocks
// its transposed CSR lists, in the list's order (ascending step / message), to lam[r][chunk's cotangents].
// With Wt (blocks [..][3H]): the sum goes through W^T on the way (3H -> DIN); without (blocks [..][DIN]): as it is.
struct SrcAdjArgs {
  float* lam;                  // [rows][Kp][DIN] the source entity's cotangent states, added to
  const float* blocks;         // [item][n_blk * 16][W]
  const int32_t* ptr;          // [rows + 1]
  const int32_t* idx;
  const float* Wt;             // null: plain
  int64_t rows;
  int32_t kp, blk0, n_blk;
};
hipError_t launch_src_adj(const SrcAdjArgs& a, int din, int h, hipStream_t st);

// g[p][k][u] = cot[k][p][u] for k < n_cot, zeros for the padding cotangents
hipError_t launch_cot_transpose(const float* cot, int64_t n_pred, int64_t n_cot, int units, float* g, hipStream_t st);
// out[k][r][f] = lam[r][k][f] for k < n_cot, f < F: the feature columns of the cotangent of h0
hipError_t launch_feature_rows_adj(const float* lam, int64_t rows, int64_t n_cot, int H, int F, float* out, hipStream_t st);
