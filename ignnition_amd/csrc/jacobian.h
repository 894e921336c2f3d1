// jacobian.h — launchers of the kernels behind ign_forward_jacobian (jacobian.hip, jacobian.cpp): K
// feature directions through ONE linearised forward.  The primal runs once on ordinary
// rows and leaves, per (destination, step), the five coefficient rows [H] of the tangent update
//   hd' = z hd + P gz + R gr + Q ad_h + S gh,   gz = ad_z + hd.U_z, gr = ad_r + hd.U_r, gh = hd.U_h
// (kJacCoef rows, in the order z, P, R, Q, S); the K tangents then run a purely linear recurrence in
// scenario.hip's layout with the 16 rows of an MFMA tile on the DIRECTION axis: Kp = K rounded up to
// 16, tangent states [row][Kp][H], tangent tables [table row][Kp][3H] (scenario_layout.h).  The
// kernels read pack_gru's unscaled fragments and the combined bias block [4][H]; cells are reset_after.
#pragma once
#include "gru_cell.h"
#include "scenario_layout.h"

constexpr int kJacCoef = 5;   // z, P = (h - c) z', R = Q r' u, Q = (1 - z) c', S = Q r

// Linearising primal, ordered update: seq_gru_tangent's primal on p (hs_save and the split pieces
// unused), plus coef[step_ptr[pos] + t][kJacCoef][H] for every real step t < len[pos].
hipError_t launch_seq_gru_lin(const SeqGruArgs& p, float* coef, int h, CellOpt o, hipStream_t st);
// Linearising primal, sum update: sum_gru_tangent's primal on p, plus coef[pos][kJacCoef][H].
hipError_t launch_sum_gru_lin(const SumGruArgs& p, float* coef, int din, int h, CellOpt o, hipStream_t st);

// Tangent, ordered update over the batch's own order / len / step tables.
struct SeqJacArgs {
  const float* hd_in;          // [rows][Kp][H]
  float* hd_out;
  const float* table_d;        // [sources' rows | hole row | multi rows][Kp][3H]: xd.W, no bias
  const float* coef;           // [n_steps][kJacCoef][H]
  const int32_t* order;
  const int32_t* len;
  const int32_t* step_ptr;
  const uint32_t* step_code;
  const float* Up;             // pack_gru's unscaled U fragments
  int64_t n_dst;
  int32_t n_blk;               // Kp / 16
};
// Tangent, sum update over the MP's own CSR (plain sums), message code = slot << 29 | row.
struct SumJacArgs {
  const float* hd_in;          // [rows][Kp][H]
  float* hd_out;
  SrcBases src_d;              // per slot [rows][Kp][DIN]
  const float* coef;           // [n_dst][kJacCoef][H] per order position
  const int32_t* order;
  const int32_t* msg_ptr;
  const uint32_t* msg_src;
  const float* Wp;
  const float* Up;
  int64_t n_dst;
  int32_t n_blk;
};
// jacobian_shape_supported(h, h) / (din, h)
hipError_t launch_seq_gru_jac(const SeqJacArgs& a, int h, hipStream_t st);
hipError_t launch_sum_gru_jac(const SumJacArgs& a, int din, int h, hipStream_t st);

// state[r][k] = [dir[k][r] | 0] for k < n_dir, zeros for the padding directions; dir [n_dir][rows][F] or
// null (zeros everywhere).  H 16, 32, 64
hipError_t launch_init_dir(float* state, const float* dir, int64_t rows, int64_t n_dir, int H, int F, hipStream_t st);
// the tangent table's hole row (zeros, all Kp directions) and its multi rows (per direction, the sum of
// the listed projected rows; a listed hole row adds nothing); W = 3H
hipError_t launch_table_rows_jac(float* table, int64_t zero_row, int64_t n_multi, const int32_t* ptr,
                                 const uint32_t* rows, int W, int64_t kp, hipStream_t st);
// dz[r * kp + k][c] = da[r * kp + k][c] act'(y[r][c]), act' through the output y (act_grad_out)
hipError_t launch_act_bwd_bcast(const float* da, const float* y, int64_t rows, int64_t kp, int width, int act, float* dz,
                                hipStream_t st);
// out[k][p][u] = yd[p][k][u] for k < n_dir: the padding directions stay behind
hipError_t launch_gather_dpred(const float* yd, int64_t n_pred, int64_t n_dir, int units, float* out, hipStream_t st);
