// gru_cell.h — launchers of the generalised GRU cell kernels (gru_cell.hip): the forward and backward
// of a cell whose activation, recurrent_activation, use_bias or reset_after differ from the Keras
// defaults (ign_plan_set_cell_options).  They take the argument blocks of the kernels they generalise
// (kernels.h, train_kernels.h) plus the options; the fragments they read are pack_gru's unscaled form.
#pragma once
#include "kernels.h"
#include "train_kernels.h"

struct CellOpt {
  int act;          // the candidate's activation code
  int ract;         // the gates'
  int reset_after;  // 0: c = act(x.W_h + b_h + (r * h).U_h), a second K = H sweep
};

// What the backward of a reset_after = 0 cell writes beside ga / gu, rows aligned with gu's: the
// recurrent-kernel gradient is dU = h^T gu + (r * h)^T gu2 with gu = (dz, dr, 0), gu2 = (0, 0, dc),
// two row contractions of tsgemm's.  Null for a reset_after cell (gu = (dz, dr, dc r) alone).
struct CellBwdExtra {
  float* gu2 = nullptr;   // [rows][3H]
  float* rh = nullptr;    // [rows][H] r * h_prev
};

// seq_gru2_kernel's update (H 16, 32, 64; hs_save: the training forward)
hipError_t launch_seq_gru_cell(const SeqGruArgs& args, int h, CellOpt o, hipStream_t st);
// sum_gru_kernel's (the four 16 / 32 shapes, with attention and convolution) and sum_gru_lds_kernel's
// (64 / 64, plain sums)
hipError_t launch_sum_gru_cell(const SumGruArgs& args, int din, int h, CellOpt o, hipStream_t st);
// seq_gru_bwd_kernel's unfused form: ga per step, gu (and x.gu2 / x.rh) per hs row
hipError_t launch_seq_gru_cell_bwd(const SeqBwdArgs& a, int h, CellOpt o, CellBwdExtra x, hipStream_t st);
// sum_gru_bwd_kernel's
hipError_t launch_sum_gru_cell_bwd(const SumBwdArgs& a, int din, int h, CellOpt o, CellBwdExtra x, hipStream_t st);
