// tangent.h — launchers of the dual-number GRU kernels (tangent.hip) behind ign_forward_tangent
// (tangent.cpp): one forward step of a state row h together with its tangent row hd = dh/d(eps) along
// a caller-given feature direction.  They take the argument blocks and lane layout of gru_cell.hip's
// forward kernels plus the tangent pointers, and read pack_gru's unscaled fragments and the combined
// bias block [4][H].
#pragma once
#include "gru_cell.h"

// Ordered update.  p: seq_gru_cell_kernel's block (hs_save and the split pieces unused); the tangent
// rides on the same order / len / step tables.
struct SeqTangentArgs {
  SeqGruArgs p;
  const float* hd_in;     // [rows][H] tangent of h_in
  float* hd_out;          // [rows][H] tangent of h_out
  const float* table_d;   // the tangent of p.table, row for row: xd.W, no bias
};

// Sum update (plain sums).  p: sum_gru_cell_kernel's block; the tangent of a message row lives at the
// same (slot, row) of src_d.
struct SumTangentArgs {
  SumGruArgs p;
  SrcBases src_d;
  const float* hd_in;
  float* hd_out;
};

// H 16, 32, 64 (gru_cell_seq_supported)
hipError_t launch_seq_gru_tangent(const SeqTangentArgs& a, int h, CellOpt o, hipStream_t st);
// the five shapes of gru_cell_sum_supported(din, h, 0)
hipError_t launch_sum_gru_tangent(const SumTangentArgs& a, int din, int h, CellOpt o, hipStream_t st);
