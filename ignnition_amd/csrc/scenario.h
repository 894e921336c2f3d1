// scenario.h — launchers of the scenario-major GRU kernels (scenario.hip) behind ign_forward_scenarios
// (scenario.cpp): S feature sets on one topology in one pass.  Every state array is
// [row][Sp][H] with Sp = S rounded up to 16, a projected table [table row][Sp][3H]: a 16-row MFMA tile
// is 16 consecutive scenarios of ONE row, so a tile has one length, one step code per step and one
// CSR range, and every block it loads is contiguous.  The kernels read pack_gru's unscaled fragments
// and the combined bias block [4][H] of a default cell.
#pragma once
#include "kernels.h"
#include "scenario_layout.h"

// Ordered / interleave / concat (axis 1) update, the batch's own order / len / step tables.
struct SeqScenArgs {
  const float* h_in;           // [rows][Sp][H]
  float* h_out;
  const float* table;          // [sources' rows | hole row | multi rows][Sp][3H]
  const int32_t* order;        // [n_dst] destination rows, longest sequence first
  const int32_t* len;
  const int32_t* step_ptr;
  const uint32_t* step_code;   // table row of every step
  const float* Up;             // pack_gru's unscaled U fragments
  const float* bias;           // [4][H]
  int64_t n_dst;
  int32_t n_blk;               // Sp / 16
};

// Sum update over the MP's own CSR (plain sums), message code = slot << 29 | row.
struct SumScenArgs {
  const float* h_in;           // [rows][Sp][H]
  float* h_out;
  SrcBases src;                // per slot [rows][Sp][DIN]
  const int32_t* order;
  const int32_t* msg_ptr;      // [n_dst + 1] per order position
  const uint32_t* msg_src;
  const float* Wp;
  const float* Up;
  const float* bias;
  int64_t n_dst;
  int32_t n_blk;
};

// state[r][s] = [feat row | 0]: feat [n_scen][rows][F] (scen) or [rows][F] for every scenario (shared),
// neither: zeros; a padding scenario s >= n_scen copies scenario n_scen - 1.  H 16, 32, 64
hipError_t launch_init_state_scen(float* state, const float* scen, const float* shared, int64_t rows, int64_t n_scen,
                                  int H, int F, hipStream_t st);
// the table's hole row (bias alone, all Sp scenarios) and its multi rows (per scenario, the sum of the
// listed projected rows carrying the bias once: multi_sum_kernel's arithmetic); W = 3H
hipError_t launch_table_rows_scen(float* table, int64_t zero_row, int64_t n_multi, const int32_t* ptr,
                                  const uint32_t* rows, const float* bias, int W, int64_t sp, hipStream_t st);
// With coef (16-byte aligned) the two updates also store the linearisation of every real step, PER
// SCENARIO (ign_backward_scenarios): the rows (z, P, R, Q, S) of jacobian.h as tiles
// [item][n_blk][kScenCoef][16][H], item = the step's index in step_code (ordered) or the order position
// (sum), so the five [16][H] blocks of a tile-step are contiguous.  The states written are the same bits
// with and without.
constexpr int kScenCoef = 5;
inline int64_t scen_coef_floats(int64_t items, int64_t n_blk, int H) { return items * n_blk * kScenCoef * 16 * H; }
// With keep (16-byte aligned, coef given) they also store what a weight gradient contracts the adjoint's
// products with (ign_backward_scenarios_params): the ordered update the state in front of
// every real step, one [16][H] tile per (step, block) -- row-major, i.e. the flat rows step * Sp + s, or with
// keep_t transposed [H][16] --, the sum update its summed messages [order position][Sp][DIN].
// scen_seq_supported(h)
hipError_t launch_seq_gru_scen(const SeqScenArgs& a, int h, hipStream_t st, float* coef = nullptr, float* keep = nullptr,
                               bool keep_t = false);
// scen_sum_supported(din, h)
hipError_t launch_sum_gru_scen(const SumScenArgs& a, int din, int h, hipStream_t st, float* coef = nullptr,
                               float* keep = nullptr);
// out[s][p][u] = y[p][s][u] for s < n_scen: the padding scenarios stay behind
hipError_t launch_gather_pred_scen(const float* y, int64_t n_pred, int64_t n_scen, int units, float* out, hipStream_t st);
