// kernel_shapes.h — the shapes the kernels are instantiated for and the floats their packed weight
// fragments take, for the plan lowering (plan_lower.cpp) and the launchers alike.  No HIP header.
// A launcher returns hipErrorInvalidValue for a shape its predicate refuses: that check ties each
// predicate here to its dispatch.
#pragma once
#include <stdint.h>

inline bool gru_shape_supported(int din, int h) {
  return ((din == 16 || din == 32) && (h == 16 || h == 32)) || (din == 64 && h == 64);
}
// the activation codes (ignmp.h's IGN_ACT_*, kernels.h's IGN_K_ACT_*): a launcher refuses any other
inline bool act_code_ok(int a) { return a >= 0 && a <= 9; }
// linear, relu, selu, sigmoid, tanh: the codes every templated kernel is instantiated for.  elu ..
// hard_sigmoid (5 .. 9) run on the runtime-switched kernels and on dense_h16's forward.
inline bool act_first_five(int a) { return a >= 0 && a <= 4; }
// The fused readouts (readout3, readout_bf, readout_h16, readout_h32) are instantiated for those five
// alone, and the scaled split-fp16 forms bound their layer-2 input by those activations' growth
// (DESIGN.md §3b'); a stack with any other code runs layer by layer.
inline bool fused_readout_acts(int act1, int act2, int act3) {
  return act1 == act2 && act_first_five(act1) && act_first_five(act3);
}
inline bool readout3_supported(int din, int n1, int n2, int act1, int act2, int act3) {
  return (din == 16 || din == 32 || din == 64) && n1 == 256 && n2 == 256 && fused_readout_acts(act1, act2, act3);
}
inline bool readout_bf_supported(int din, int n1, int n2, int act1, int act2, int act3) {
  return (din == 32 || din == 64) && n1 == 256 && n2 == 256 && fused_readout_acts(act1, act2, act3);
}
// dense_bf / dense_h16 and their transposed forms: K in {32, 64, 128, 256}, M a multiple of 128
inline bool dense_bf_supported(int K, int M) {
  // whole stages of G 16-unit tiles: G <= 8 for K < 256; K = 256 stages two tiles (NP = 2) or one,
  // so the readout's first-layer input gradient (K = 256 -> M = 32, RouteNet's state width) runs
  // here instead of on row_gemm_t's f32 MFMA
#ifndef IGN_DENSE_BF_M128
  if (K == 256) return M > 0 && M % 32 == 0;
#endif
  return (K == 32 || K == 64 || K == 128 || K == 256) && M % 128 == 0 && M > 0;
}
inline bool bwd_shape_supported(int din, int h) {
  return (din == 16 || din == 32 || din == 64) && (h == 16 || h == 32 || h == 64) && (h != 64 || din == 64) &&
         (din != 64 || h == 64);
}
inline bool seq_bwd_fused_supported(int h) { return h == 16 || h == 32; }
// the generalised cell kernels (gru_cell.hip): the ordered update and its backward at H 16 / 32 / 64;
// the sum update at the four 16 / 32 shapes in every mode (0 sum, 1 attention, 2 convolution: DIN = H)
// and at 64 / 64 as a plain sum; the sum backward (mode 0's predicate) at all five
inline bool gru_cell_seq_supported(int h) { return h == 16 || h == 32 || h == 64; }
inline bool gru_cell_sum_supported(int din, int h, int mode) {
  if (din == 64 && h == 64) return mode == 0;
  return (din == 16 || din == 32) && (h == 16 || h == 32) && mode >= 0 && mode <= 2 && (mode != 2 || din == h);
}
// pack_gru's mode: 0 the default cell (scaled fragments, bias [2][3H]); else kPackGruRaw | the raw
// bias tensor's rows (2: [2][3H], 1: [3H], 0: none, a block of zeros)
constexpr int kPackGruRaw = 4;
inline bool row_gemm_supported(int K, int M) {
  return (K == 48 || K == 96 || K == 192 || K == 256) && (M == 16 || M == 32 || M == 64 || M == 256);
}
inline bool dense_fwd_supported(int K, int M) {
  return (K == 16 || K == 32 || K == 48 || K == 64 || K == 96 || K == 128 || K == 256) &&
         (M == 16 || M == 32 || M == 64 || M == 128 || M == 256);
}

// floats of d_packed each pack launch writes (0: the launch is not instantiated for the shape)
inline int64_t pack_gru_w_floats(int din, int H) { return 3LL * din * H; }   // pack_gru's W / pack_a of W, U
inline int64_t pack_gru_u_floats(int H) { return 3LL * H * H; }
inline int64_t pack_gru_b_floats(int H) { return 4LL * H; }                  // the combined biases [4][H]
inline int64_t pack_u_bf16_floats(int H) { return (H == 32 || H == 64) ? 9LL * H * H / 2 : 0; }
inline int64_t pack_u_f16_floats(int H) { return (H == 32 || H == 64) ? 3LL * H * H + 64 : 0; }
inline int64_t pack_ut_f16_floats(int H) { return H == 32 ? 3LL * H * H + 64 : 0; }
inline int64_t pack_w_f16_floats(int K, int H) { return ((H == 32 || H == 64) && K % 32 == 0) ? 3LL * K * H + 64 : 0; }
inline int64_t pack_w_bf16_floats(int K, int H) { return ((H == 32 || H == 64) && K % 32 == 0) ? 9LL * K * H / 2 : 0; }
inline int64_t pack_dense_floats(int in, int out) { return (int64_t)in * out; }            // pack_dense(_pad), pack_a
inline int64_t pack_dense_bf16_floats(int in, int out) { return 3LL * in * out / 2; }      // three bf16 pieces
inline int64_t pack_dense_f16_floats(int in, int out) { return (int64_t)in * out + 64; }   // two fp16 pieces + header
// the fused readout's split-fp16 block: W2, header, W1, header (pack_readout_h16 / _h32)
inline int64_t pack_readout_h16_floats(int in1, int n1, int n2) {
  return pack_dense_f16_floats(n1, n2) + pack_dense_f16_floats(in1, n1);
}
inline int64_t attn_vectors_floats(int F) { return 2LL * F; }
