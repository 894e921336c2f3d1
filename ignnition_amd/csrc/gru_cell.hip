// gru_cell.hip — the GRU cell with the options of ign_plan_set_cell_options, on f32 MFMA
// (v_mfma_f32_16x16x4_f32), forward and backward.  Each kernel takes the structure, argument block and
// lane layout of the default-cell kernel it generalises (kernels.hip: seq_gru2_kernel, sum_gru_kernel,
// sum_gru_lds_kernel; train_kernels.hip: seq_gru_bwd_kernel's unfused form, sum_gru_bwd_kernel); a
// default cell never runs here, so those kernels stay as they were tuned.
//
// The cell (Keras GRUCell v2; a = x.W + b_in, gate column order z, r, h):
//   z = ract(a_z + h.U_z + b_z) ; r = ract(a_r + h.U_r + b_r)
//   reset_after:      c = act(a_h + r * (h.U_h + b_hh))
//   not reset_after:  c = act(a_h + (r * h).U_h)              (bias [3H]: b_hh = 0)
//   h' = z h + (1 - z) c
// The fragments are pack_gru's UNSCALED form (the default cell's carry the sigmoid / tanh exponent
// scales) and the combined bias block [4][H] = b_z, b_r, b_h(in), b_hh holds zeros where the cell has
// no bias, so no kernel needs a flag for use_bias.
//
// reset_after = 0 needs a second pass: z and r need all of h.U_z, h.U_r before (r * h).U_h can start.
// The state tile h[NT] is at once the accumulator layout and the B operand of the next contraction
// (kernels.hip's k order), so r * h is formed in registers and fed straight back as B: another K = H
// sweep, no LDS exchange.  Both cell forms take that order (gates, then the candidate's sweep on h or
// on r * h): one straight-line step.
//
// Backward (dh' = d; derivatives through the outputs, act_grad_out):
//   dz = d (h - c) ract'(z) ; dc = d (1 - z) act'(c)
//   reset_after:      dr = dc u_h ract'(r), u_h = h.U_h + b_hh ; da = (dz, dr, dc) ; du = (dz, dr, dc r)
//                     dh = d z + du.U^T
//   not reset_after:  drh = dc.U_h^T ; dr = drh h ract'(r) ; da = (dz, dr, dc)
//                     dh = d z + drh r + (dz, dr).(U_z, U_r)^T
//                     dU = h^T (dz, dr, 0) + (r h)^T (0, 0, dc): gu, and CellBwdExtra's gu2 / rh
//   dx = da.W^T (the callers' row_gemm_t / this file's sum backward)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "device_common.h"
#include "gru_cell.h"

namespace {

__device__ __forceinline__ const float* cell_src_ptr(const SrcBases& sb, uint32_t code, int din) {
  const uint32_t slot = code >> IGN_SLOT_SHIFT;
  const uint32_t row = code & IGN_ROW_MASK;
  const float* b = sb.base[0];
  if (slot == 1) b = sb.base[1];
  if (slot == 2) b = sb.base[2];
  if (slot == 3) b = sb.base[3];
  return b + (int64_t)row * din;
}

// acc[G][t] += M_G . v for the gates G in [G0, G1) of a float4-grouped fragment array M4
// ([3][NT][K / 16][64] x f4: one 16-B read per lane feeds 4 MFMAs); v: K / 16 B-operand tiles
template <int K, int H, int G0, int G1>
__device__ __forceinline__ void cell_sweep(const f4* M4, int lane, const f4 (&v)[K / 16], f4 (&acc)[3][H / 16]) {
  constexpr int NT = H / 16, K4 = K / 16;
#pragma unroll
  for (int s4 = 0; s4 < K4; ++s4)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int G = G0; G < G1; ++G) {
        const f4 w = M4[((G * NT + t) * K4 + s4) * 64 + lane];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[G][t] = MFMA(w[q], v[s4][q], acc[G][t]);
      }
}

// The recurrent half of a step and the gates.  in: a[0..2] = x.W + b_in (+ b_rec for z, r), uh = b_hh.
// out: z, r in a[0], a[1]; c in a[2]; uh = h.U_h + b_hh (reset_after) or (r h).U_h; rh = r * h
template <int H>
__device__ __forceinline__ void cell_gates(const f4* U4, int lane, const f4 (&h)[H / 16], f4 (&a)[3][H / 16],
                                           f4 (&uh)[H / 16], f4 (&rh)[H / 16], CellOpt o) {
  constexpr int NT = H / 16;
  f4 acc[3][NT], bh[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    acc[0][t] = a[0][t];
    acc[1][t] = a[1][t];
    acc[2][t] = uh[t];
  }
  cell_sweep<H, H, 0, 2>(U4, lane, h, acc);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      a[0][t][r] = act_apply(acc[0][t][r], o.ract);
      a[1][t][r] = act_apply(acc[1][t][r], o.ract);
      rh[t][r] = a[1][t][r] * h[t][r];
      bh[t][r] = o.reset_after ? h[t][r] : rh[t][r];
    }
  // the candidate's sweep runs once, after the gates, on h or on r * h (a select per element): one
  // straight-line path for both cell forms, no branch around an MFMA sweep
  cell_sweep<H, H, 2, 3>(U4, lane, bh, acc);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      uh[t][r] = acc[2][t][r];
      const float pre = o.reset_after ? a[2][t][r] + a[1][t][r] * uh[t][r] : a[2][t][r] + uh[t][r];
      a[2][t][r] = act_apply(pre, o.act);
    }
}

// ---------------------------------------------------------------------------------------------
// Ordered / interleave / concat update (seq_gru2_kernel): one wave per 16 length-sorted destinations,
// the recurrent fragments in LDS, the step input from the projected table (x.W + b_in, project_kernel
// on the unscaled fragments).
template <int H, bool SAVE>
__global__ __launch_bounds__(256) void seq_gru_cell_kernel(SeqGruArgs a, CellOpt o) {
  constexpr int NT = H / 16, K4 = H / 16;
  __shared__ float sbias[4 * H];
  __shared__ f4 su[3 * NT * K4 * 64];
  for (int i = threadIdx.x; i < 4 * H; i += blockDim.x) sbias[i] = a.bias[i];
  {
    const f4* s4 = reinterpret_cast<const f4*>(a.Up);
    for (int e = threadIdx.x; e < 3 * NT * K4 * 64; e += blockDim.x) su[e] = s4[e];
  }
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const float* tab = a.table + 4 * g;
  __syncthreads();
  const int64_t n_tiles = (a.n_dst + 15) / 16;
  for (int64_t tile = xcd_block(a.xcd_remap) * 4 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t pos = tile * 16 + j;
    const bool valid = pos < a.n_dst;
    const int row = valid ? a.order[pos] : 0;
    const int L = valid ? a.len[pos] : 0;
    const uint32_t* codes = a.step_code + (valid ? a.step_ptr[pos] : 0);
    f4 h[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) h[t] = valid ? ld4(a.h_in + (int64_t)row * H + 16 * t + 4 * g) : f4{0, 0, 0, 0};
    int Lmax = L;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) Lmax = max(Lmax, __shfl_xor(Lmax, s));
    float* hsv = nullptr;
    if constexpr (SAVE) {   // h_0 .. h_L of the sequence, seq_gru2_kernel's rows
      hsv = a.hs_save + (valid ? (int64_t)a.step_ptr[pos] + pos : 0) * H + 4 * g;
      if (valid) {
#pragma unroll
        for (int t = 0; t < NT; ++t) st4(hsv + 16 * t, h[t]);
      }
    }
    uint32_t code = codes[0];
    for (int t = 0; t < Lmax; ++t) {
      f4 x[3][NT], uh[NT], rh[NT];
      const float* p = tab + (int64_t)code * (3 * H);
#pragma unroll
      for (int G = 0; G < 3; ++G)
#pragma unroll
        for (int i = 0; i < NT; ++i) x[G][i] = ld4(p + G * H + 16 * i);
      const uint32_t next = codes[t + 1];   // (step_code is padded past every sequence)
#pragma unroll
      for (int i = 0; i < NT; ++i) uh[i] = *reinterpret_cast<const f4*>(sbias + 3 * H + 16 * i + 4 * g);
      cell_gates<H>(su, lane, h, x, uh, rh, o);
      const bool on = t < L;
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float c = x[2][i][r];
          const float hn = c + x[0][i][r] * (h[i][r] - c);
          h[i][r] = on ? hn : h[i][r];
        }
      if constexpr (SAVE) {
        if (on && valid) {
#pragma unroll
          for (int i = 0; i < NT; ++i) st4(hsv + (int64_t)(t + 1) * H + 16 * i, h[i]);
        }
      }
      code = next;
    }
    if (valid) {
#pragma unroll
      for (int t = 0; t < NT; ++t) st4(a.h_out + (int64_t)row * H + 16 * t + 4 * g, h[t]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Sum / attention / convolution aggregation, then one step (sum_gru_kernel's MODE 0 / 1 / 2 and its
// summation order).  LDSW (sum_gru_lds_kernel, 64 / 64): W and U staged in LDS once per block, the
// block persistent over the tiles; otherwise one tile per wave and the fragments from L2.
template <int DIN, int H, int MODE, bool LDSW, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void sum_gru_cell_kernel(SumGruArgs a, CellOpt o) {
  constexpr int NC = DIN / 16, NT = H / 16;
  constexpr int WF = 3 * NT * NC * 64, UF = 3 * NT * NT * 64;   // float4 fragments
  static_assert(MODE != 2 || DIN == H, "convolution needs message dim == destination dim");
  __shared__ f4 sW[LDSW ? WF : 1];
  __shared__ f4 sU[LDSW ? UF : 1];
  __shared__ float sbias[4 * H];
  for (int i = threadIdx.x; i < 4 * H; i += 64 * WAVES) sbias[i] = a.bias[i];
  if constexpr (LDSW) {
    const f4* gW = reinterpret_cast<const f4*>(a.Wp);
    const f4* gU = reinterpret_cast<const f4*>(a.Up);
    for (int i = threadIdx.x; i < WF; i += 64 * WAVES) sW[i] = gW[i];
    for (int i = threadIdx.x; i < UF; i += 64 * WAVES) sU[i] = gU[i];
  }
  __syncthreads();
  const f4* W4 = LDSW ? sW : reinterpret_cast<const f4*>(a.Wp);
  const f4* U4 = LDSW ? sU : reinterpret_cast<const f4*>(a.Up);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int64_t n_tiles = (a.n_dst + 15) / 16;
  for (int64_t tile = xcd_block(a.xcd_remap) * WAVES + wave; tile < n_tiles; tile += (int64_t)gridDim.x * WAVES) {
    const int64_t pos = tile * 16 + j;
    const bool valid = pos < a.n_dst;
    const int row = valid ? a.order[pos] : 0;
    const int64_t m0 = valid ? a.msg_ptr[pos] : 0;
    const int64_t m1 = valid ? a.msg_ptr[pos + 1] : 0;
    f4 x[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) x[c] = f4{0, 0, 0, 0};
    int64_t m = m0;
    if constexpr (MODE == 1) {
      for (; m < m1; ++m) {
        const float w = a.msg_w[m];
        const float* p = cell_src_ptr(a.src, a.msg_src[m], DIN);
#pragma unroll
        for (int c = 0; c < NC; ++c) x[c] += ld4(p + 16 * c + 4 * g) * w;
      }
    } else {
      for (; m + 4 <= m1; m += 4) {   // four rows in flight, added in CSR order
        const float* p0 = cell_src_ptr(a.src, a.msg_src[m], DIN);
        const float* p1 = cell_src_ptr(a.src, a.msg_src[m + 1], DIN);
        const float* p2 = cell_src_ptr(a.src, a.msg_src[m + 2], DIN);
        const float* p3 = cell_src_ptr(a.src, a.msg_src[m + 3], DIN);
        f4 v0[NC], v1[NC], v2[NC], v3[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          v0[c] = ld4(p0 + 16 * c + 4 * g);
          v1[c] = ld4(p1 + 16 * c + 4 * g);
          v2[c] = ld4(p2 + 16 * c + 4 * g);
          v3[c] = ld4(p3 + 16 * c + 4 * g);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) x[c] = (((x[c] + v0[c]) + v1[c]) + v2[c]) + v3[c];
      }
      for (; m < m1; ++m) {
        const float* p = cell_src_ptr(a.src, a.msg_src[m], DIN);
#pragma unroll
        for (int c = 0; c < NC; ++c) x[c] += ld4(p + 16 * c + 4 * g);
      }
    }
    f4 h[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) h[t] = valid ? ld4(a.h_in + (int64_t)row * H + 16 * t + 4 * g) : f4{0, 0, 0, 0};
    if constexpr (MODE == 2) {   // x = act((sum . K + h) / deg), AUX:384-401 (sum_gru_kernel)
      if (a.sum_save && valid) {
#pragma unroll
        for (int c = 0; c < NC; ++c) st4(a.sum_save + (int64_t)row * DIN + 16 * c + 4 * g, x[c]);
      }
      f4 y[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) y[c] = f4{0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < DIN / 4; ++s) {
        const float xb = x[s >> 2][s & 3];
#pragma unroll
        for (int t = 0; t < NC; ++t) y[t] = MFMA(a.conv_kp[frag_idx(t, s, DIN / 4, lane)], xb, y[t]);
      }
      const float deg = (float)(m1 - m0);
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float u = (y[c][r] + h[c][r]) / deg;   // relu(NaN) is NaN in the reference, not 0
          x[c][r] = u != u ? u : act_apply(u, a.conv_act);
        }
    }
    if (a.x_save && valid) {
#pragma unroll
      for (int c = 0; c < NC; ++c) st4(a.x_save + (int64_t)row * DIN + 16 * c + 4 * g, x[c]);
    }
    // (LDS form: an opaque lane offset keeps the loop-invariant fragment reads inside the tile loop)
    int wofs = lane;
    if constexpr (LDSW) asm volatile("" : "+v"(wofs));
    f4 acc[3][NT], uh[NT], rh[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int u0 = 16 * t + 4 * g;
      acc[0][t] = *reinterpret_cast<const f4*>(sbias + 0 * H + u0);
      acc[1][t] = *reinterpret_cast<const f4*>(sbias + 1 * H + u0);
      acc[2][t] = *reinterpret_cast<const f4*>(sbias + 2 * H + u0);
      uh[t] = *reinterpret_cast<const f4*>(sbias + 3 * H + u0);
    }
    cell_sweep<DIN, H, 0, 3>(W4, wofs, x, acc);
    cell_gates<H>(U4, wofs, h, acc, uh, rh, o);
    if (valid) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        f4 hn;
#pragma unroll
        for (int r = 0; r < 4; ++r) hn[r] = acc[2][t][r] + acc[0][t][r] * (h[t][r] - acc[2][t][r]);
        st4(a.h_out + (int64_t)row * H + 16 * t + 4 * g, hn);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The backward of one step for the wave's 16 rows, shared by the two backward kernels.
// in: hp = h_prev, d = dh', a = x.W + b_in (+ b_rec for z, r), uh = b_hh.  out: gz, gr, gh = da;
// guh = du's h gate (dc r; reset_after = 0: dc); rh = r * h_prev; acc = dh_prev.  Up4 / Ut: the
// forward's U fragments and pack_a's U^T fragments (tiles over H, k over 3H, gate-major).
template <int H>
__device__ __forceinline__ void cell_step_bwd(const f4* Up4, const float* Ut, int lane, const f4 (&hp)[H / 16],
                                              const f4 (&d)[H / 16], f4 (&a)[3][H / 16], f4 (&uh)[H / 16],
                                              f4 (&rh)[H / 16], f4 (&gz)[H / 16], f4 (&gr)[H / 16],
                                              f4 (&gh)[H / 16], f4 (&guh)[H / 16], f4 (&acc)[H / 16], CellOpt o) {
  constexpr int NT = H / 16, KH = H / 4, K3 = 3 * H / 4;
  cell_gates<H>(Up4, lane, hp, a, uh, rh, o);   // a = z, r, c; uh = u_h or (r h).U_h
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z = a[0][t][r], c = a[2][t][r];
      gz[t][r] = d[t][r] * (hp[t][r] - c) * act_grad_out(z, o.ract);
      gh[t][r] = d[t][r] * (1.f - z) * act_grad_out(c, o.act);
      acc[t][r] = d[t][r] * z;
    }
  if (o.reset_after) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float rr = a[1][t][r];
        gr[t][r] = gh[t][r] * uh[t][r] * act_grad_out(rr, o.ract);
        guh[t][r] = gh[t][r] * rr;
      }
  } else {
    // drh = dc . U_h^T: the h gate's k range of the U^T fragments (16-column tiles 2 NT .. 3 NT - 1)
    f4 drh[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) drh[t] = f4{0, 0, 0, 0};
#pragma unroll
    for (int s = 2 * KH; s < K3; ++s) {
      const float b = gh[(s >> 2) - 2 * NT][s & 3];
#pragma unroll
      for (int t = 0; t < NT; ++t) drh[t] = MFMA(Ut[frag_idx(t, s, K3, lane)], b, drh[t]);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float rr = a[1][t][r];
        gr[t][r] = drh[t][r] * hp[t][r] * act_grad_out(rr, o.ract);
        acc[t][r] += drh[t][r] * rr;
        guh[t][r] = gh[t][r];
      }
  }
  // dh_prev += du . U^T over the gates whose pre-activation reads h.U: z, r (and h under reset_after)
#pragma unroll
  for (int s = 0; s < 2 * KH; ++s) {
    const int gt = s >> 2;
    const float b = gt < NT ? gz[gt][s & 3] : gr[gt - NT][s & 3];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = MFMA(Ut[frag_idx(t, s, K3, lane)], b, acc[t]);
  }
  if (o.reset_after) {
#pragma unroll
    for (int s = 2 * KH; s < K3; ++s) {
      const float b = guh[(s >> 2) - 2 * NT][s & 3];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = MFMA(Ut[frag_idx(t, s, K3, lane)], b, acc[t]);
    }
  }
}

// da / du rows of one step (and gu2 / rh under reset_after = 0)
template <int H>
__device__ __forceinline__ void cell_store_grads(float* pa, float* pu, float* pu2, float* prh, int g,
                                                 const f4 (&gz)[H / 16], const f4 (&gr)[H / 16],
                                                 const f4 (&gh)[H / 16], const f4 (&guh)[H / 16],
                                                 const f4 (&rh)[H / 16], CellOpt o) {
  constexpr int NT = H / 16;
  const f4 zero = f4{0, 0, 0, 0};
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int u = 16 * t + 4 * g;
    st4(pa + u, gz[t]);
    st4(pa + H + u, gr[t]);
    st4(pa + 2 * H + u, gh[t]);
    st4(pu + u, gz[t]);
    st4(pu + H + u, gr[t]);
    st4(pu + 2 * H + u, o.reset_after ? guh[t] : zero);
    if (!o.reset_after) {
      st4(pu2 + u, zero);
      st4(pu2 + H + u, zero);
      st4(pu2 + 2 * H + u, gh[t]);
      st4(prh + u, rh[t]);
    }
  }
}

// Ordered update backward (seq_gru_bwd_kernel's unfused form): one wave = the forward's 16-row tile,
// steps in reverse; a lane past its sequence passes its gradient through.  H <= 32: U and U^T in LDS.
template <int H>
__global__ __launch_bounds__(256) void seq_gru_cell_bwd_kernel(SeqBwdArgs a, CellOpt o, CellBwdExtra e) {
  constexpr int NT = H / 16;
  constexpr bool LDSU = H <= 32;
  constexpr int NU = 3 * H * H;   // floats of the U fragments, and of U^T's
  __shared__ float sUp[LDSU ? NU : 4];
  __shared__ float sUt[LDSU ? NU : 4];
  if constexpr (LDSU) {
    for (int i = threadIdx.x; i < NU / 4; i += blockDim.x) {
      reinterpret_cast<f4*>(sUp)[i] = reinterpret_cast<const f4*>(a.Up)[i];
      reinterpret_cast<f4*>(sUt)[i] = reinterpret_cast<const f4*>(a.Ut)[i];
    }
    __syncthreads();
  }
  const f4* Up4 = reinterpret_cast<const f4*>(LDSU ? sUp : a.Up);
  const float* Ut = LDSU ? sUt : a.Ut;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int64_t pos = ((int64_t)blockIdx.x * 4 + wave) * 16 + j;
  const bool valid = pos < a.n_dst;
  const int row = valid ? a.order[pos] : 0;
  const int L = valid ? a.len[pos] : 0;
  const int64_t sp = valid ? a.step_ptr[pos] : 0;
  const int64_t hbase = sp + (valid ? pos : 0);
  f4 dh[NT], bh[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    dh[t] = valid ? ld4(a.dh_in + (int64_t)row * H + 16 * t + 4 * g) : f4{0, 0, 0, 0};
    bh[t] = ld4(a.bias + 3 * H + 16 * t + 4 * g);
  }
  int Lmax = L;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) Lmax = max(Lmax, __shfl_xor(Lmax, s));
  for (int step = Lmax - 1; step >= 0; --step) {
    const bool on = step < L;
    const int64_t tt = on ? step : 0;       // a lane past its sequence recomputes its step 0, masked
    const int64_t i = sp + tt, hr = hbase + tt;
    // h_prev: step 0's is the state before the MP (the batched forward also saves it as hs row hbase)
    const float* hsrc = tt == 0 ? a.h_in + (int64_t)row * H : a.hs + hr * H;
    const uint32_t code = a.step_code[i];
    f4 hp[NT], x[3][NT], d[NT], uh[NT], rh[NT], gz[NT], gr[NT], gh[NT], guh[NT], acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      hp[t] = ld4(hsrc + 16 * t + 4 * g);
      uh[t] = bh[t];
#pragma unroll
      for (int r = 0; r < 4; ++r) d[t][r] = on ? dh[t][r] : 0.f;
#pragma unroll
      for (int G = 0; G < 3; ++G) x[G][t] = ld4(a.table + (int64_t)code * (3 * H) + G * H + 16 * t + 4 * g);
    }
    cell_step_bwd<H>(Up4, Ut, lane, hp, d, x, uh, rh, gz, gr, gh, guh, acc, o);
    if (on)
      cell_store_grads<H>(a.ga + i * (3 * H), a.gu + hr * (3 * H), e.gu2 ? e.gu2 + hr * (3 * H) : nullptr,
                          e.rh ? e.rh + hr * H : nullptr, g, gz, gr, gh, guh, rh, o);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) dh[t][r] = on ? acc[t][r] : dh[t][r];
  }
  if (valid) {
    const f4 zero = f4{0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < NT; ++t) st4(a.dh_out + (int64_t)row * H + 16 * t + 4 * g, dh[t]);
    // the final state's row has no step: zeros, so the row contractions over all hs rows skip it
    const int64_t fr = hbase + L;
#pragma unroll
    for (int t = 0; t < 3 * NT; ++t) {
      st4(a.gu + fr * (3 * H) + 16 * t + 4 * g, zero);
      if (!o.reset_after) st4(e.gu2 + fr * (3 * H) + 16 * t + 4 * g, zero);
    }
    if (!o.reset_after) {
#pragma unroll
      for (int t = 0; t < NT; ++t) st4(e.rh + fr * H + 16 * t + 4 * g, zero);
    }
  }
}

// Sum update backward (sum_gru_bwd_kernel): one wave = 16 destination rows, identity order.
template <int DIN, int H>
__global__ __launch_bounds__(256) void sum_gru_cell_bwd_kernel(SumBwdArgs a, CellOpt o, CellBwdExtra e) {
  constexpr int NC = DIN / 16, NT = H / 16, K3 = 3 * H / 4;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * 16 + j;
  const bool valid = row < a.n_dst;
  const int64_t rr0 = valid ? row : 0;
  f4 x[NC], h[NT], d[NT], acc3[3][NT], uh[NT], rh[NT], gz[NT], gr[NT], gh[NT], guh[NT], acc[NT];
#pragma unroll
  for (int c = 0; c < NC; ++c) x[c] = ld4(a.x + rr0 * DIN + 16 * c + 4 * g);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    h[t] = ld4(a.h + rr0 * H + 16 * t + 4 * g);
    d[t] = valid ? ld4(a.dh_in + rr0 * H + 16 * t + 4 * g) : f4{0, 0, 0, 0};
    acc3[0][t] = ld4(a.bias + 0 * H + 16 * t + 4 * g);
    acc3[1][t] = ld4(a.bias + 1 * H + 16 * t + 4 * g);
    acc3[2][t] = ld4(a.bias + 2 * H + 16 * t + 4 * g);
    uh[t] = ld4(a.bias + 3 * H + 16 * t + 4 * g);
  }
  cell_sweep<DIN, H, 0, 3>(reinterpret_cast<const f4*>(a.Wp), lane, x, acc3);
  cell_step_bwd<H>(reinterpret_cast<const f4*>(a.Up), a.Ut, lane, h, d, acc3, uh, rh, gz, gr, gh, guh, acc, o);
  f4 dxa[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) dxa[c] = f4{0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < K3; ++s) {   // dx = da . W^T
    const int gt = s >> 2, G = gt / NT, t2 = gt % NT;
    const float b = G == 0 ? gz[t2][s & 3] : G == 1 ? gr[t2][s & 3] : gh[t2][s & 3];
#pragma unroll
    for (int c = 0; c < NC; ++c) dxa[c] = MFMA(a.Wt[frag_idx(c, s, K3, lane)], b, dxa[c]);
  }
  if (valid) {
#pragma unroll
    for (int t = 0; t < NT; ++t) st4(a.dh_out + row * H + 16 * t + 4 * g, acc[t]);
    cell_store_grads<H>(a.ga + row * (3 * H), a.gu + row * (3 * H), e.gu2 ? e.gu2 + row * (3 * H) : nullptr,
                        e.rh ? e.rh + row * H : nullptr, g, gz, gr, gh, guh, rh, o);
#pragma unroll
    for (int c = 0; c < NC; ++c) st4(a.dx + row * DIN + 16 * c + 4 * g, dxa[c]);
  }
}

int grid_for(int64_t n, int per_block) { return (int)((n + per_block - 1) / per_block); }

// resident blocks per CU x CUs, at most the work (a persistent grid); the device's answer is asked
// once per kernel (KERNEL: a template argument, so each instantiation keeps its own)
template <auto KERNEL, int BLOCK>
int persistent_grid(int64_t n_blocks_of_work) {
  static const int64_t resident = [] {
    int dev = 0, cus = 0, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus <= 0) cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, KERNEL, BLOCK, 0) != hipSuccess || per_cu <= 0) per_cu = 1;
    return (int64_t)per_cu * cus;
  }();
  return (int)std::max<int64_t>(1, std::min<int64_t>(resident, n_blocks_of_work));
}

template <int H>
hipError_t seq_cell_launch(const SeqGruArgs& args, CellOpt o, hipStream_t st) {
  const int64_t work = grid_for(args.n_dst, 64);
  if (args.hs_save)
    hipLaunchKernelGGL((seq_gru_cell_kernel<H, true>), dim3(persistent_grid<seq_gru_cell_kernel<H, true>, 256>(work)),
                       dim3(256), 0, st, args, o);
  else
    hipLaunchKernelGGL((seq_gru_cell_kernel<H, false>), dim3(persistent_grid<seq_gru_cell_kernel<H, false>, 256>(work)),
                       dim3(256), 0, st, args, o);
  return hipGetLastError();
}

// the sum update at a 16 / 32 shape: one tile per wave; convolution (mode 2) exists for DIN = H alone
template <int D, int HH>
hipError_t sum_cell_launch(const SumGruArgs& args, int mode, CellOpt o, dim3 grid, hipStream_t st) {
  if (mode == 1) hipLaunchKernelGGL((sum_gru_cell_kernel<D, HH, 1, false, 4>), grid, dim3(256), 0, st, args, o);
  else if (mode == 2) {
    if constexpr (D == HH) hipLaunchKernelGGL((sum_gru_cell_kernel<D, HH, 2, false, 4>), grid, dim3(256), 0, st, args, o);
    else return hipErrorInvalidValue;
  } else hipLaunchKernelGGL((sum_gru_cell_kernel<D, HH, 0, false, 4>), grid, dim3(256), 0, st, args, o);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_seq_gru_cell(const SeqGruArgs& args, int h, CellOpt o, hipStream_t st) {
  if (!gru_cell_seq_supported(h) || !act_code_ok(o.act) || !act_code_ok(o.ract)) return hipErrorInvalidValue;
  if (args.n_dst == 0) return hipSuccess;
  switch (h) {
    case 16: return seq_cell_launch<16>(args, o, st);
    case 32: return seq_cell_launch<32>(args, o, st);
    case 64: return seq_cell_launch<64>(args, o, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_sum_gru_cell(const SumGruArgs& args, int din, int h, CellOpt o, hipStream_t st) {
  const int mode = args.conv_kp ? 2 : args.msg_w ? 1 : 0;
  if (!gru_cell_sum_supported(din, h, mode) || !act_code_ok(o.act) || !act_code_ok(o.ract) ||
      (mode == 2 && !act_code_ok(args.conv_act)) || args.proj_out)
    return hipErrorInvalidValue;
  if (args.n_dst == 0) return hipSuccess;
  const dim3 grid(grid_for(args.n_dst, 64));
  if (din == 32 && h == 32) return sum_cell_launch<32, 32>(args, mode, o, grid, st);
  if (din == 16 && h == 16) return sum_cell_launch<16, 16>(args, mode, o, grid, st);
  if (din == 16 && h == 32) return sum_cell_launch<16, 32>(args, mode, o, grid, st);
  if (din == 32 && h == 16) return sum_cell_launch<32, 16>(args, mode, o, grid, st);
  if (din == 64 && h == 64) {   // (mode 0: the predicate)
    constexpr int WV = 12;
    const int64_t work = (args.n_dst + 16 * WV - 1) / (16 * WV);
    hipLaunchKernelGGL((sum_gru_cell_kernel<64, 64, 0, true, WV>),
                       dim3(persistent_grid<sum_gru_cell_kernel<64, 64, 0, true, WV>, 64 * WV>(work)), dim3(64 * WV), 0, st,
                       args, o);
    return hipGetLastError();
  }
  return hipErrorInvalidValue;
}

hipError_t launch_seq_gru_cell_bwd(const SeqBwdArgs& a, int h, CellOpt o, CellBwdExtra x, hipStream_t st) {
  if (!gru_cell_seq_supported(h) || !act_code_ok(o.act) || !act_code_ok(o.ract)) return hipErrorInvalidValue;
  if (!a.h_in || !a.gu || !a.ga || (!o.reset_after && (!x.gu2 || !x.rh))) return hipErrorInvalidValue;
  if (a.n_dst == 0) return hipSuccess;
  const dim3 grid((unsigned)((a.n_dst + 63) / 64));
  switch (h) {
    case 16: hipLaunchKernelGGL((seq_gru_cell_bwd_kernel<16>), grid, dim3(256), 0, st, a, o, x); break;
    case 32: hipLaunchKernelGGL((seq_gru_cell_bwd_kernel<32>), grid, dim3(256), 0, st, a, o, x); break;
    case 64: hipLaunchKernelGGL((seq_gru_cell_bwd_kernel<64>), grid, dim3(256), 0, st, a, o, x); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_sum_gru_cell_bwd(const SumBwdArgs& a, int din, int h, CellOpt o, CellBwdExtra x, hipStream_t st) {
  if (!gru_cell_sum_supported(din, h, 0) || !act_code_ok(o.act) || !act_code_ok(o.ract)) return hipErrorInvalidValue;
  if (!o.reset_after && (!x.gu2 || !x.rh)) return hipErrorInvalidValue;
  if (a.n_dst == 0) return hipSuccess;
  const dim3 grid((unsigned)((a.n_dst + 63) / 64));
#define SB_CELL(D, HH)                                                                          \
  if (din == D && h == HH) {                                                                    \
    hipLaunchKernelGGL((sum_gru_cell_bwd_kernel<D, HH>), grid, dim3(256), 0, st, a, o, x);      \
    return hipGetLastError();                                                                   \
  }
  SB_CELL(32, 32)
  SB_CELL(16, 16)
  SB_CELL(16, 32)
  SB_CELL(32, 16)
  SB_CELL(64, 64)
#undef SB_CELL
  return hipErrorInvalidValue;
}
