// jacobian.hip — K feature directions through one linearised forward, on f32 MFMA
// (v_mfma_f32_16x16x4_f32), behind ign_forward_jacobian.
//
// The dual step of tangent.hip for a reset_after cell, derivatives through the outputs (act_grad_out):
//   gz = ad_z + hd.U_z ; gr = ad_r + hd.U_r ; gh = hd.U_h
//   hd' = z hd + P gz + R gr + Q ad_h + S gh
//   P = (h - c) z' ; Q = (1 - z) c' ; R = Q r' u ; S = Q r        (u = h.U_h + b_hh)
// Every factor but (hd, ad) is primal and does not depend on the direction.  So two kernel families:
//   * the LINEARISING PRIMAL (seq_gru_lin, sum_gru_lin) is the tangent kernels' primal on ordinary rows
//     -- their lane layout, tile walk and accumulation order, so the states are their bits -- and its
//     gate epilogue stores the five rows (z, P, R, Q, S) of every real step with 16-byte stores;
//   * the TANGENT kernels (seq_gru_jac, sum_gru_jac) run the linear recurrence above for all K
//     directions in scenario.hip's layout: Kp = K rounded up to 16, states [row][Kp][H], tables
//     [table row][Kp][3H], a wave owns (order position, direction block), so every lane of a tile is
//     the same destination.  No exp, no tanh, no select, no mask; one step code per wave and step; a
//     step's [16][3H] block and its coefficient rows are fetched 16-byte-wise one step ahead; a
//     coefficient row is the same for the 16 directions of a tile, so a lane's four units are one
//     broadcast float4.  One sweep over U feeds gz, gr and gh; hd stays in registers for a sequence.
// A padding direction is a zero row and stays one.  Every tangent operation is linear in (hd, ad): zero
// directions give zeros, a power-of-two scale commutes with every rounding, and an MFMA column depends
// on its own B column only, so a direction's bits depend neither on K nor on its index.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "device_common.h"
#include "jacobian.h"

namespace {

// acc[G][t] += M_G . v for the three gates of a float4-grouped fragment array ([3][NT][K / 16][64] x f4):
// per accumulator the k order of cell_sweep
template <int K, int H>
__device__ __forceinline__ void sweep3(const f4* M4, int lane, const f4 (&v)[K / 16], f4 (&acc)[3][H / 16]) {
  constexpr int NT = H / 16, K4 = K / 16;
#pragma unroll
  for (int s4 = 0; s4 < K4; ++s4)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int G = 0; G < 3; ++G) {
        const f4 w = M4[((G * NT + t) * K4 + s4) * 64 + lane];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[G][t] = MFMA(w[q], v[s4][q], acc[G][t]);
      }
}

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// One primal step of a reset_after cell for the wave's 16 rows, and its linearisation.  a: x.W + b
// (+ b_rec for z, r); out: hn = h', cf = (z, P, R, Q, S).
template <int H>
__device__ __forceinline__ void lin_step(const f4* U4, int lane, const f4 (&h)[H / 16], const f4 (&a)[3][H / 16],
                                         const f4 (&bhh)[H / 16], CellOpt o, f4 (&hn)[H / 16],
                                         f4 (&cf)[kJacCoef][H / 16]) {
  constexpr int NT = H / 16;
  f4 acc[3][NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    acc[0][t] = a[0][t];
    acc[1][t] = a[1][t];
    acc[2][t] = bhh[t];
  }
  sweep3<H, H>(U4, lane, h, acc);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z = act_apply(acc[0][t][r], o.ract), rr = act_apply(acc[1][t][r], o.ract);
      const float uu = acc[2][t][r];
      // r u rounded on its own, then added: the tangent kernels' candidate (their select between the two
      // reset forms keeps the product out of an fma), whose bits this primal has to give
      float ru = rr * uu;
      asm volatile("" : "+v"(ru));
      const float pre = a[2][t][r] + ru;
      const float c = act_apply(pre, o.act);
      const float hc = h[t][r] - c;
      hn[t][r] = c + z * hc;
      const float Q = (1.f - z) * act_grad_out(c, o.act);
      cf[0][t][r] = z;
      cf[1][t][r] = hc * act_grad_out(z, o.ract);
      cf[2][t][r] = Q * act_grad_out(rr, o.ract) * uu;
      cf[3][t][r] = Q;
      cf[4][t][r] = Q * rr;
    }
}

// ---------------------------------------------------------------------------------------------
// Linearising primal, ordered update: seq_gru_tangent_kernel's primal (one wave per 16 length-sorted
// destinations, U in LDS once per block, a lane past its sequence passes h through).  A lane inside
// its sequence stores the step's coefficient rows; a padding position stores nothing.
template <int H>
__global__ __launch_bounds__(256) void seq_gru_lin_kernel(SeqGruArgs a, float* __restrict__ coef, CellOpt o) {
  constexpr int NT = H / 16, CF = kJacCoef * H;
  __shared__ float sbhh[H];
  __shared__ f4 su[3 * NT * NT * 64];
  for (int i = threadIdx.x; i < H; i += blockDim.x) sbhh[i] = a.bias[3 * H + i];
  {
    const f4* s4 = reinterpret_cast<const f4*>(a.Up);
    for (int e = threadIdx.x; e < 3 * NT * NT * 64; e += blockDim.x) su[e] = s4[e];
  }
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const float* tab = a.table + 4 * g;
  __syncthreads();
  const int64_t n_tiles = (a.n_dst + 15) / 16;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t pos = tile * 16 + j;
    const bool valid = pos < a.n_dst;
    const int row = valid ? a.order[pos] : 0;
    const int L = valid ? a.len[pos] : 0;
    const int s0 = valid ? a.step_ptr[pos] : 0;
    const uint32_t* codes = a.step_code + s0;
    float* cfp = coef + (int64_t)s0 * CF + 4 * g;
    f4 h[NT], bhh[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      h[t] = valid ? ld4(a.h_in + (int64_t)row * H + 16 * t + 4 * g) : f4{0, 0, 0, 0};
      bhh[t] = *reinterpret_cast<const f4*>(sbhh + 16 * t + 4 * g);
    }
    int Lmax = L;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) Lmax = max(Lmax, __shfl_xor(Lmax, s));
    uint32_t code = codes[0];
    for (int t = 0; t < Lmax; ++t) {
      f4 x[3][NT], hn[NT], cf[kJacCoef][NT];
      const int64_t ofs = (int64_t)code * (3 * H);
#pragma unroll
      for (int G = 0; G < 3; ++G)
#pragma unroll
        for (int i = 0; i < NT; ++i) x[G][i] = ld4(tab + ofs + G * H + 16 * i);
      const uint32_t next = codes[t + 1];   // (step_code is padded past every sequence)
      lin_step<H>(su, lane, h, x, bhh, o, hn, cf);
      if (t < L) {
#pragma unroll
        for (int i = 0; i < NT; ++i) h[i] = hn[i];
#pragma unroll
        for (int c = 0; c < kJacCoef; ++c)
#pragma unroll
          for (int i = 0; i < NT; ++i) st4(cfp + (int64_t)t * CF + c * H + 16 * i, cf[c][i]);
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
// Linearising primal, sum update: sum_gru_tangent_kernel's primal (one tile per wave, four message rows
// in flight added in CSR order, x.W then the step; LDSW (64 / 64): W and U in LDS once per block, the
// block persistent).  coef is indexed by order position.
__device__ __forceinline__ const float* msg_row(const SrcBases& sb, uint32_t code, int64_t row_floats) {
  const uint32_t slot = code >> IGN_SLOT_SHIFT;
  const float* b = sb.base[0];
  if (slot == 1) b = sb.base[1];
  if (slot == 2) b = sb.base[2];
  if (slot == 3) b = sb.base[3];
  return b + (int64_t)(code & IGN_ROW_MASK) * row_floats;
}

template <int DIN, int H, bool LDSW, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void sum_gru_lin_kernel(SumGruArgs a, float* __restrict__ coef, CellOpt o) {
  constexpr int NC = DIN / 16, NT = H / 16, CF = kJacCoef * H;
  constexpr int WF = 3 * NT * NC * 64, UF = 3 * NT * NT * 64;   // float4 fragments
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
  for (int64_t tile = (int64_t)blockIdx.x * WAVES + wave; tile < n_tiles; tile += (int64_t)gridDim.x * WAVES) {
    const int64_t pos = tile * 16 + j;
    const bool valid = pos < a.n_dst;
    const int row = valid ? a.order[pos] : 0;
    const int64_t m0 = valid ? a.msg_ptr[pos] : 0;
    const int64_t m1 = valid ? a.msg_ptr[pos + 1] : 0;
    f4 x[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) x[c] = f4{0, 0, 0, 0};
    int64_t m = m0;
    for (; m + 4 <= m1; m += 4) {
      f4 v[4][NC];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float* pp = msg_row(a.src, a.msg_src[m + k], DIN) + 4 * g;
#pragma unroll
        for (int c = 0; c < NC; ++c) v[k][c] = ld4(pp + 16 * c);
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) x[c] = (((x[c] + v[0][c]) + v[1][c]) + v[2][c]) + v[3][c];
    }
    for (; m < m1; ++m) {
      const float* pp = msg_row(a.src, a.msg_src[m], DIN) + 4 * g;
#pragma unroll
      for (int c = 0; c < NC; ++c) x[c] += ld4(pp + 16 * c);
    }
    f4 h[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) h[t] = valid ? ld4(a.h_in + (int64_t)row * H + 16 * t + 4 * g) : f4{0, 0, 0, 0};
    // (LDS form: an opaque lane offset keeps the loop-invariant fragment reads inside the tile loop)
    int wofs = lane;
    if constexpr (LDSW) asm volatile("" : "+v"(wofs));
    f4 acc[3][NT], bhh[NT], hn[NT], cf[kJacCoef][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int u0 = 16 * t + 4 * g;
      acc[0][t] = *reinterpret_cast<const f4*>(sbias + 0 * H + u0);
      acc[1][t] = *reinterpret_cast<const f4*>(sbias + 1 * H + u0);
      acc[2][t] = *reinterpret_cast<const f4*>(sbias + 2 * H + u0);
      bhh[t] = *reinterpret_cast<const f4*>(sbias + 3 * H + u0);
    }
    sweep3<DIN, H>(W4, wofs, x, acc);
    lin_step<H>(U4, wofs, h, acc, bhh, o, hn, cf);
    if (valid) {
#pragma unroll
      for (int t = 0; t < NT; ++t) st4(a.h_out + (int64_t)row * H + 16 * t + 4 * g, hn[t]);
#pragma unroll
      for (int c = 0; c < kJacCoef; ++c)
#pragma unroll
        for (int t = 0; t < NT; ++t) st4(coef + pos * CF + c * H + 16 * t + 4 * g, cf[c][t]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The five-term update for the wave's 16 directions.  acc: gz, gr, gh; adh: ad_h; cf: the
// destination's coefficient rows, the same in every tile row.
template <int H>
__device__ __forceinline__ void jac_update(f4 (&hd)[H / 16], const f4 (&acc)[3][H / 16], const f4 (&adh)[H / 16],
                                           const f4 (&cf)[kJacCoef][H / 16]) {
#pragma unroll
  for (int t = 0; t < H / 16; ++t)
    hd[t] = cf[0][t] * hd[t] + cf[1][t] * acc[0][t] + cf[2][t] * acc[1][t] + cf[3][t] * adh[t] + cf[4][t] * acc[2][t];
}

// ---------------------------------------------------------------------------------------------
// Tangent, ordered update.  One wave per (order position, direction block) for the whole sequence: hd in
// registers, U in LDS once per workgroup (48 KB at H = 64), the grid persistent.
template <int H>
__global__ __launch_bounds__(256) void seq_gru_jac_kernel(SeqJacArgs a) {
  constexpr int NT = H / 16, W3 = 3 * H, CF = kJacCoef * H;
  __shared__ f4 su[3 * NT * NT * 64];
  {
    const f4* s4 = reinterpret_cast<const f4*>(a.Up);
    for (int e = threadIdx.x; e < 3 * NT * NT * 64; e += blockDim.x) su[e] = s4[e];
  }
  const int lane = threadIdx.x & 63;
  const int wave = uniform(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  __syncthreads();
  const int64_t kp = (int64_t)a.n_blk * 16;
  const int64_t tab_row = kp * W3;   // floats between table rows
  const int64_t n_work = a.n_dst * a.n_blk;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < n_work; w += (int64_t)gridDim.x * 4) {
    const int64_t pos = w / a.n_blk;
    const int64_t k = (w - pos * a.n_blk) * 16 + j;   // this lane's direction
    const int row = uniform(a.order[pos]);
    const int L = uniform(a.len[pos]);
    const int s0 = uniform(a.step_ptr[pos]);
    const uint32_t* codes = a.step_code + s0;
    const int64_t hofs = scen_offset(row, k, kp, H) + 4 * g;
    f4 hd[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) hd[t] = ld4(a.hd_in + hofs + 16 * t);
    if (L > 0) {
      const float* tab = a.table_d + k * W3 + 4 * g;
      const float* cfp = a.coef + (int64_t)s0 * CF + 4 * g;
      f4 x[3][NT], cf[kJacCoef][NT];
      {
        const float* p = tab + (int64_t)uniform((int)codes[0]) * tab_row;
#pragma unroll
        for (int G = 0; G < 3; ++G)
#pragma unroll
          for (int i = 0; i < NT; ++i) x[G][i] = ld4(p + G * H + 16 * i);
#pragma unroll
        for (int c = 0; c < kJacCoef; ++c)
#pragma unroll
          for (int i = 0; i < NT; ++i) cf[c][i] = ld4(cfp + c * H + 16 * i);
      }
      for (int t = 0; t < L; ++t) {
        // the next step's block and coefficient rows leave now and land behind this step's MFMAs (the
        // last step asks for its own again: no branch, no read past the sequence)
        const int tn = std::min(t + 1, L - 1);
        f4 xn[3][NT], cn[kJacCoef][NT];
        const float* p = tab + (int64_t)uniform((int)codes[tn]) * tab_row;
        const float* q = cfp + (int64_t)tn * CF;
#pragma unroll
        for (int G = 0; G < 3; ++G)
#pragma unroll
          for (int i = 0; i < NT; ++i) xn[G][i] = ld4(p + G * H + 16 * i);
#pragma unroll
        for (int c = 0; c < kJacCoef; ++c)
#pragma unroll
          for (int i = 0; i < NT; ++i) cn[c][i] = ld4(q + c * H + 16 * i);
        f4 acc[3][NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          acc[0][i] = x[0][i];
          acc[1][i] = x[1][i];
          acc[2][i] = f4{0, 0, 0, 0};
        }
        sweep3<H, H>(su, lane, hd, acc);
        jac_update<H>(hd, acc, x[2], cf);
#pragma unroll
        for (int i = 0; i < NT; ++i) {
#pragma unroll
          for (int G = 0; G < 3; ++G) x[G][i] = xn[G][i];
#pragma unroll
          for (int c = 0; c < kJacCoef; ++c) cf[c][i] = cn[c][i];
        }
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) st4(a.hd_out + hofs + 16 * t, hd[t]);
  }
}

// ---------------------------------------------------------------------------------------------
// Tangent, sum update.  One wave per (order position, direction block); W and U in LDS once per
// workgroup, the grid persistent.  xd = the destination's message blocks added one by one in CSR order,
// four [16][DIN] blocks in flight, at every in-degree; without a message xd = 0.
template <int DIN, int H>
__global__ __launch_bounds__(256) void sum_gru_jac_kernel(SumJacArgs a) {
  constexpr int NC = DIN / 16, NT = H / 16, CF = kJacCoef * H;
  constexpr int WF = 3 * NT * NC * 64, UF = 3 * NT * NT * 64;   // float4 fragments
  __shared__ f4 sW[WF];
  __shared__ f4 sU[UF];
  {
    const f4* gW = reinterpret_cast<const f4*>(a.Wp);
    const f4* gU = reinterpret_cast<const f4*>(a.Up);
    for (int i = threadIdx.x; i < WF; i += blockDim.x) sW[i] = gW[i];
    for (int i = threadIdx.x; i < UF; i += blockDim.x) sU[i] = gU[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = uniform(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const int64_t kp = (int64_t)a.n_blk * 16;
  const int64_t src_row = kp * DIN;   // floats between source rows
  const int64_t n_work = a.n_dst * a.n_blk;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < n_work; w += (int64_t)gridDim.x * 4) {
    const int64_t pos = w / a.n_blk;
    const int64_t k = (w - pos * a.n_blk) * 16 + j;
    const int row = uniform(a.order[pos]);
    const int m0 = uniform(a.msg_ptr[pos]), m1 = uniform(a.msg_ptr[pos + 1]);
    const int64_t sofs = k * DIN + 4 * g;
    auto msg = [&](int m) { return msg_row(a.src_d, (uint32_t)uniform((int)a.msg_src[m]), src_row) + sofs; };
    // the destination's coefficient rows travel with the message blocks
    const float* cfp = a.coef + pos * CF + 4 * g;
    f4 cf[kJacCoef][NT];
#pragma unroll
    for (int c = 0; c < kJacCoef; ++c)
#pragma unroll
      for (int t = 0; t < NT; ++t) cf[c][t] = ld4(cfp + c * H + 16 * t);
    const int64_t hofs = scen_offset(row, k, kp, H) + 4 * g;
    f4 hd[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) hd[t] = ld4(a.hd_in + hofs + 16 * t);
    f4 x[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) x[c] = f4{0, 0, 0, 0};
    int m = m0;
    for (; m + 4 <= m1; m += 4) {
      const float *p0 = msg(m), *p1 = msg(m + 1), *p2 = msg(m + 2), *p3 = msg(m + 3);
      f4 v0[NC], v1[NC], v2[NC], v3[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        v0[c] = ld4(p0 + 16 * c);
        v1[c] = ld4(p1 + 16 * c);
        v2[c] = ld4(p2 + 16 * c);
        v3[c] = ld4(p3 + 16 * c);
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) x[c] = (((x[c] + v0[c]) + v1[c]) + v2[c]) + v3[c];
    }
    for (; m < m1; ++m) {
      const float* p = msg(m);
#pragma unroll
      for (int c = 0; c < NC; ++c) x[c] += ld4(p + 16 * c);
    }
    // (an opaque lane offset keeps the loop-invariant fragment reads inside the work loop)
    int wofs = lane;
    asm volatile("" : "+v"(wofs));
    f4 ad[3][NT], acc[3][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) ad[0][t] = ad[1][t] = ad[2][t] = f4{0, 0, 0, 0};
    sweep3<DIN, H>(sW, wofs, x, ad);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      acc[0][t] = ad[0][t];
      acc[1][t] = ad[1][t];
      acc[2][t] = f4{0, 0, 0, 0};
    }
    sweep3<H, H>(sU, wofs, hd, acc);
    jac_update<H>(hd, acc, ad[2], cf);
#pragma unroll
    for (int t = 0; t < NT; ++t) st4(a.hd_out + hofs + 16 * t, hd[t]);
  }
}

// ---------------------------------------------------------------------------------------------
// h0d = [direction | 0] per (row, direction), one float4 per thread; dir: [n_dir][rows][F] or null.
template <int HQ>
__global__ void init_dir_kernel(f4* __restrict__ state, const float* __restrict__ dir, int64_t rows, int64_t n_dir,
                                int64_t kp, int F) {
  const int64_t total = rows * kp * HQ;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t rk = i / HQ;
    const int c = 4 * (int)(i - rk * HQ);
    const int64_t row = rk / kp, k = rk - row * kp;
    f4 v = f4{0, 0, 0, 0};
    if (dir && c < F && k < n_dir) {
      const float* f = dir + (k * rows + row) * F;
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = c + q < F ? f[c + q] : 0.0f;
    }
    state[i] = v;
  }
}

// The two kinds of tangent table row no source projects, for all Kp directions: the hole row is zeros
// (the tangent of a bias); multi row m is, per direction, the sum of the projected rows listed for it,
// in their order.  One thread per float4 of a row.
__global__ void table_rows_jac_kernel(float* __restrict__ table, int64_t zero_row, int64_t n_multi,
                                      const int32_t* __restrict__ ptr, const uint32_t* __restrict__ rows, int W,
                                      int64_t kp) {
  const int64_t q = W / 4, per_row = kp * q;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1 + n_multi) * per_row;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / per_row, rem = i - m * per_row;
    const int64_t k = rem / q;
    const int c = (int)(rem - k * q) * 4;
    f4 acc = f4{0, 0, 0, 0};
    if (m > 0)
      for (int e = ptr[m - 1]; e < ptr[m]; ++e)
        if ((int64_t)rows[e] != zero_row) acc += ld4(table + scen_offset(rows[e], k, kp, W) + c);
    st4(table + scen_offset(zero_row + m, k, kp, W) + c, acc);
  }
}

__global__ void act_bwd_bcast_kernel(const float* __restrict__ da, const float* __restrict__ y, int64_t rows, int64_t kp,
                                     int width, int act, float* __restrict__ dz) {
  const int64_t per_row = kp * width;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * per_row;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / per_row;
    const int c = (int)((i - r * per_row) % width);
    dz[i] = da[i] * act_grad_out(y[r * width + c], act);
  }
}

__global__ void gather_dpred_kernel(const float* __restrict__ yd, int64_t n_pred, int64_t n_dir, int64_t kp, int units,
                                    float* __restrict__ out) {
  const int64_t total = n_dir * n_pred * units;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t kr = i / units;
    const int u = (int)(i - kr * units);
    const int64_t k = kr / n_pred, r = kr - k * n_pred;
    out[i] = yd[scen_offset(r, k, kp, units) + u];
  }
}

int blocks_for(int64_t threads, int64_t cap) { return (int)std::max<int64_t>(1, std::min<int64_t>((threads + 255) / 256, cap)); }

// resident workgroups per CU x CUs, at most the work (a persistent grid), asked once per kernel
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
hipError_t seq_lin_launch(const SeqGruArgs& p, float* coef, CellOpt o, hipStream_t st) {
  const int64_t work = (p.n_dst + 63) / 64;
  hipLaunchKernelGGL((seq_gru_lin_kernel<H>), dim3(persistent_grid<seq_gru_lin_kernel<H>, 256>(work)), dim3(256), 0, st, p,
                     coef, o);
  return hipGetLastError();
}

template <int H>
hipError_t seq_jac_launch(const SeqJacArgs& a, hipStream_t st) {
  const int64_t work = (a.n_dst * a.n_blk + 3) / 4;
  hipLaunchKernelGGL((seq_gru_jac_kernel<H>), dim3(persistent_grid<seq_gru_jac_kernel<H>, 256>(work)), dim3(256), 0, st, a);
  return hipGetLastError();
}

template <int DIN, int H>
hipError_t sum_jac_launch(const SumJacArgs& a, hipStream_t st) {
  const int64_t work = (a.n_dst * a.n_blk + 3) / 4;
  hipLaunchKernelGGL((sum_gru_jac_kernel<DIN, H>), dim3(persistent_grid<sum_gru_jac_kernel<DIN, H>, 256>(work)), dim3(256), 0,
                     st, a);
  return hipGetLastError();
}

bool cell_ok(CellOpt o) { return act_code_ok(o.act) && act_code_ok(o.ract) && o.reset_after; }

}  // namespace

hipError_t launch_seq_gru_lin(const SeqGruArgs& p, float* coef, int h, CellOpt o, hipStream_t st) {
  if (!jacobian_shape_supported(h, h) || !cell_ok(o)) return hipErrorInvalidValue;
  if (!p.h_in || !p.h_out || !p.table || !p.Up || !p.bias || !coef || p.hs_save) return hipErrorInvalidValue;
  if (p.n_dst == 0) return hipSuccess;
  switch (h) {
    case 16: return seq_lin_launch<16>(p, coef, o, st);
    case 32: return seq_lin_launch<32>(p, coef, o, st);
    default: return seq_lin_launch<64>(p, coef, o, st);
  }
}

hipError_t launch_sum_gru_lin(const SumGruArgs& p, float* coef, int din, int h, CellOpt o, hipStream_t st) {
  if (!jacobian_shape_supported(din, h) || !cell_ok(o)) return hipErrorInvalidValue;
  if (p.msg_w || p.conv_kp || p.x_save || p.sum_save || p.proj_out || !p.h_in || !p.h_out || !coef) return hipErrorInvalidValue;
  if (p.n_dst == 0) return hipSuccess;
  const dim3 grid((unsigned)((p.n_dst + 63) / 64));
#define SL_CASE(D, HH)                                                                                 \
  if (din == D && h == HH) {                                                                           \
    hipLaunchKernelGGL((sum_gru_lin_kernel<D, HH, false, 4>), grid, dim3(256), 0, st, p, coef, o);     \
    return hipGetLastError();                                                                          \
  }
  SL_CASE(32, 32)
  SL_CASE(16, 16)
  SL_CASE(16, 32)
  SL_CASE(32, 16)
#undef SL_CASE
  hipLaunchKernelGGL((sum_gru_lin_kernel<64, 64, true, 4>),
                     dim3(persistent_grid<sum_gru_lin_kernel<64, 64, true, 4>, 256>((p.n_dst + 63) / 64)), dim3(256), 0, st, p,
                     coef, o);
  return hipGetLastError();
}

hipError_t launch_seq_gru_jac(const SeqJacArgs& a, int h, hipStream_t st) {
  if (!jacobian_shape_supported(h, h) || a.n_blk < 1) return hipErrorInvalidValue;
  if (!a.hd_in || !a.hd_out || !a.table_d || !a.coef || !a.Up) return hipErrorInvalidValue;
  if (a.n_dst == 0) return hipSuccess;
  switch (h) {
    case 16: return seq_jac_launch<16>(a, st);
    case 32: return seq_jac_launch<32>(a, st);
    default: return seq_jac_launch<64>(a, st);
  }
}

hipError_t launch_sum_gru_jac(const SumJacArgs& a, int din, int h, hipStream_t st) {
  if (!jacobian_shape_supported(din, h) || a.n_blk < 1) return hipErrorInvalidValue;
  if (!a.hd_in || !a.hd_out || !a.coef || !a.Wp || !a.Up) return hipErrorInvalidValue;
  if (a.n_dst == 0) return hipSuccess;
  if (din == 32 && h == 32) return sum_jac_launch<32, 32>(a, st);
  if (din == 16 && h == 16) return sum_jac_launch<16, 16>(a, st);
  if (din == 16 && h == 32) return sum_jac_launch<16, 32>(a, st);
  if (din == 32 && h == 16) return sum_jac_launch<32, 16>(a, st);
  return sum_jac_launch<64, 64>(a, st);
}

hipError_t launch_init_dir(float* state, const float* dir, int64_t rows, int64_t n_dir, int H, int F, hipStream_t st) {
  if (!jacobian_shape_supported(H, H) || n_dir < 1 || F < 0 || F > H || (reinterpret_cast<uintptr_t>(state) & 15))
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  const int64_t kp = scen_padded(n_dir);
  const int blocks = blocks_for(rows * kp * (H / 4), 16384);
  f4* s4 = reinterpret_cast<f4*>(state);
  if (H == 16) hipLaunchKernelGGL(init_dir_kernel<4>, dim3(blocks), dim3(256), 0, st, s4, dir, rows, n_dir, kp, F);
  else if (H == 32) hipLaunchKernelGGL(init_dir_kernel<8>, dim3(blocks), dim3(256), 0, st, s4, dir, rows, n_dir, kp, F);
  else hipLaunchKernelGGL(init_dir_kernel<16>, dim3(blocks), dim3(256), 0, st, s4, dir, rows, n_dir, kp, F);
  return hipGetLastError();
}

hipError_t launch_table_rows_jac(float* table, int64_t zero_row, int64_t n_multi, const int32_t* ptr,
                                 const uint32_t* rows, int W, int64_t kp, hipStream_t st) {
  if (!table || W % 4 || kp < 16 || kp % 16 || n_multi < 0 || (n_multi && (!ptr || !rows))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(table_rows_jac_kernel, dim3(blocks_for((1 + n_multi) * kp * (W / 4), 4096)), dim3(256), 0, st, table,
                     zero_row, n_multi, ptr, rows, W, kp);
  return hipGetLastError();
}

hipError_t launch_act_bwd_bcast(const float* da, const float* y, int64_t rows, int64_t kp, int width, int act, float* dz,
                                hipStream_t st) {
  if (!da || !y || !dz || !act_code_ok(act) || kp < 1 || width < 1) return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(act_bwd_bcast_kernel, dim3(blocks_for(rows * kp * width, 16384)), dim3(256), 0, st, da, y, rows, kp,
                     width, act, dz);
  return hipGetLastError();
}

hipError_t launch_gather_dpred(const float* yd, int64_t n_pred, int64_t n_dir, int units, float* out, hipStream_t st) {
  if (!yd || !out || n_dir < 1 || units < 1) return hipErrorInvalidValue;
  if (n_pred == 0) return hipSuccess;
  hipLaunchKernelGGL(gather_dpred_kernel, dim3(blocks_for(n_dir * n_pred * units, 8192)), dim3(256), 0, st, yd, n_pred, n_dir,
                     scen_padded(n_dir), units, out);
  return hipGetLastError();
}
