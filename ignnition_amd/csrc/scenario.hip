// scenario.hip — the GRU updates of ign_forward_scenarios on f32 MFMA (v_mfma_f32_16x16x4_f32): S
// feature sets on one topology, the 16 rows of a tile on the SCENARIO axis.
//
// Layout: Sp = S rounded up to 16; a state array is [row][Sp][H], a projected table
// [table row][Sp][3H].  Flat row r * Sp + s makes the 16 scenarios of block k of row r the contiguous
// [16][width] block at (r * Sp + 16 k) * width, and lets the row kernels of the batched forward
// (project_kernel, the Dense forward) run unchanged on rows * Sp rows.
//
// What that buys the two updates.  A wave owns one (destination, scenario block) and every lane of
// it is the same destination:
//   * ordered: one length, so no mask, no padding step and no wave-wide max; one step code per step,
//     read once per wave through the scalar unit; the step's projected rows are one [16][3H] block
//     fetched with 16-byte loads, and the next step's block is in flight during this step's MFMAs;
//   * sum: the CSR range and every message code are read once per wave; a message is one [16][DIN]
//     block; four blocks are in flight and are added in the destination's CSR order, whatever the
//     in-degree -- a scenario's bits depend on the destination's CSR range alone, not on S, not on
//     its place in the block (an MFMA column depends on its own B column only).
// Work item w = position * n_blk + block walks the batch's order arrays (longest sequence / highest
// in-degree first), so the waves of a workgroup take the scenario blocks of one destination, or of
// neighbouring destinations when Sp = 16.  The weight fragments (pack_gru's unscaled form) are staged
// in LDS once per workgroup and the grid is persistent.
//
// The cell is the default one (Keras GRUCell v2, reset_after):
//   z = s(a_z + h.U_z) ; r = s(a_r + h.U_r) ; c = tanh(a_h + r (h.U_h + b_hh)) ; h' = c + z (h - c)
// with a = x.W + b the step input (a table row, or formed here from the summed messages).  One sweep
// over the U fragments feeds all three gates: each 16-byte LDS read is four MFMAs.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "device_common.h"
#include "scenario.h"

namespace {

// acc[G][t] += M_G . v for the three gates of a float4-grouped fragment array ([3][NT][K / 16][64] x f4)
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

// One step for the wave's 16 scenarios.  acc: a_z, a_r, b_hh on entry (used up); ah: a_h; h in, h' out.
// LIN (ign_backward_scenarios): the step's linearisation too, the rows (z, P, R, Q, S) of
//   hd' = z hd + P (ad_z + hd.U_z) + R (ad_r + hd.U_r) + Q ad_h + S (hd.U_h)
// of THIS lane's scenario, into the tile's five [16][H] blocks at cf (the lane's row and unit group of
// block 0): a lane's four accumulator registers are four consecutive units, so every store is 16 bytes.
// The primal's own expressions are the ones above the if: h' keeps forward_scenarios' bits.
template <int H, bool LIN>
__device__ __forceinline__ void scen_step(const f4* U4, int lane, f4 (&h)[H / 16], f4 (&acc)[3][H / 16],
                                          const f4 (&ah)[H / 16], float* cf) {
  constexpr int NT = H / 16;
  sweep3<H, H>(U4, lane, h, acc);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f4 k[kScenCoef];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z = sigmoidf_(acc[0][t][r]);
      const float rr = sigmoidf_(acc[1][t][r]);
      const float c = tanhf_(ah[t][r] + rr * acc[2][t][r]);
      const float h0 = h[t][r];
      h[t][r] = c + z * (h[t][r] - c);
      if constexpr (LIN) {
        const float Q = (1.f - z) * (1.f - c * c);
        k[0][r] = z;
        k[1][r] = (h0 - c) * (z * (1.f - z));
        k[2][r] = Q * (rr * (1.f - rr)) * acc[2][t][r];
        k[3][r] = Q;
        k[4][r] = Q * rr;
      }
    }
    if constexpr (LIN) {
#pragma unroll
      for (int q = 0; q < kScenCoef; ++q) st4(cf + q * 16 * H + 16 * t, k[q]);
    }
  }
}

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ---------------------------------------------------------------------------------------------
// h0 = [features | 0] per (row, scenario), one float4 per thread.  scen: [n_scen][rows][F]; shared:
// [rows][F], the batch's values for every scenario.  A padding scenario copies the last real one: its
// rows are finite and are never returned.
template <int HQ>
__global__ void init_state_scen_kernel(f4* __restrict__ state, const float* __restrict__ scen,
                                       const float* __restrict__ shared, int64_t rows, int64_t n_scen, int64_t sp, int F) {
  const int64_t total = rows * sp * HQ;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t rs = i / HQ;
    const int c = 4 * (int)(i - rs * HQ);
    f4 v = f4{0, 0, 0, 0};
    if (c < F && (scen || shared)) {
      const int64_t row = rs / sp;
      const int64_t s = std::min<int64_t>(rs - row * sp, n_scen - 1);
      const float* f = scen ? scen + (s * rows + row) * F : shared + row * F;
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = c + q < F ? f[c + q] : 0.0f;
    }
    state[i] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// The two kinds of table row no source projects, for all Sp scenarios: the hole row is the bias alone;
// multi row k is, per scenario, the sum of the projected rows listed for it, the bias carried once
// (multi_sum_kernel's arithmetic and order).  One thread per float4 of a row.
__global__ void table_rows_scen_kernel(float* __restrict__ table, int64_t zero_row, int64_t n_multi,
                                       const int32_t* __restrict__ ptr, const uint32_t* __restrict__ rows,
                                       const float* __restrict__ bias, int W, int64_t sp) {
  const int64_t q = W / 4, per_row = sp * q;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1 + n_multi) * per_row;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = i / per_row, rem = i - k * per_row;
    const int64_t s = rem / q;
    const int c = (int)(rem - s * q) * 4;
    const f4 b = ld4(bias + c);
    f4 acc = b;
    if (k > 0) {
      const int m0 = ptr[k - 1], m1 = ptr[k];
      acc = f4{0, 0, 0, 0};
      for (int m = m0; m < m1; ++m)
        acc += (int64_t)rows[m] == zero_row ? b : ld4(table + scen_offset(rows[m], s, sp, W) + c);
      acc -= (float)(m1 - m0 - 1) * b;
    }
    st4(table + scen_offset(zero_row + k, s, sp, W) + c, acc);
  }
}

// ---------------------------------------------------------------------------------------------
// Ordered update.  One wave per (order position, scenario block) for the whole sequence: h in
// registers, U in LDS once per workgroup (48 KB at H = 64), the bias b_hh in registers.
// LIN: every real step's coefficient tile goes to coef [step][block][5][16][H], step counted over the
// batch's step_code array (step_ptr[pos] + t).
// KEEP (ign_backward_scenarios_params): the state in front of every real step too, one
// [16][H] tile per (step, block) at keep: 1 row-major, so the tiles are the flat rows step * Sp + s of a
// row contraction; 2 transposed [H][16], the 16-byte A operand loads of the adjoint's fused h_prev^T . ubar.
template <int H, bool LIN, int KEEP>
__global__ __launch_bounds__(256) void seq_gru_scen_kernel(SeqScenArgs a, float* __restrict__ coef, float* __restrict__ keep) {
  constexpr int NT = H / 16, W3 = 3 * H;
  __shared__ f4 su[3 * NT * NT * 64];
  {
    const f4* s4 = reinterpret_cast<const f4*>(a.Up);
    for (int e = threadIdx.x; e < 3 * NT * NT * 64; e += blockDim.x) su[e] = s4[e];
  }
  const int lane = threadIdx.x & 63;
  const int wave = uniform(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  f4 bhh[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) bhh[t] = ld4(a.bias + 3 * H + 16 * t + 4 * g);
  __syncthreads();
  const int64_t sp = (int64_t)a.n_blk * 16;
  const int64_t tab_row = sp * W3;   // floats between table rows
  const int64_t n_work = a.n_dst * a.n_blk;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < n_work; w += (int64_t)gridDim.x * 4) {
    const int64_t pos = w / a.n_blk;
    const int64_t s = (w - pos * a.n_blk) * 16 + j;   // this lane's scenario
    const int row = uniform(a.order[pos]);
    const int L = uniform(a.len[pos]);
    const int s0 = uniform(a.step_ptr[pos]);
    const uint32_t* codes = a.step_code + s0;
    const int64_t hofs = scen_offset(row, s, sp, H) + 4 * g;
    f4 h[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) h[t] = ld4(a.h_in + hofs + 16 * t);
    if (L > 0) {
      const float* tab = a.table + s * W3 + 4 * g;
      f4 x[3][NT];
      {
        const float* p = tab + (int64_t)uniform((int)codes[0]) * tab_row;
#pragma unroll
        for (int G = 0; G < 3; ++G)
#pragma unroll
          for (int i = 0; i < NT; ++i) x[G][i] = ld4(p + G * H + 16 * i);
      }
      for (int t = 0; t < L; ++t) {
        // the next step's block leaves now and lands behind this step's MFMAs (the last step asks for
        // its own block again: no branch, no read past the sequence)
        f4 xn[3][NT];
        const float* p = tab + (int64_t)uniform((int)codes[std::min(t + 1, L - 1)]) * tab_row;
#pragma unroll
        for (int G = 0; G < 3; ++G)
#pragma unroll
          for (int i = 0; i < NT; ++i) xn[G][i] = ld4(p + G * H + 16 * i);
        f4 acc[3][NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          acc[0][i] = x[0][i];
          acc[1][i] = x[1][i];
          acc[2][i] = bhh[i];
        }
        float* cf = nullptr;
        if constexpr (LIN) cf = coef + (((int64_t)(s0 + t) * a.n_blk + (w - pos * a.n_blk)) * kScenCoef * 16 + j) * H + 4 * g;
        if constexpr (KEEP != 0) {
          float* hp = keep + ((int64_t)(s0 + t) * a.n_blk + (w - pos * a.n_blk)) * 16 * H;
#pragma unroll
          for (int i = 0; i < NT; ++i) {
            if constexpr (KEEP == 1) st4(hp + j * H + 16 * i + 4 * g, h[i]);
            else
#pragma unroll
              for (int r = 0; r < 4; ++r) hp[(16 * i + 4 * g + r) * 16 + j] = h[i][r];
          }
        }
        scen_step<H, LIN>(su, lane, h, acc, x[2], cf);
#pragma unroll
        for (int G = 0; G < 3; ++G)
#pragma unroll
          for (int i = 0; i < NT; ++i) x[G][i] = xn[G][i];
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) st4(a.h_out + hofs + 16 * t, h[t]);
  }
}

// ---------------------------------------------------------------------------------------------
// Sum update.  One wave per (order position, scenario block); W and U in LDS once per workgroup, the
// grid persistent.  x = the destination's messages added one by one in CSR order, four [16][DIN]
// blocks in flight; without a message x = 0.
// LIN: the destination's coefficient tile goes to coef [order position][block][5][16][H].
// KEEP: the summed messages x too, [order position][Sp][DIN] at keep.
template <int DIN, int H, bool LIN, bool KEEP>
__global__ __launch_bounds__(256) void sum_gru_scen_kernel(SumScenArgs a, float* __restrict__ coef, float* __restrict__ keep) {
  constexpr int NC = DIN / 16, NT = H / 16;
  constexpr int WF = 3 * NT * NC * 64, UF = 3 * NT * NT * 64;   // float4 fragments
  __shared__ f4 sW[WF];
  __shared__ f4 sU[UF];
  __shared__ float sbias[4 * H];
  for (int i = threadIdx.x; i < 4 * H; i += blockDim.x) sbias[i] = a.bias[i];
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
  const int64_t sp = (int64_t)a.n_blk * 16;
  const int64_t src_row = sp * DIN;   // floats between source rows
  const int64_t n_work = a.n_dst * a.n_blk;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wave; w < n_work; w += (int64_t)gridDim.x * 4) {
    const int64_t pos = w / a.n_blk;
    const int64_t s = (w - pos * a.n_blk) * 16 + j;
    const int row = uniform(a.order[pos]);
    const int m0 = uniform(a.msg_ptr[pos]), m1 = uniform(a.msg_ptr[pos + 1]);
    const int64_t sofs = s * DIN + 4 * g;
    auto msg = [&](int m) -> const float* {
      const uint32_t code = (uint32_t)uniform((int)a.msg_src[m]);
      const uint32_t slot = code >> IGN_SLOT_SHIFT;
      const float* b = a.src.base[0];
      if (slot == 1) b = a.src.base[1];
      if (slot == 2) b = a.src.base[2];
      if (slot == 3) b = a.src.base[3];
      return b + (int64_t)(code & IGN_ROW_MASK) * src_row + sofs;
    };
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
    if constexpr (KEEP) {
#pragma unroll
      for (int c = 0; c < NC; ++c) st4(keep + (w * 16 + j) * DIN + 16 * c + 4 * g, x[c]);
    }
    const int64_t hofs = scen_offset(row, s, sp, H) + 4 * g;
    f4 h[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) h[t] = ld4(a.h_in + hofs + 16 * t);
    // (an opaque lane offset keeps the loop-invariant fragment reads inside the work loop)
    int wofs = lane;
    asm volatile("" : "+v"(wofs));
    f4 ax[3][NT], acc[3][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int G = 0; G < 3; ++G) ax[G][t] = *reinterpret_cast<const f4*>(sbias + G * H + 16 * t + 4 * g);
    sweep3<DIN, H>(sW, wofs, x, ax);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      acc[0][t] = ax[0][t];
      acc[1][t] = ax[1][t];
      acc[2][t] = *reinterpret_cast<const f4*>(sbias + 3 * H + 16 * t + 4 * g);
    }
    float* cf = nullptr;
    if constexpr (LIN) cf = coef + ((w * kScenCoef * 16) + j) * H + 4 * g;
    scen_step<H, LIN>(sU, wofs, h, acc, ax[2], cf);
#pragma unroll
    for (int t = 0; t < NT; ++t) st4(a.h_out + hofs + 16 * t, h[t]);
  }
}

// ---------------------------------------------------------------------------------------------
__global__ void gather_pred_scen_kernel(const float* __restrict__ y, int64_t n_pred, int64_t n_scen, int64_t sp, int units,
                                        float* __restrict__ out) {
  const int64_t total = n_scen * n_pred * units;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t sr = i / units;
    const int u = (int)(i - sr * units);
    const int64_t s = sr / n_pred, r = sr - s * n_pred;
    out[i] = y[scen_offset(r, s, sp, units) + u];
  }
}

int blocks_for(int64_t threads, int64_t cap) { return (int)std::max<int64_t>(1, std::min<int64_t>((threads + 255) / 256, cap)); }

// resident workgroups per CU x CUs, at most the work (a persistent grid), asked once per kernel
template <auto KERNEL>
int persistent_grid(int64_t n_work) {
  static const int64_t resident = [] {
    int dev = 0, cus = 0, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus <= 0) cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, KERNEL, 256, 0) != hipSuccess || per_cu <= 0) per_cu = 1;
    return (int64_t)per_cu * cus;
  }();
  return (int)std::max<int64_t>(1, std::min<int64_t>(resident, (n_work + 3) / 4));
}

template <auto KERNEL, class Args>
hipError_t scen_launch(const Args& a, int64_t n_work, float* coef, float* keep, hipStream_t st) {
  hipLaunchKernelGGL(KERNEL, dim3(persistent_grid<KERNEL>(n_work)), dim3(256), 0, st, a, coef, keep);
  return hipGetLastError();
}

template <int H>
hipError_t seq_scen_launch(const SeqScenArgs& a, float* coef, float* keep, bool keep_t, hipStream_t st) {
  const int64_t n_work = a.n_dst * a.n_blk;
  if (keep && keep_t) return scen_launch<seq_gru_scen_kernel<H, true, 2>>(a, n_work, coef, keep, st);
  if (keep) return scen_launch<seq_gru_scen_kernel<H, true, 1>>(a, n_work, coef, keep, st);
  if (coef) return scen_launch<seq_gru_scen_kernel<H, true, 0>>(a, n_work, coef, keep, st);
  return scen_launch<seq_gru_scen_kernel<H, false, 0>>(a, n_work, coef, keep, st);
}

template <int DIN, int H>
hipError_t sum_scen_launch(const SumScenArgs& a, float* coef, float* keep, hipStream_t st) {
  const int64_t n_work = a.n_dst * a.n_blk;
  if (keep) return scen_launch<sum_gru_scen_kernel<DIN, H, true, true>>(a, n_work, coef, keep, st);
  if (coef) return scen_launch<sum_gru_scen_kernel<DIN, H, true, false>>(a, n_work, coef, keep, st);
  return scen_launch<sum_gru_scen_kernel<DIN, H, false, false>>(a, n_work, coef, keep, st);
}

}  // namespace

hipError_t launch_init_state_scen(float* state, const float* scen, const float* shared, int64_t rows, int64_t n_scen,
                                  int H, int F, hipStream_t st) {
  if (!scen_seq_supported(H) || n_scen < 1 || F < 0 || F > H || (reinterpret_cast<uintptr_t>(state) & 15))
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  const int64_t sp = scen_padded(n_scen);
  const int blocks = blocks_for(rows * sp * (H / 4), 16384);
  f4* s4 = reinterpret_cast<f4*>(state);
  if (H == 16) hipLaunchKernelGGL(init_state_scen_kernel<4>, dim3(blocks), dim3(256), 0, st, s4, scen, shared, rows, n_scen, sp, F);
  else if (H == 32) hipLaunchKernelGGL(init_state_scen_kernel<8>, dim3(blocks), dim3(256), 0, st, s4, scen, shared, rows, n_scen, sp, F);
  else hipLaunchKernelGGL(init_state_scen_kernel<16>, dim3(blocks), dim3(256), 0, st, s4, scen, shared, rows, n_scen, sp, F);
  return hipGetLastError();
}

hipError_t launch_table_rows_scen(float* table, int64_t zero_row, int64_t n_multi, const int32_t* ptr,
                                  const uint32_t* rows, const float* bias, int W, int64_t sp, hipStream_t st) {
  if (!table || !bias || W % 4 || sp < 16 || sp % 16 || n_multi < 0 || (n_multi && (!ptr || !rows))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(table_rows_scen_kernel, dim3(blocks_for((1 + n_multi) * sp * (W / 4), 4096)), dim3(256), 0, st, table,
                     zero_row, n_multi, ptr, rows, bias, W, sp);
  return hipGetLastError();
}

hipError_t launch_seq_gru_scen(const SeqScenArgs& a, int h, hipStream_t st, float* coef, float* keep, bool keep_t) {
  if (!scen_seq_supported(h) || a.n_blk < 1 || ((reinterpret_cast<uintptr_t>(coef) | reinterpret_cast<uintptr_t>(keep)) & 15) ||
      (keep && !coef))
    return hipErrorInvalidValue;
  if (!a.h_in || !a.h_out || !a.table || !a.Up || !a.bias) return hipErrorInvalidValue;
  if (a.n_dst == 0) return hipSuccess;
  switch (h) {
    case 16: return seq_scen_launch<16>(a, coef, keep, keep_t, st);
    case 32: return seq_scen_launch<32>(a, coef, keep, keep_t, st);
    case 64: return seq_scen_launch<64>(a, coef, keep, keep_t, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_sum_gru_scen(const SumScenArgs& a, int din, int h, hipStream_t st, float* coef, float* keep) {
  if (!scen_sum_supported(din, h) || a.n_blk < 1 || ((reinterpret_cast<uintptr_t>(coef) | reinterpret_cast<uintptr_t>(keep)) & 15) ||
      (keep && !coef))
    return hipErrorInvalidValue;
  if (!a.h_in || !a.h_out || !a.Wp || !a.Up || !a.bias) return hipErrorInvalidValue;
  if (a.n_dst == 0) return hipSuccess;
  if (din == 32 && h == 32) return sum_scen_launch<32, 32>(a, coef, keep, st);
  if (din == 16 && h == 16) return sum_scen_launch<16, 16>(a, coef, keep, st);
  if (din == 16 && h == 32) return sum_scen_launch<16, 32>(a, coef, keep, st);
  if (din == 32 && h == 16) return sum_scen_launch<32, 16>(a, coef, keep, st);
  return sum_scen_launch<64, 64>(a, coef, keep, st);
}

hipError_t launch_gather_pred_scen(const float* y, int64_t n_pred, int64_t n_scen, int units, float* out, hipStream_t st) {
  if (!y || !out || n_scen < 1 || units < 1) return hipErrorInvalidValue;
  if (n_pred == 0) return hipSuccess;
  hipLaunchKernelGGL(gather_pred_scen_kernel, dim3(blocks_for(n_scen * n_pred * units, 8192)), dim3(256), 0, st, y, n_pred,
                     n_scen, scen_padded(n_scen), units, out);
  return hipGetLastError();
}
