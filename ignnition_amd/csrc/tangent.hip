// tangent.hip — the GRU update on dual numbers, on f32 MFMA (v_mfma_f32_16x16x4_f32): every state row h
// carries a tangent row hd = dh/d(eps) along one input direction, and one launch moves both through an
// ordered or a sum update (forward mode: J.v in one pass the shape of an inference forward, nothing
// saved).  The kernels take the lane layout, argument blocks and tile walk of gru_cell.hip's forward
// kernels, pack_gru's UNSCALED fragments and the combined bias block [4][H], for default cells and
// cells with options alike; what is their own is the dual step below.
//
// The cell (gru_cell.hip's header) and its tangent, derivatives through the outputs (act_grad_out):
//   z = ract(a_z + h.U_z)                zd = ract'(z) (ad_z + hd.U_z)          (r, rd likewise)
//   reset_after:      c = act(a_h + r u),  u = h.U_h + b_hh
//                     cd = act'(c) (ad_h + rd u + r ud),  ud = hd.U_h
//   not reset_after:  c = act(a_h + (r h).U_h)
//                     cd = act'(c) (ad_h + (rd h + r hd).U_h)
//   h' = c + z (h - c)                   hd' = zd (h - c) + z hd + (1 - z) cd
// a = x.W + b is the primal step input and ad = xd.W its tangent (no bias: a constant).
//
// Every contraction by U or W is a DUAL SWEEP: the primal operand and its tangent are two B operands of
// the same A fragments, so each 16-byte fragment read (LDS or L2) feeds eight MFMAs, four into the
// primal accumulator and four into the tangent's, and the tangent costs no fragment traffic.  The
// candidate's second sweep (gru_cell.hip: on h or on r * h) is dual in the same way, on hd or on
// rd h + r hd.  The primal accumulates in cell_sweep's order, so the primal rows are the generalised
// forward's bits, and nothing of the primal reads a tangent value.  Every tangent operation is linear
// in (hd, ad) with primal factors: a zero direction gives zeros and a direction scaled by a power of two
// the scaled tangent, bit for bit.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "device_common.h"
#include "tangent.h"

namespace {

// acc[G - G0][t] += M_G . v and accd[G - G0][t] += M_G . vd for the gates G in [G0, G0 + NG) of a
// float4-grouped fragment array M4 ([3][NT][K / 16][64] x f4); v, vd: K / 16 B-operand tiles each
template <int K, int H, int G0, int NG, int R>
__device__ __forceinline__ void dual_sweep(const f4* M4, int lane, const f4 (&v)[K / 16], const f4 (&vd)[K / 16],
                                           f4 (&acc)[R][H / 16], f4 (&accd)[R][H / 16]) {
  constexpr int NT = H / 16, K4 = K / 16;
  static_assert(NG <= R && G0 + NG <= 3, "gate range");
#pragma unroll
  for (int s4 = 0; s4 < K4; ++s4)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int G = 0; G < NG; ++G) {
        const f4 w = M4[(((G0 + G) * NT + t) * K4 + s4) * 64 + lane];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[G][t] = MFMA(w[q], v[s4][q], acc[G][t]);
#pragma unroll
        for (int q = 0; q < 4; ++q) accd[G][t] = MFMA(w[q], vd[s4][q], accd[G][t]);
      }
}

// One dual step for the wave's 16 rows.  in: a = x.W + b (+ b_rec for z, r), ad = xd.W, bhh = b_hh;
// out: hn = h', hdn = hd'.  a / ad are used up (they end as z, r and zd, rd).
template <int H>
__device__ __forceinline__ void dual_step(const f4* U4, int lane, const f4 (&h)[H / 16], const f4 (&hd)[H / 16],
                                          f4 (&a)[3][H / 16], f4 (&ad)[3][H / 16], const f4 (&bhh)[H / 16], CellOpt o,
                                          f4 (&hn)[H / 16], f4 (&hdn)[H / 16]) {
  constexpr int NT = H / 16;
  dual_sweep<H, H, 0, 2>(U4, lane, h, hd, a, ad);
  f4 bh[NT], bhd[NT], u[1][NT], ud[1][NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z = act_apply(a[0][t][r], o.ract), rr = act_apply(a[1][t][r], o.ract);
      const float zd = act_grad_out(z, o.ract) * ad[0][t][r], rd = act_grad_out(rr, o.ract) * ad[1][t][r];
      a[0][t][r] = z;
      a[1][t][r] = rr;
      ad[0][t][r] = zd;
      ad[1][t][r] = rd;
      // the candidate's second operand and its tangent: h, hd or r h, rd h + r hd (a select per element)
      const float rh = rr * h[t][r], rhd = rd * h[t][r] + rr * hd[t][r];
      bh[t][r] = o.reset_after ? h[t][r] : rh;
      bhd[t][r] = o.reset_after ? hd[t][r] : rhd;
    }
    u[0][t] = bhh[t];
    ud[0][t] = f4{0, 0, 0, 0};
  }
  dual_sweep<H, H, 2, 1>(U4, lane, bh, bhd, u, ud);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z = a[0][t][r], rr = a[1][t][r], zd = ad[0][t][r], rd = ad[1][t][r];
      const float uu = u[0][t][r], uud = ud[0][t][r];
      const float pre = o.reset_after ? a[2][t][r] + rr * uu : a[2][t][r] + uu;
      const float pred = o.reset_after ? ad[2][t][r] + (rd * uu + rr * uud) : ad[2][t][r] + uud;
      const float c = act_apply(pre, o.act);
      const float cd = act_grad_out(c, o.act) * pred;
      const float hc = h[t][r] - c;
      hn[t][r] = c + z * hc;
      hdn[t][r] = zd * hc + z * hd[t][r] + (1.f - z) * cd;
    }
}

// ---------------------------------------------------------------------------------------------
// Ordered / interleave / concat (axis 1) update: one wave per 16 length-sorted destinations, U in LDS
// once per block, h[NT] and hd[NT] in registers over the whole sequence.  Each step loads the primal
// projected row and the tangent projected row by the same step code.  A lane past its sequence passes
// h and hd through; invalid lanes of the last tile store nothing.
template <int H>
__global__ __launch_bounds__(256) void seq_gru_tangent_kernel(SeqTangentArgs a, CellOpt o) {
  constexpr int NT = H / 16, K4 = H / 16;
  __shared__ float sbhh[H];
  __shared__ f4 su[3 * NT * K4 * 64];
  for (int i = threadIdx.x; i < H; i += blockDim.x) sbhh[i] = a.p.bias[3 * H + i];
  {
    const f4* s4 = reinterpret_cast<const f4*>(a.p.Up);
    for (int e = threadIdx.x; e < 3 * NT * K4 * 64; e += blockDim.x) su[e] = s4[e];
  }
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const float* tab = a.p.table + 4 * g;
  const float* tabd = a.table_d + 4 * g;
  __syncthreads();
  const int64_t n_tiles = (a.p.n_dst + 15) / 16;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t pos = tile * 16 + j;
    const bool valid = pos < a.p.n_dst;
    const int row = valid ? a.p.order[pos] : 0;
    const int L = valid ? a.p.len[pos] : 0;
    const uint32_t* codes = a.p.step_code + (valid ? a.p.step_ptr[pos] : 0);
    f4 h[NT], hd[NT], bhh[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      h[t] = valid ? ld4(a.p.h_in + (int64_t)row * H + 16 * t + 4 * g) : f4{0, 0, 0, 0};
      hd[t] = valid ? ld4(a.hd_in + (int64_t)row * H + 16 * t + 4 * g) : f4{0, 0, 0, 0};
      bhh[t] = *reinterpret_cast<const f4*>(sbhh + 16 * t + 4 * g);
    }
    int Lmax = L;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) Lmax = max(Lmax, __shfl_xor(Lmax, s));
    uint32_t code = codes[0];
    for (int t = 0; t < Lmax; ++t) {
      f4 x[3][NT], xd[3][NT], hn[NT], hdn[NT];
      const int64_t ofs = (int64_t)code * (3 * H);
#pragma unroll
      for (int G = 0; G < 3; ++G)
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          x[G][i] = ld4(tab + ofs + G * H + 16 * i);
          xd[G][i] = ld4(tabd + ofs + G * H + 16 * i);
        }
      const uint32_t next = codes[t + 1];   // (step_code is padded past every sequence)
      dual_step<H>(su, lane, h, hd, x, xd, bhh, o, hn, hdn);
      const bool on = t < L;
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          h[i][r] = on ? hn[i][r] : h[i][r];
          hd[i][r] = on ? hdn[i][r] : hd[i][r];
        }
      code = next;
    }
    if (valid) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        st4(a.p.h_out + (int64_t)row * H + 16 * t + 4 * g, h[t]);
        st4(a.hd_out + (int64_t)row * H + 16 * t + 4 * g, hd[t]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Sum update: one tile per wave.  The lane walk reads each message code once and adds the primal row
// and the tangent row it names, the primal in sum_gru_cell_kernel's order (four rows in flight, added
// in CSR order); x.W and xd.W share each W fragment read, then the dual step.  A destination without
// messages has x = xd = 0: its hd' still carries z hd, the state's own term.  LDSW (64 / 64): W and U
// staged in LDS once per block, the block persistent over the tiles.
__device__ __forceinline__ int64_t code_ofs(uint32_t code, int din) { return (int64_t)(code & IGN_ROW_MASK) * din; }
__device__ __forceinline__ const float* slot_base(const SrcBases& sb, uint32_t code) {
  const uint32_t slot = code >> IGN_SLOT_SHIFT;
  const float* b = sb.base[0];
  if (slot == 1) b = sb.base[1];
  if (slot == 2) b = sb.base[2];
  if (slot == 3) b = sb.base[3];
  return b;
}

template <int DIN, int H, bool LDSW, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void sum_gru_tangent_kernel(SumTangentArgs a, CellOpt o) {
  constexpr int NC = DIN / 16, NT = H / 16;
  constexpr int WF = 3 * NT * NC * 64, UF = 3 * NT * NT * 64;   // float4 fragments
  __shared__ f4 sW[LDSW ? WF : 1];
  __shared__ f4 sU[LDSW ? UF : 1];
  __shared__ float sbias[4 * H];
  for (int i = threadIdx.x; i < 4 * H; i += 64 * WAVES) sbias[i] = a.p.bias[i];
  if constexpr (LDSW) {
    const f4* gW = reinterpret_cast<const f4*>(a.p.Wp);
    const f4* gU = reinterpret_cast<const f4*>(a.p.Up);
    for (int i = threadIdx.x; i < WF; i += 64 * WAVES) sW[i] = gW[i];
    for (int i = threadIdx.x; i < UF; i += 64 * WAVES) sU[i] = gU[i];
  }
  __syncthreads();
  const f4* W4 = LDSW ? sW : reinterpret_cast<const f4*>(a.p.Wp);
  const f4* U4 = LDSW ? sU : reinterpret_cast<const f4*>(a.p.Up);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int64_t n_tiles = (a.p.n_dst + 15) / 16;
  for (int64_t tile = (int64_t)blockIdx.x * WAVES + wave; tile < n_tiles; tile += (int64_t)gridDim.x * WAVES) {
    const int64_t pos = tile * 16 + j;
    const bool valid = pos < a.p.n_dst;
    const int row = valid ? a.p.order[pos] : 0;
    const int64_t m0 = valid ? a.p.msg_ptr[pos] : 0;
    const int64_t m1 = valid ? a.p.msg_ptr[pos + 1] : 0;
    f4 x[NC], xd[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) x[c] = xd[c] = f4{0, 0, 0, 0};
    int64_t m = m0;
    for (; m + 4 <= m1; m += 4) {
      f4 v[4][NC], w[4][NC];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t code = a.p.msg_src[m + k];
        const int64_t ofs = code_ofs(code, DIN) + 4 * g;
        const float* pp = slot_base(a.p.src, code) + ofs;
        const float* pd = slot_base(a.src_d, code) + ofs;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          v[k][c] = ld4(pp + 16 * c);
          w[k][c] = ld4(pd + 16 * c);
        }
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        x[c] = (((x[c] + v[0][c]) + v[1][c]) + v[2][c]) + v[3][c];
        xd[c] = (((xd[c] + w[0][c]) + w[1][c]) + w[2][c]) + w[3][c];
      }
    }
    for (; m < m1; ++m) {
      const uint32_t code = a.p.msg_src[m];
      const int64_t ofs = code_ofs(code, DIN) + 4 * g;
      const float* pp = slot_base(a.p.src, code) + ofs;
      const float* pd = slot_base(a.src_d, code) + ofs;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        x[c] += ld4(pp + 16 * c);
        xd[c] += ld4(pd + 16 * c);
      }
    }
    f4 h[NT], hd[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      h[t] = valid ? ld4(a.p.h_in + (int64_t)row * H + 16 * t + 4 * g) : f4{0, 0, 0, 0};
      hd[t] = valid ? ld4(a.hd_in + (int64_t)row * H + 16 * t + 4 * g) : f4{0, 0, 0, 0};
    }
    // (LDS form: an opaque lane offset keeps the loop-invariant fragment reads inside the tile loop)
    int wofs = lane;
    if constexpr (LDSW) asm volatile("" : "+v"(wofs));
    f4 acc[3][NT], accd[3][NT], bhh[NT], hn[NT], hdn[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int u0 = 16 * t + 4 * g;
      acc[0][t] = *reinterpret_cast<const f4*>(sbias + 0 * H + u0);
      acc[1][t] = *reinterpret_cast<const f4*>(sbias + 1 * H + u0);
      acc[2][t] = *reinterpret_cast<const f4*>(sbias + 2 * H + u0);
      bhh[t] = *reinterpret_cast<const f4*>(sbias + 3 * H + u0);
      accd[0][t] = accd[1][t] = accd[2][t] = f4{0, 0, 0, 0};
    }
    dual_sweep<DIN, H, 0, 3>(W4, wofs, x, xd, acc, accd);
    dual_step<H>(U4, wofs, h, hd, acc, accd, bhh, o, hn, hdn);
    if (valid) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        st4(a.p.h_out + (int64_t)row * H + 16 * t + 4 * g, hn[t]);
        st4(a.hd_out + (int64_t)row * H + 16 * t + 4 * g, hdn[t]);
      }
    }
  }
}

int grid_for(int64_t n, int per_block) { return (int)((n + per_block - 1) / per_block); }

// resident blocks per CU x CUs, at most the work (a persistent grid), asked once per kernel
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
hipError_t seq_tangent_launch(const SeqTangentArgs& a, CellOpt o, hipStream_t st) {
  const int64_t work = grid_for(a.p.n_dst, 64);
  hipLaunchKernelGGL((seq_gru_tangent_kernel<H>), dim3(persistent_grid<seq_gru_tangent_kernel<H>, 256>(work)), dim3(256), 0,
                     st, a, o);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_seq_gru_tangent(const SeqTangentArgs& a, int h, CellOpt o, hipStream_t st) {
  if (!gru_cell_seq_supported(h) || !act_code_ok(o.act) || !act_code_ok(o.ract)) return hipErrorInvalidValue;
  if (!a.p.h_in || !a.p.h_out || !a.hd_in || !a.hd_out || !a.p.table || !a.table_d || a.p.hs_save)
    return hipErrorInvalidValue;
  if (a.p.n_dst == 0) return hipSuccess;
  switch (h) {
    case 16: return seq_tangent_launch<16>(a, o, st);
    case 32: return seq_tangent_launch<32>(a, o, st);
    case 64: return seq_tangent_launch<64>(a, o, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_sum_gru_tangent(const SumTangentArgs& a, int din, int h, CellOpt o, hipStream_t st) {
  if (!gru_cell_sum_supported(din, h, 0) || !act_code_ok(o.act) || !act_code_ok(o.ract)) return hipErrorInvalidValue;
  if (a.p.msg_w || a.p.conv_kp || a.p.x_save || a.p.sum_save || a.p.proj_out || !a.hd_in || !a.hd_out)
    return hipErrorInvalidValue;
  if (a.p.n_dst == 0) return hipSuccess;
  const dim3 grid(grid_for(a.p.n_dst, 64));
#define ST_CASE(D, HH)                                                                                   \
  if (din == D && h == HH) {                                                                             \
    hipLaunchKernelGGL((sum_gru_tangent_kernel<D, HH, false, 4>), grid, dim3(256), 0, st, a, o);         \
    return hipGetLastError();                                                                            \
  }
  ST_CASE(32, 32)
  ST_CASE(16, 16)
  ST_CASE(16, 32)
  ST_CASE(32, 16)
#undef ST_CASE
  // 64 / 64: four waves per block, one per SIMD, so the dual step's registers fit without spilling
  constexpr int WV = 4;
  const int64_t work = (a.p.n_dst + 16 * WV - 1) / (16 * WV);
  hipLaunchKernelGGL((sum_gru_tangent_kernel<64, 64, true, WV>),
                     dim3(persistent_grid<sum_gru_tangent_kernel<64, 64, true, WV>, 64 * WV>(work)), dim3(64 * WV), 0, st, a,
                     o);
  return hipGetLastError();
}
