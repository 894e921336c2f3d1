// kernels_bf.hip — the split-bf16 kernels: fp32 contractions formed from exact
// 3-piece bf16 splits on v_mfma_f32_16x16x32_bf16.  A separate translation unit so that it can be
// compiled with -mllvm -amdgpu-mfma-vgpr-form (accumulators in VGPRs: the gate / activation VALU
// reads them without v_accvgpr_read), which the f32-MFMA kernels of kernels.hip measured slower with.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include "kernels.h"

#include "device_common.h"

namespace {

int64_t grid_for(int64_t n, int64_t per_block) { return (n + per_block - 1) / per_block; }

// resident blocks per CU (occupancy API) x CUs, at most the work
template <typename K>
int persistent_grid(K kernel, int64_t n_blocks_of_work, int block = 256) {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus <= 0) cus = 256;
  }
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) != hipSuccess || per_cu <= 0) per_cu = 1;
  // IGN_PERSIST_CAP (probe): at most this many resident blocks per CU, leaving the other wave
  // slots to a kernel on another stream
  static const int cap = getenv("IGN_PERSIST_CAP") ? atoi(getenv("IGN_PERSIST_CAP")) : 0;
  if (cap > 0) per_cu = std::min(per_cu, cap);
  const int64_t g = (int64_t)per_cu * cus;
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, n_blocks_of_work));
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Variants 4 / 5 of the ordered update: seq_gru2's recurrence with h.U on the bf16 matrix path,
// fp32-exact (device_common.h, split-bf16).  U (pre-scaled as for pack_gru) is split once into
// three bf16 pieces (pack_u_bf16); every step splits the wave's hidden state the same way and
// forms the 9 (variant 5) or 6 (variant 4) piece products per gate tile with
// v_mfma_f32_16x16x32_bf16, accumulated in fp32 from the bias.
// Fragment layout of 16x16x32 (lane l, element j): A[m = l&15][k = 8(l>>4) + j],
// B[k][n = l&15].  The k order is permuted, kperm(s, g, j) = 16 (2s + (j>>2)) + 4g + (j&3), so
// the B fragment of k-step s is exactly registers (2s .. 2s+1) of the lane's accumulator tiles:
// the state still never leaves the lane.
// K: rows of the matrix (H for the recurrent kernel U, DIN for the input kernel W of the sum update)
__global__ void pack_u_bf16_kernel(const float* __restrict__ U, uint16_t* __restrict__ out, int K, int H) {
  const int NT = H / 16, KS = K / 32;
  const int64_t total = 9LL * NT * KS * 64 * 8;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(e & 7), lane = (int)((e >> 3) & 63);
    int64_t f = e >> 9;                       // ((piece * 3 + gate) * NT + tile) * KS + s
    const int s = (int)(f % KS); f /= KS;
    const int i = (int)(f % NT); f /= NT;
    const int G = (int)(f % 3);
    const int piece = (int)(f / 3);
    const int k = 16 * (2 * s + (j >> 2)) + 4 * (lane >> 4) + (j & 3);
    const int col = G * H + 16 * i + (lane & 15);
    const float sc = G == 2 ? IGN_2LOG2E : IGN_NLOG2E;   // as pack_gru
    float p[3];
    split3(sc * U[(int64_t)k * 3 * H + col], p[0], p[1], p[2]);
    out[e] = (uint16_t)(__float_as_uint(p[piece]) >> 16);
  }
}

template <int H, bool SAVE, int PASSES>
__global__ __launch_bounds__(256) void seq_gru_bf_kernel(SeqGruArgs a) {
  constexpr int NT = H / 16, KS = H / 32;
  constexpr int NF = 9 * NT * KS;            // fragments: 3 pieces x 3 gates x NT tiles x KS k-steps
  static_assert(H == 32 || H == 64, "split-bf16 ordered update: 32 or 64 units");
  __shared__ float sbias[4 * H];
  __shared__ bf8 su[NF * 64];
  for (int i = threadIdx.x; i < 4 * H; i += blockDim.x) sbias[i] = a.bias[i];
  {
    const u4v* src = reinterpret_cast<const u4v*>(a.Ubf);
    u4v* dst = reinterpret_cast<u4v*>(su);
    for (int e = threadIdx.x; e < NF * 64; e += blockDim.x) dst[e] = src[e];
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
    for (int o = 32; o >= 1; o >>= 1) Lmax = max(Lmax, __shfl_xor(Lmax, o));
    float* hsv = nullptr;
    if constexpr (SAVE) {
      hsv = a.hs_save + (valid ? (int64_t)a.step_ptr[pos] + pos : 0) * H + 4 * g;
      if (valid) {
#pragma unroll
        for (int t = 0; t < NT; ++t) st4(hsv + 16 * t, h[t]);
      }
    }
    // the projected row of step t is loaded at the start of step t and consumed by the gates after
    // the h.U MFMAs (measured faster than a one-step-ahead prefetch at 3 waves per SIMD or seeded
    // into the first MFMA's C operand: profiles/r02/seq_experiments)
    uint32_t code = codes[0];
    for (int t = 0; t < Lmax; ++t) {
      f4 x[3][NT];
      {
        const float* p = tab + (int64_t)code * (3 * H);
#pragma unroll
        for (int G = 0; G < 3; ++G)
#pragma unroll
          for (int i = 0; i < NT; ++i) x[G][i] = ld4(p + G * H + 16 * i);
      }
      const uint32_t next = codes[t + 1];
      // B fragments: the three exact bf16 pieces of the state, k-step s = accumulator tiles 2s, 2s+1
      bf8 hf[3][KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        u4v w0, w1, w2;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e0 = 2 * q, e1 = 2 * q + 1;
          float a0, a1, a2, b0, b1, b2;
          split3(h[2 * s + (e0 >> 2)][e0 & 3], a0, a1, a2);
          split3(h[2 * s + (e1 >> 2)][e1 & 3], b0, b1, b2);
          w0[q] = pack_hi16(a0, b0);
          w1[q] = pack_hi16(a1, b1);
          w2[q] = pack_hi16(a2, b2);
        }
        hf[0][s] = __builtin_bit_cast(bf8, w0);
        hf[1][s] = __builtin_bit_cast(bf8, w1);
        hf[2][s] = __builtin_bit_cast(bf8, w2);
      }
      f4 acc[3][NT];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        acc[0][i] = f4{0, 0, 0, 0};
        acc[1][i] = f4{0, 0, 0, 0};
        acc[2][i] = *reinterpret_cast<const f4*>(sbias + 3 * H + 16 * i + 4 * g);
      }
      // the fragment reads are loop-invariant: an opaque lane offset keeps the compiler from
      // hoisting all of them out of the step loop into registers (occupancy)
      int lofs = lane;
      asm volatile("" : "+v"(lofs));
      // piece products, grouped by U piece (each A fragment read once per step), small first:
      // x9: U lo x {lo, mid, hi}, U mid x {lo, mid, hi}, U hi x {lo, mid, hi}
      // x6: U lo x hi, U mid x {mid, hi}, U hi x {lo, mid, hi}
#pragma unroll
      for (int pu = 2; pu >= 0; --pu) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
          for (int i = 0; i < NT; ++i) {
            bf8 w[3];
#pragma unroll
            for (int G = 0; G < 3; ++G) w[G] = su[(((pu * 3 + G) * NT + i) * KS + s) * 64 + lofs];
#pragma unroll
            for (int ph = 2; ph >= 0; --ph) {
              if (PASSES == 6 && pu + ph > 2) continue;
#pragma unroll
              for (int G = 0; G < 3; ++G) acc[G][i] = MFMA_BF(w[G], hf[ph][s], acc[G][i]);
            }
          }
        }
      }
      const bool act = t < L;
#pragma unroll
      for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {   // x rows carry the input-side biases (project_kernel)
          const float z = sig2_(acc[0][i][r] + x[0][i][r]);
          const float rr = sig2_(acc[1][i][r] + x[1][i][r]);
          const float c = tanh2_(x[2][i][r] + rr * acc[2][i][r]);
          const float hn = c + z * (h[i][r] - c);
          h[i][r] = act ? hn : h[i][r];
        }
      }
      if constexpr (SAVE) {
        if (act && valid) {
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
  }  // tile loop
}

// ---------------------------------------------------------------------------------------------
// Variants 6 / 7 of the ordered update: seq_gru_bf's recurrence with h.U from scaled two-piece
// fp16 operands (device_common.h split2h) on v_mfma_f32_16x16x32_f16: 3 (variant 6) or 4
// (variant 7, adds lo*lo) products per gate tile instead of 6, and 2 pieces to split per state
// value instead of 3.
// Scales (exact powers of two, so every product is the fp32 product of the scaled values):
// - U (pre-scaled as for pack_gru) by sigma = 2^(14 - floor(log2 max|U|)), once at pack time
//   (pack_u_f16_kernel, stored after the fragments);
// - the wave's state by S = 2^(15 - E), m = max(1, max |h| over the tile's 16 rows) < 2^E.  The
//   GRU keeps |h| <= max(|h_0|, 1) along the sequence (h' = z h + (1 - z) tanh, a convex
//   combination), so |S h| < 2^15 holds at every step and the fp16 pieces never overflow.
// The kernel carries S h: with SS = S sigma and c = 1 / SS the gate arithmetic absorbs the
// scales at no extra instruction:
//   z  = 1 / (1 + 2^(c acc_z + x_z))
//   rc = 1 / ((1 + 2^(c acc_r + x_r)) SS)            (= r / SS)
//   n' = S tanh2_(x_n + rc acc_n)                     (acc_n seeded with SS b_n)
//   h' = n' + z (h' - n')
// SAVE (training forward, PASSES 3): also writes every state of the sequence to hs_save as
// seq_gru_bf<SAVE> does (the state before, then the state after each step, unscaled), for the
// backward's bitwise gate recompute (train_kernels.hip seq_gru_bwd_kernel<H, true, 2>).
#ifdef IGN_SEQ_STAMP
// Diagnostic build only (tools/build_ab.sh NAME -DIGN_SEQ_STAMP; tools/probes/seq_stamps.py): per
// wave of the inference ordered update, s_memtime sums of its segments (cdna_hip_programming.md §7,
// In-kernel stamps).  The stamps' waits and sched barriers change the schedule: read the shares.
__device__ unsigned long long ign_seq_stamps[4096 * 8];
#define IGN_STAMP(v)                                                                      \
  do {                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");             \
    __builtin_amdgcn_sched_barrier(0);                                                    \
  } while (0)
extern "C" int ign_debug_seq_stamps(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(ign_seq_stamps), (size_t)n * 8, 0, hipMemcpyDeviceToHost);
}
#endif
template <int H, int PASSES, bool SAVE = false>
__global__ __launch_bounds__(256) void seq_gru_h16_kernel(SeqGruArgs a) {
  constexpr int NT = H / 16, KS = H / 32;
  constexpr int NF = 6 * NT * KS;            // fragments: 2 pieces x 3 gates x NT tiles x KS k-steps
  static_assert(H == 32 || H == 64, "split-fp16 ordered update: 32 or 64 units");
  static_assert(PASSES == 3, "3 piece products (lo*lo dropped)");
  __shared__ float sbias[H];
  __shared__ float sbn[4][H];                // per wave: the candidate's recurrent bias times SS
  __shared__ h8 su[NF * 64];
  for (int i = threadIdx.x; i < H; i += blockDim.x) sbias[i] = a.bias[3 * H + i];
  {
    const u4v* src = reinterpret_cast<const u4v*>(a.Uh);
    u4v* dst = reinterpret_cast<u4v*>(su);
    for (int e = threadIdx.x; e < NF * 64; e += blockDim.x) dst[e] = src[e];
  }
  // sigma's exponent (stored after the fragments by pack_u_f16_kernel)
  const int es = __float_as_int(reinterpret_cast<const float*>(a.Uh)[(int64_t)NF * 64 * 4]);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const float* tab = a.table + 4 * g;
  __syncthreads();
  const int64_t n_tiles = (a.n_dst + 15) / 16;
  const int64_t tile_stride = (int64_t)gridDim.x * 4;
  // Tile prologue, one memory round trip: the 16-B position headers (row, final_len, first step,
  // first step's code; padded to whole tiles with empty positions) of the wave's next tile are
  // loaded while the current tile runs, so a tile starts by issuing its state rows and first
  // projected rows together.  No branch guards a load.
  int64_t tile = xcd_block(a.xcd_remap) * 4 + wave;
  i4v hd = *reinterpret_cast<const i4v*>(a.hdr + 4 * (min(tile, n_tiles - 1) * 16 + j));
#ifdef IGN_SEQ_STAMP
  unsigned long long s_pro = 0, s_mma = 0, s_gate = 0, s_epi = 0, n_tl = 0, n_st = 0, t_0, t_1, t_2, t_3;
  IGN_STAMP(t_0);
  const unsigned long long t_begin = t_0;
#endif
  for (; tile < n_tiles; tile += tile_stride) {
#ifdef IGN_SEQ_STAMP
    IGN_STAMP(t_0);
#endif
    const int64_t pos = tile * 16 + j;
    const bool valid = pos < a.n_dst;
    const int row = hd[0];
    const int L = hd[1];
    const uint32_t* codes = a.step_code + hd[2];
    float* hsv = nullptr;
    if constexpr (SAVE) hsv = a.hs_save + ((int64_t)hd[2] + pos) * H + 4 * g;
    f4 h[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const f4 v = ld4(a.h_in + (int64_t)row * H + 16 * t + 4 * g);
      h[t] = valid ? v : f4{0, 0, 0, 0};
    }
    // the first step's projected rows (and the second step's code) are in flight with the state
    f4 x[3][NT];
    {
      const float* p = tab + (int64_t)(uint32_t)hd[3] * (3 * H);
#pragma unroll
      for (int G = 0; G < 3; ++G)
#pragma unroll
        for (int i = 0; i < NT; ++i) x[G][i] = ld4(p + G * H + 16 * i);
    }
    uint32_t code = codes[1];
    if constexpr (SAVE) {
      if (valid) {
#pragma unroll
        for (int t = 0; t < NT; ++t) st4(hsv + 16 * t, h[t]);
      }
    }
    hd = *reinterpret_cast<const i4v*>(a.hdr + 4 * (min(tile + tile_stride, n_tiles - 1) * 16 + j));
    // positions are sorted by final_len, descending: lane 0 (position tile * 16) is the longest
    const int Lmax = __builtin_amdgcn_readfirstlane(L);
    float m = 1.0f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) m = fmaxf(m, fabsf(h[t][r]));
    // m = max(1, max |h|) over the tile: after the first iteration every |h| <= 1 (a GRU output
    // is a convex combination of h and tanh), so a ballot settles it; the cross-lane reduction
    // runs only for a tile that holds a larger state
    if (__ballot(m > 1.0f) != 0) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    }
    // m = f 2^E, f in [0.5, 1): S = 2^(15 - E); SS = S sigma
    const int E = (__builtin_amdgcn_readfirstlane(__float_as_int(m)) >> 23) - 126;
    const int eS = 15 - E;
    const float S = __int_as_float((127 + eS) << 23);
    const float SS = __int_as_float((127 + eS + es) << 23);
    const float c = __int_as_float((127 - eS - es) << 23);
    const float iS = __int_as_float((127 - eS) << 23);
    // every lane writes (and later reads back) exactly its own bias slots: no cross-lane hand-off
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      h[t] *= S;
      *reinterpret_cast<f4*>(&sbn[wave][16 * t + 4 * g]) = *reinterpret_cast<const f4*>(sbias + 16 * t + 4 * g) * SS;
    }
    auto load_x = [&](uint32_t code, f4 (&x)[3][NT]) {
      const float* p = tab + (int64_t)code * (3 * H);
#pragma unroll
      for (int G = 0; G < 3; ++G)
#pragma unroll
        for (int i = 0; i < NT; ++i) x[G][i] = ld4(p + G * H + 16 * i);
    };
    // MASKED: some row of the tile ends before step t (t >= the tile's shortest final_len);
    // the steps before that update every row without a select
    auto step = [&](int t, const f4 (&x)[3][NT], auto masked) __attribute__((always_inline)) {
      // B fragments: the two fp16 pieces of the scaled state, k-step s = accumulator tiles 2s, 2s+1
      h8 hf[2][KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        u4v w0, w1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e0 = 2 * q, e1 = 2 * q + 1;
          const hpair p = split2h(h[2 * s + (e0 >> 2)][e0 & 3], h[2 * s + (e1 >> 2)][e1 & 3]);
          w0[q] = p.hi;
          w1[q] = p.lo;
        }
        hf[0][s] = __builtin_bit_cast(h8, w0);
        hf[1][s] = __builtin_bit_cast(h8, w1);
      }
      f4 acc[3][NT];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        acc[0][i] = f4{0, 0, 0, 0};
        acc[1][i] = f4{0, 0, 0, 0};
        acc[2][i] = *reinterpret_cast<const f4*>(&sbn[wave][16 * i + 4 * g]);
      }
      // the fragment reads are loop-invariant: an opaque lane offset keeps the compiler from
      // hoisting them out of the step loop into registers (occupancy)
      int lofs = lane;
      asm volatile("" : "+v"(lofs));
      // U lo x {lo (x4), hi}, then U hi x {lo, hi}: small products first
#pragma unroll
      for (int pu = 1; pu >= 0; --pu) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
          for (int i = 0; i < NT; ++i) {
            h8 w[3];
#pragma unroll
            for (int G = 0; G < 3; ++G) w[G] = su[(((pu * 3 + G) * NT + i) * KS + s) * 64 + lofs];
#pragma unroll
            for (int ph = 1; ph >= 0; --ph) {
              if (PASSES == 3 && pu + ph > 1) continue;
#pragma unroll
              for (int G = 0; G < 3; ++G) acc[G][i] = MFMA_H(w[G], hf[ph][s], acc[G][i]);
            }
          }
        }
      }
      const bool act = t < L;
#ifdef IGN_SEQ_STAMP
      if constexpr (!SAVE) {
        IGN_STAMP(t_2);
        s_mma += t_2 - t_1;
      }
#endif
#pragma unroll
      for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {   // x rows carry the input-side biases (project_kernel)
          const float z = rcpf_(1.0f + __builtin_amdgcn_exp2f(fmaf(acc[0][i][r], c, x[0][i][r])));
          const float rc = rcpf_(fmaf(__builtin_amdgcn_exp2f(fmaf(acc[1][i][r], c, x[1][i][r])), SS, SS));
          const float n = S * tanh2_(fmaf(rc, acc[2][i][r], x[2][i][r]));
          const float hn = n + z * (h[i][r] - n);
          if constexpr (decltype(masked)::value) h[i][r] = act ? hn : h[i][r];
          else h[i][r] = hn;
        }
      }
    };
    auto save = [&](int t) __attribute__((always_inline)) {   // the state after step t
      if constexpr (SAVE) {
        if (valid && t < L) {
#pragma unroll
          for (int i = 0; i < NT; ++i) st4(hsv + (int64_t)(t + 1) * H + 16 * i, h[i] * iS);
        }
      }
    };
    // the projected row of step t is loaded at the start of step t and consumed by the gates after
    // the h.U MFMAs (a two-buffer one-step-ahead prefetch, loop unrolled by two, measured slower:
    // 0.242 vs 0.214 ms per launch, 144 VGPRs -> 3 waves per SIMD)
    // every tile has Lmax >= 1 (a destination without messages is rejected at batch build);
    // Lmin: final_len of the tile's last valid position (sorted descending); padding lanes of
    // the last tile run the unmasked steps too, harmlessly (their rows are never stored)
    const int Lmin = __builtin_amdgcn_readlane(L, (int)min<int64_t>(15, a.n_dst - 1 - tile * 16));
#ifdef IGN_SEQ_STAMP
    IGN_STAMP(t_1);
    s_pro += t_1 - t_0;
#endif
    for (int t = 0;;) {
#ifdef IGN_SEQ_STAMP
      IGN_STAMP(t_1);
#endif
      if (t < Lmin) step(t, x, std::false_type{});
      else step(t, x, std::true_type{});
      save(t);
#ifdef IGN_SEQ_STAMP
      IGN_STAMP(t_3);
      s_gate += t_3 - t_2;
      ++n_st;
#endif
      if (++t >= Lmax) break;
      load_x(code, x);
      code = codes[t + 1];
    }
#ifdef IGN_SEQ_STAMP
    IGN_STAMP(t_1);
#endif
    if (valid) {
#pragma unroll
      for (int t = 0; t < NT; ++t) st4(a.h_out + (int64_t)row * H + 16 * t + 4 * g, h[t] * iS);
    }
#ifdef IGN_SEQ_STAMP
    IGN_STAMP(t_2);
    s_epi += t_2 - t_1;
    ++n_tl;
#endif
  }  // tile loop
#ifdef IGN_SEQ_STAMP
  if constexpr (!SAVE) {
    IGN_STAMP(t_3);
    const int gw = blockIdx.x * 4 + wave;
    if (lane == 0 && gw < 4096) {
      unsigned long long* o = ign_seq_stamps + 8 * gw;
      o[0] = s_pro; o[1] = s_mma; o[2] = s_gate; o[3] = s_epi; o[4] = n_tl; o[5] = n_st;
      o[6] = t_3 - t_begin; o[7] = 1;
    }
  }
#endif
}

// U (pre-scaled as for pack_gru) -> sigma U as fp16 (hi, lo) A fragments of seq_gru_h16 (layout of
// pack_u_bf16 with 2 pieces), then sigma's exponent as an int after them.  One block.
__global__ __launch_bounds__(1024) void pack_u_f16_kernel(const float* __restrict__ U, uint16_t* __restrict__ out,
                                                         int K, int H) {
  const int NT = H / 16, KS = K / 32, n = K * 3 * H;
  __shared__ float red[1024];
  float m = 0.f;
  for (int e = threadIdx.x; e < n; e += blockDim.x) {
    const float sc = (e % (3 * H)) >= 2 * H ? IGN_2LOG2E : IGN_NLOG2E;
    m = fmaxf(m, fabsf(sc * U[e]));
  }
  red[threadIdx.x] = m;
  __syncthreads();
  for (int o = blockDim.x / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  m = red[0];
  // sigma = 2^(15 - E) with m = f 2^E, f in [0.5, 1): max |sigma U| < 2^15; clamped for tiny / zero U
  int es = m > 0.f ? 15 - ((__float_as_int(m) >> 23) - 126) : 0;
  es = min(100, max(-100, es));
  const float sigma = __int_as_float((127 + es) << 23);
  const int64_t total = 6LL * NT * KS * 64 * 8;
  for (int64_t e = threadIdx.x; e < total; e += blockDim.x) {
    const int jj = (int)(e & 7), lane = (int)((e >> 3) & 63);
    int64_t f = e >> 9;                       // ((piece * 3 + gate) * NT + tile) * KS + s
    const int s = (int)(f % KS); f /= KS;
    const int i = (int)(f % NT); f /= NT;
    const int G = (int)(f % 3);
    const int piece = (int)(f / 3);
    const int k = 16 * (2 * s + (jj >> 2)) + 4 * (lane >> 4) + (jj & 3);
    const int col = G * H + 16 * i + (lane & 15);
    const float sc = G == 2 ? IGN_2LOG2E : IGN_NLOG2E;
    const float v = sigma * (sc * U[(int64_t)k * 3 * H + col]);
    const _Float16 hi = (_Float16)v;
    const _Float16 p = piece == 0 ? hi : (_Float16)(v - (float)hi);
    out[e] = __builtin_bit_cast(uint16_t, p);
  }
  if (threadIdx.x == 0) reinterpret_cast<int*>(out)[total / 2] = es;
}

// ---------------------------------------------------------------------------------------------
// Variant 7 of the sum update (kernels.hip sum_gru_lds, DIN = H = 64): the same persistent,
// in-degree-sorted tiles and message gather, with x.W and h.U on the bf16 matrix path,
// fp32-exact (6 piece products).  At 64/64 the f32 form issues 384 f32 MFMAs per
// 16 rows (12.3k cycles); this one 288 bf16 MFMAs (~4.6k) plus the splits of x and h.
// W and U pieces (147 KB) are staged once per block in LDS: one 12-wave block per CU.
__device__ __forceinline__ const float* src_row_bf(const SrcBases& sb, uint32_t code, int din) {
  const uint32_t slot = code >> IGN_SLOT_SHIFT;
  const float* b = sb.base[0];
  if (slot == 1) b = sb.base[1];
  if (slot == 2) b = sb.base[2];
  if (slot == 3) b = sb.base[3];
  return b + (int64_t)(code & IGN_ROW_MASK) * din;
}

// B fragments of a lane's values v[2 * KS] (chained k order): the three exact bf16 pieces
template <int KS>
__device__ __forceinline__ void split_frags(const f4* v, bf8 (&f)[3][KS]) {
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    u4v w0, w1, w2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e0 = 2 * q, e1 = 2 * q + 1;
      float a0, a1, a2, b0, b1, b2;
      split3(v[2 * s + (e0 >> 2)][e0 & 3], a0, a1, a2);
      split3(v[2 * s + (e1 >> 2)][e1 & 3], b0, b1, b2);
      w0[q] = pack_hi16(a0, b0);
      w1[q] = pack_hi16(a1, b1);
      w2[q] = pack_hi16(a2, b2);
    }
    f[0][s] = __builtin_bit_cast(bf8, w0);
    f[1][s] = __builtin_bit_cast(bf8, w1);
    f[2][s] = __builtin_bit_cast(bf8, w2);
  }
}

template <int DIN, int H, int WAVES, int GU>
__global__ __launch_bounds__(64 * WAVES) void sum_gru_bf_kernel(SumGruArgs a) {
  constexpr int NC = DIN / 16, NT = H / 16, KX = DIN / 32, KH = H / 32;
  constexpr int WF = 9 * NT * KX * 64, UF = 9 * NT * KH * 64;   // bf8 fragments (16 B)
  __shared__ bf8 sW[WF];
  __shared__ bf8 sU[UF];
  __shared__ float sbias[4 * H];
  {
    const u4v* gW = static_cast<const u4v*>(a.Wbf);
    const u4v* gU = static_cast<const u4v*>(a.Ubf);
    u4v* dW = reinterpret_cast<u4v*>(sW);
    u4v* dU = reinterpret_cast<u4v*>(sU);
    for (int i = threadIdx.x; i < WF; i += 64 * WAVES) dW[i] = gW[i];
    for (int i = threadIdx.x; i < UF; i += 64 * WAVES) dU[i] = gU[i];
    for (int i = threadIdx.x; i < 4 * H; i += 64 * WAVES) sbias[i] = a.bias[i];
  }
  __syncthreads();
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
    f4 h[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) h[t] = valid ? ld4(a.h_in + (int64_t)row * H + 16 * t + 4 * g) : f4{0, 0, 0, 0};
    f4 x[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) x[c] = f4{0, 0, 0, 0};
    // the same summation order as sum_gru_lds (GU at a time, then pairs, then singles)
    int64_t m = m0;
    for (; m + GU <= m1; m += GU) {
      f4 v[GU][NC];
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        const float* p = src_row_bf(a.src, a.msg_src[m + u], DIN);
#pragma unroll
        for (int c = 0; c < NC; ++c) v[u][c] = ld4(p + 16 * c + 4 * g);
      }
#pragma unroll
      for (int u = 0; u < GU; ++u)
#pragma unroll
        for (int c = 0; c < NC; ++c) x[c] += v[u][c];
    }
    for (; m + 2 <= m1; m += 2) {
      const float* p0 = src_row_bf(a.src, a.msg_src[m], DIN);
      const float* p1 = src_row_bf(a.src, a.msg_src[m + 1], DIN);
      f4 v0[NC], v1[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        v0[c] = ld4(p0 + 16 * c + 4 * g);
        v1[c] = ld4(p1 + 16 * c + 4 * g);
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) x[c] = (x[c] + v0[c]) + v1[c];
    }
    for (; m < m1; ++m) {
      const float* p = src_row_bf(a.src, a.msg_src[m], DIN);
#pragma unroll
      for (int c = 0; c < NC; ++c) x[c] += ld4(p + 16 * c + 4 * g);
    }
    if (a.x_save && valid) {
#pragma unroll
      for (int c = 0; c < NC; ++c) st4(a.x_save + (int64_t)row * DIN + 16 * c + 4 * g, x[c]);
    }
    bf8 xf[3][KX], hf[3][KH];
    split_frags<KX>(x, xf);
    split_frags<KH>(h, hf);
    int lofs = lane;                    // opaque: keeps the fragment reads inside the tile loop
    asm volatile("" : "+v"(lofs));
    f4 hn[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int u0 = 16 * t + 4 * g;
      f4 az = *reinterpret_cast<const f4*>(sbias + 0 * H + u0);
      f4 ar = *reinterpret_cast<const f4*>(sbias + 1 * H + u0);
      f4 ax = *reinterpret_cast<const f4*>(sbias + 2 * H + u0);
      f4 ah = *reinterpret_cast<const f4*>(sbias + 3 * H + u0);
      // piece products grouped by weight piece, small first; x6 drops pu + ph > 2
#pragma unroll
      for (int pu = 2; pu >= 0; --pu) {
#pragma unroll
        for (int s = 0; s < KX; ++s) {
          const bf8 wz = sW[(((pu * 3 + 0) * NT + t) * KX + s) * 64 + lofs];
          const bf8 wr = sW[(((pu * 3 + 1) * NT + t) * KX + s) * 64 + lofs];
          const bf8 wh = sW[(((pu * 3 + 2) * NT + t) * KX + s) * 64 + lofs];
#pragma unroll
          for (int ph = 2 - pu; ph >= 0; --ph) {
            az = MFMA_BF(wz, xf[ph][s], az);
            ar = MFMA_BF(wr, xf[ph][s], ar);
            ax = MFMA_BF(wh, xf[ph][s], ax);
          }
        }
#pragma unroll
        for (int s = 0; s < KH; ++s) {
          const bf8 wz = sU[(((pu * 3 + 0) * NT + t) * KH + s) * 64 + lofs];
          const bf8 wr = sU[(((pu * 3 + 1) * NT + t) * KH + s) * 64 + lofs];
          const bf8 wh = sU[(((pu * 3 + 2) * NT + t) * KH + s) * 64 + lofs];
#pragma unroll
          for (int ph = 2 - pu; ph >= 0; --ph) {
            az = MFMA_BF(wz, hf[ph][s], az);
            ar = MFMA_BF(wr, hf[ph][s], ar);
            ah = MFMA_BF(wh, hf[ph][s], ah);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = sig2_(az[r]);
        const float rr = sig2_(ar[r]);
        const float c = tanh2_(ax[r] + rr * ah[r]);
        hn[t][r] = c + z * (h[t][r] - c);
      }
    }
    if (valid) {
#pragma unroll
      for (int t = 0; t < NT; ++t) st4(a.h_out + (int64_t)row * H + 16 * t + 4 * g, hn[t]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Variant 8 of the sum update at DIN = H = 64: sum_gru_bf with x.W and h.U on scaled two-piece
// fp16 operands (3 products, v_mfma_f32_16x16x32_f16; device_common.h split2h): 144 MFMAs per
// 16-row tile instead of 288, and 2 pieces to split per value instead of 3.  W and U carry
// pack-time powers of two (sigma_W, sigma_U); the tile's message sums x and states h are scaled so
// that both products land on ONE accumulator scale K = S_x sigma_W = S_h sigma_U, the largest with
// |S_x x| < 2^15 and |S_h h| < 2^15 (m = f 2^E, f in [0.5, 1) -> S <= 2^(15 - E)).  The biases seed
// the accumulators times K and the gates take c = 1 / K.
template <int DIN, int H, int WAVES, int GU>
__global__ __launch_bounds__(64 * WAVES) void sum_gru_h16_kernel(SumGruArgs a) {
  constexpr int NC = DIN / 16, NT = H / 16, KX = DIN / 32, KH = H / 32;
  constexpr int WF = 6 * NT * KX * 64, UF = 6 * NT * KH * 64;   // h8 fragments (16 B)
  __shared__ h8 sW[WF];
  __shared__ h8 sU[UF];
  __shared__ float sbias[4 * H];
  {
    const u4v* gW = static_cast<const u4v*>(a.Wbf);
    const u4v* gU = static_cast<const u4v*>(a.Ubf);
    u4v* dW = reinterpret_cast<u4v*>(sW);
    u4v* dU = reinterpret_cast<u4v*>(sU);
    for (int i = threadIdx.x; i < WF; i += 64 * WAVES) dW[i] = gW[i];
    for (int i = threadIdx.x; i < UF; i += 64 * WAVES) dU[i] = gU[i];
    for (int i = threadIdx.x; i < 4 * H; i += 64 * WAVES) sbias[i] = a.bias[i];
  }
  const int esW = reinterpret_cast<const int*>(a.Wbf)[WF * 4];   // after the fragments (pack_u_f16)
  const int esU = reinterpret_cast<const int*>(a.Ubf)[UF * 4];
  __syncthreads();
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
    f4 h[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) h[t] = valid ? ld4(a.h_in + (int64_t)row * H + 16 * t + 4 * g) : f4{0, 0, 0, 0};
    f4 x[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) x[c] = f4{0, 0, 0, 0};
    // the same summation order as sum_gru_bf / sum_gru_lds (GU at a time, then pairs, then singles)
    int64_t m = m0;
    for (; m + GU <= m1; m += GU) {
      f4 v[GU][NC];
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        const float* p = src_row_bf(a.src, a.msg_src[m + u], DIN);
#pragma unroll
        for (int c = 0; c < NC; ++c) v[u][c] = ld4(p + 16 * c + 4 * g);
      }
#pragma unroll
      for (int u = 0; u < GU; ++u)
#pragma unroll
        for (int c = 0; c < NC; ++c) x[c] += v[u][c];
    }
    for (; m + 2 <= m1; m += 2) {
      const float* p0 = src_row_bf(a.src, a.msg_src[m], DIN);
      const float* p1 = src_row_bf(a.src, a.msg_src[m + 1], DIN);
      f4 v0[NC], v1[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        v0[c] = ld4(p0 + 16 * c + 4 * g);
        v1[c] = ld4(p1 + 16 * c + 4 * g);
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) x[c] = (x[c] + v0[c]) + v1[c];
    }
    for (; m < m1; ++m) {
      const float* p = src_row_bf(a.src, a.msg_src[m], DIN);
#pragma unroll
      for (int c = 0; c < NC; ++c) x[c] += ld4(p + 16 * c + 4 * g);
    }
    if (a.x_save && valid) {
#pragma unroll
      for (int c = 0; c < NC; ++c) st4(a.x_save + (int64_t)row * DIN + 16 * c + 4 * g, x[c]);
    }
    // one accumulator scale K for both products (see above)
    float mx = 1e-18f, mh = 1e-18f;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int q = 0; q < 4; ++q) mx = fmaxf(mx, fabsf(x[c][q]));
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) mh = fmaxf(mh, fabsf(h[t][q]));
    mx = wave_max_nonneg(mx);
    mh = wave_max_nonneg(mh);
    const int Ex = (__builtin_amdgcn_readfirstlane(__float_as_int(mx)) >> 23) - 126;
    const int Eh = (__builtin_amdgcn_readfirstlane(__float_as_int(mh)) >> 23) - 126;
    const int eK = min(100, min(15 - Ex + esW, 15 - Eh + esU));
    const float Sx = __int_as_float((127 + max(-120, eK - esW)) << 23);
    const float Sh = __int_as_float((127 + max(-120, eK - esU)) << 23);
    const float K = __int_as_float((127 + max(-120, eK)) << 23);
    const float c = __int_as_float((127 - max(-120, eK)) << 23);
    h8 xf[2][KX], hf[2][KH];
#pragma unroll
    for (int s = 0; s < KX; ++s) {
      u4v w0, w1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e0 = 2 * q, e1 = 2 * q + 1;
        const hpair p = split2h(x[2 * s + (e0 >> 2)][e0 & 3] * Sx, x[2 * s + (e1 >> 2)][e1 & 3] * Sx);
        w0[q] = p.hi;
        w1[q] = p.lo;
      }
      xf[0][s] = __builtin_bit_cast(h8, w0);
      xf[1][s] = __builtin_bit_cast(h8, w1);
    }
#pragma unroll
    for (int s = 0; s < KH; ++s) {
      u4v w0, w1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e0 = 2 * q, e1 = 2 * q + 1;
        const hpair p = split2h(h[2 * s + (e0 >> 2)][e0 & 3] * Sh, h[2 * s + (e1 >> 2)][e1 & 3] * Sh);
        w0[q] = p.hi;
        w1[q] = p.lo;
      }
      hf[0][s] = __builtin_bit_cast(h8, w0);
      hf[1][s] = __builtin_bit_cast(h8, w1);
    }
    int lofs = lane;                    // opaque: keeps the fragment reads inside the tile loop
    asm volatile("" : "+v"(lofs));
    f4 hn[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int u0 = 16 * t + 4 * g;
      f4 az = *reinterpret_cast<const f4*>(sbias + 0 * H + u0) * K;
      f4 ar = *reinterpret_cast<const f4*>(sbias + 1 * H + u0) * K;
      f4 ax = *reinterpret_cast<const f4*>(sbias + 2 * H + u0) * K;
      f4 ah = *reinterpret_cast<const f4*>(sbias + 3 * H + u0) * K;
      // piece products grouped by weight piece: W lo x {hi}, W hi x {lo, hi}
#pragma unroll
      for (int pu = 1; pu >= 0; --pu) {
#pragma unroll
        for (int s = 0; s < KX; ++s) {
          const h8 wz = sW[(((pu * 3 + 0) * NT + t) * KX + s) * 64 + lofs];
          const h8 wr = sW[(((pu * 3 + 1) * NT + t) * KX + s) * 64 + lofs];
          const h8 wh = sW[(((pu * 3 + 2) * NT + t) * KX + s) * 64 + lofs];
#pragma unroll
          for (int ph = 1 - pu; ph >= 0; --ph) {
            az = MFMA_H(wz, xf[ph][s], az);
            ar = MFMA_H(wr, xf[ph][s], ar);
            ax = MFMA_H(wh, xf[ph][s], ax);
          }
        }
#pragma unroll
        for (int s = 0; s < KH; ++s) {
          const h8 wz = sU[(((pu * 3 + 0) * NT + t) * KH + s) * 64 + lofs];
          const h8 wr = sU[(((pu * 3 + 1) * NT + t) * KH + s) * 64 + lofs];
          const h8 wh = sU[(((pu * 3 + 2) * NT + t) * KH + s) * 64 + lofs];
#pragma unroll
          for (int ph = 1 - pu; ph >= 0; --ph) {
            az = MFMA_H(wz, hf[ph][s], az);
            ar = MFMA_H(wr, hf[ph][s], ar);
            ah = MFMA_H(wh, hf[ph][s], ah);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = sig2_(az[r] * c);
        const float rr = sig2_(ar[r] * c);
        const float cc = tanh2_(fmaf(rr, ah[r], ax[r]) * c);
        hn[t][r] = cc + z * (h[t][r] - cc);
      }
    }
    if (valid) {
#pragma unroll
      for (int t = 0; t < NT; ++t) st4(a.h_out + (int64_t)row * H + 16 * t + 4 * g, hn[t]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Sum update at DIN = H = 32 (RouteNet's path -> link MP): a latency-bound gather of ~36 scattered
// 128-B rows per destination, then one GRU step.  One 16-destination tile per wave, no persistent
// loop (waves that finish free their slot for a new tile at once).  Against sum_gru_kernel<32,32>:
//  * the message codes of group k+1 load while the rows of group k are in flight (one memory
//    round trip per group instead of two); GU rows per lane in flight, codes clamped to the
//    destination's range (no branches around loads) and the adds predicated, in message order;
//  * the GRU step on the split-bf16 path (x6) with W / U pieces in LDS, staged by LDS-DMA while
//    the gather runs, instead of 96 f32 MFMAs with the weights in 96 VGPRs: about half the
//    registers, so twice the waves (and rows in flight) per SIMD.
// The message sum associates exactly as in sum_gru_kernel (one message at a time, in CSR order).
template <int GU>
__global__ __launch_bounds__(256) void sum_gru_g32_kernel(SumGruArgs a) {
  constexpr int DIN = 32, H = 32, NC = 2, NT = 2, NF = 18;   // fragments per matrix
  __shared__ bf8 sw[2 * NF * 64];                              // W pieces | U pieces
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  {   // 36 KB: 9 LDS-DMA pieces of 1 KB per wave, in flight during the gather
    const u4v* gw = static_cast<const u4v*>(a.Wbf);
    const u4v* gu = static_cast<const u4v*>(a.Ubf);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int piece = k * 4 + wave;                          // 0 .. 35
      const u4v* src = piece < NF ? gw + piece * 64 + lane : gu + (piece - NF) * 64 + lane;
      __builtin_amdgcn_global_load_lds((const void*)src,
                                       (__attribute__((address_space(3))) void*)(sw + piece * 64), 16, 0, 0);
    }
  }
  const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
  const int64_t pos = tile * 16 + j;
  const bool valid = pos < a.n_dst;
  const int row = valid ? a.order[pos] : 0;
  const int64_t m0 = valid ? a.msg_ptr[pos] : 0;
  const int64_t m1 = valid ? a.msg_ptr[pos + 1] : 0;
  const int64_t last = m1 > 0 ? m1 - 1 : 0;
  f4 x[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) x[c] = f4{0, 0, 0, 0};
  uint32_t cc[GU];
#pragma unroll
  for (int u = 0; u < GU; ++u) cc[u] = a.msg_src[m0 + u < last ? m0 + u : last];
  for (int64_t m = m0; m < m1; m += GU) {
    f4 v[GU][NC];
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      const float* p = src_row_bf(a.src, cc[u], DIN) + 4 * g;
#pragma unroll
      for (int c = 0; c < NC; ++c) v[u][c] = ld4(p + 16 * c);
    }
#pragma unroll
    for (int u = 0; u < GU; ++u) cc[u] = a.msg_src[m + GU + u < last ? m + GU + u : last];
#pragma unroll
    for (int u = 0; u < GU; ++u) {
      const bool on = m + u < m1;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const f4 s = x[c] + v[u][c];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[c][q] = on ? s[q] : x[c][q];
      }
    }
  }
  if (a.x_save && valid) {
#pragma unroll
    for (int c = 0; c < NC; ++c) st4(a.x_save + (int64_t)row * DIN + 16 * c + 4 * g, x[c]);
  }
  f4 h[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) h[t] = valid ? ld4(a.h_in + (int64_t)row * H + 16 * t + 4 * g) : f4{0, 0, 0, 0};
  f4 bz[NT], br[NT], bx[NT], bh[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int u0 = 16 * t + 4 * g;
    bz[t] = ld4(a.bias + 0 * H + u0);
    br[t] = ld4(a.bias + 1 * H + u0);
    bx[t] = ld4(a.bias + 2 * H + u0);
    bh[t] = ld4(a.bias + 3 * H + u0);
  }
  bf8 xf[3][1], hf[3][1];
  split_frags<1>(x, xf);
  split_frags<1>(h, hf);
  __syncthreads();   // the block's LDS-DMA pieces have landed
  const bf8* sW = sw;
  const bf8* sU = sw + NF * 64;
  f4 hn[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f4 az = bz[t], ar = br[t], ax = bx[t], ah = bh[t];
#pragma unroll
    for (int pu = 2; pu >= 0; --pu) {   // as sum_gru_bf: weight piece major, small products first
      const bf8 wz = sW[((pu * 3 + 0) * NT + t) * 64 + lane];
      const bf8 wr = sW[((pu * 3 + 1) * NT + t) * 64 + lane];
      const bf8 wh = sW[((pu * 3 + 2) * NT + t) * 64 + lane];
#pragma unroll
      for (int ph = 2 - pu; ph >= 0; --ph) {
        az = MFMA_BF(wz, xf[ph][0], az);
        ar = MFMA_BF(wr, xf[ph][0], ar);
        ax = MFMA_BF(wh, xf[ph][0], ax);
      }
      const bf8 uz = sU[((pu * 3 + 0) * NT + t) * 64 + lane];
      const bf8 ur = sU[((pu * 3 + 1) * NT + t) * 64 + lane];
      const bf8 uh = sU[((pu * 3 + 2) * NT + t) * 64 + lane];
#pragma unroll
      for (int ph = 2 - pu; ph >= 0; --ph) {
        az = MFMA_BF(uz, hf[ph][0], az);
        ar = MFMA_BF(ur, hf[ph][0], ar);
        ah = MFMA_BF(uh, hf[ph][0], ah);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z = sig2_(az[r]);
      const float rr = sig2_(ar[r]);
      const float c = tanh2_(ax[r] + rr * ah[r]);
      hn[t][r] = c + z * (h[t][r] - c);
    }
  }
  if (valid) {
#pragma unroll
    for (int t = 0; t < NT; ++t) st4(a.h_out + (int64_t)row * H + 16 * t + 4 * g, hn[t]);
  }
  if (a.proj_out) {
    // the next ordered MP's input projection of the new states (project_kernel's rows, formed on
    // the split-bf16 path): hn is already in the chained B layout; W' pieces come from L2
    if (a.proj_bias_row && blockIdx.x == 0)
      for (int i = threadIdx.x; i < 3 * H; i += blockDim.x) a.proj_bias_row[i] = a.proj_b[i];
    bf8 pf[3][1];
    split_frags<1>(hn, pf);
    const bf8* pw = static_cast<const bf8*>(a.proj_W);
#pragma unroll
    for (int G = 0; G < 3; ++G)
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        f4 acc = ld4(a.proj_b + G * H + 16 * i + 4 * g);
#pragma unroll
        for (int pu = 2; pu >= 0; --pu) {
          const bf8 w = pw[((pu * 3 + G) * NT + i) * 64 + lane];
#pragma unroll
          for (int ph = 2 - pu; ph >= 0; --ph) acc = MFMA_BF(w, pf[ph][0], acc);
        }
        if (valid) st4(a.proj_out + (int64_t)row * 3 * H + G * H + 16 * i + 4 * g, acc);
      }
  }
}

hipError_t launch_sum_gru_g32(const SumGruArgs& args, int gu, hipStream_t st) {
  if (args.n_dst == 0) return hipSuccess;
  if (!args.Wbf || !args.Ubf || args.msg_w || args.conv_kp) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((args.n_dst + 63) / 64));
  if (gu != 6) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sum_gru_g32_kernel<6>, grid, dim3(256), 0, st, args);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Weight-gradient row contraction part[chunk] = sum_r A[r]^T B[r] (train_kernels.hip tsgemm) on
// the bf16 matrix path, fp32-exact (x6 piece products).  Rows sit on the k axis of
// v_mfma_f32_16x16x32_bf16: lane (c = l&15, g = l>>4) holds rows r + 8g .. r + 8g + 7 of column
// m0 + 16x + c (A) / n0 + 16y + c (B), so the loads stay 64-B row segments as in tsgemm.
// One wave = one 64x64 output tile; the ones column (bias gradient) is a VALU column sum of B.
__global__ __launch_bounds__(256) void tsgemm_bf_kernel(const float* __restrict__ A, int lda,
                                                        const float* __restrict__ B, int ldb, int64_t n_rows, int M,
                                                        int N, int ones, int64_t chunk, float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int Mx = M + ones;
  // M a multiple of 64 (the readout's 256-wide layers): the ones column would be a tile row of its
  // own whose waves load and split B for column sums only; the m0 = 0 tiles sum B's columns
  // instead (every wave holds its B columns anyway; the same sums in the same order)
  const bool fold = ones && M > 0 && M % 64 == 0;
  const int tiles_m = fold ? M / 64 : (Mx + 63) / 64, tiles_n = (N + 63) / 64;
  const int tile = blockIdx.y * (blockDim.x >> 6) + wave;
  if (tile >= tiles_m * tiles_n) return;
  const int m0 = (tile / tiles_n) * 64, n0 = (tile % tiles_n) * 64;
  const int na = max(0, min(4, (M - m0 + 15) / 16)), nb = min(4, (N - n0 + 15) / 16);
  const bool has_ones = ones && (fold ? m0 == 0 : M >= m0 && M < m0 + 64);
  const int64_t r0 = (int64_t)blockIdx.x * chunk;
  const int64_t r1 = std::min<int64_t>(n_rows, r0 + chunk);
  const int g = lane >> 4, c = lane & 15;
  f4 acc[4][4];
  float csum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = f4{0, 0, 0, 0};
  for (int64_t r = r0; r < r1; r += 32) {
    float bv[4][8];
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const int n = n0 + 16 * y + c;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int64_t rr = r + 8 * g + jj;
        bv[y][jj] = (y < nb && rr < r1 && n < N) ? B[rr * ldb + n] : 0.f;
      }
    }
    float av[4][8];
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int m = m0 + 16 * x + c;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int64_t rr = r + 8 * g + jj;
        av[x][jj] = (x < na && rr < r1 && m < M) ? A[rr * lda + m] : 0.f;
      }
    }
    bf8 bp[4][3];
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      u4v w0, w1, w2;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float a0, a1, a2, b0, b1, b2;
        split3(bv[y][2 * q], a0, a1, a2);
        split3(bv[y][2 * q + 1], b0, b1, b2);
        w0[q] = pack_hi16(a0, b0);
        w1[q] = pack_hi16(a1, b1);
        w2[q] = pack_hi16(a2, b2);
      }
      bp[y][0] = __builtin_bit_cast(bf8, w0);
      bp[y][1] = __builtin_bit_cast(bf8, w1);
      bp[y][2] = __builtin_bit_cast(bf8, w2);
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) csum[y] += bv[y][jj];
    }
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      if (x >= na) continue;
      u4v w0, w1, w2;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float a0, a1, a2, b0, b1, b2;
        split3(av[x][2 * q], a0, a1, a2);
        split3(av[x][2 * q + 1], b0, b1, b2);
        w0[q] = pack_hi16(a0, b0);
        w1[q] = pack_hi16(a1, b1);
        w2[q] = pack_hi16(a2, b2);
      }
      const bf8 ap[3] = {__builtin_bit_cast(bf8, w0), __builtin_bit_cast(bf8, w1), __builtin_bit_cast(bf8, w2)};
#pragma unroll
      for (int pa = 2; pa >= 0; --pa)
#pragma unroll
        for (int pb = 2 - pa; pb >= 0; --pb)
#pragma unroll
          for (int y = 0; y < 4; ++y)
            if (y < nb) acc[x][y] = MFMA_BF(ap[pa], bp[y][pb], acc[x][y]);
    }
  }
  float* P = part + (int64_t)blockIdx.x * Mx * N;
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const int n = n0 + 16 * y + c;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = m0 + 16 * x + 4 * g + q;
        if (x < na && y < nb && m < M && n < N) P[(int64_t)m * N + n] = acc[x][y][q];
      }
    }
  if (has_ones) {
#pragma unroll
    for (int y = 0; y < 4; ++y) {      // sum over the 4 row groups g (lanes c, c+16, c+32, c+48)
      float sm = csum[y];
      sm += __shfl_xor(sm, 16);
      sm += __shfl_xor(sm, 32);
      const int n = n0 + 16 * y + c;
      if (g == 0 && n < N) P[(int64_t)M * N + n] = sm;
    }
  }
}

// tsgemm_bf_kernel for M % 64 == N % 64 == 0 with the pieces split once per block: a block of
// mtb x tiles_n waves holds the tiles of mtb 64-column groups of A against all of B.  Per 32-row
// step every (column, 8-row group) pair of the block's A columns and of B is loaded once (64 lanes =
// 64 consecutive columns of one row per load), split into its three bf16 pieces and written to LDS
// as 16-B fragments [piece][column][row group]; the waves read their MFMA operands from there (one
// contiguous 1 KB per fragment read).  Two buffers: the next step's pieces are loaded and split
// while this step's MFMAs run, one barrier per step (1.53 -> 1.38 ms against one buffer).  The
// old kernel split every value once per wave that used it (4 times at 256 x 256).  Same products in
// the same order per accumulator and the same column-sum order: bitwise the old kernel's partials.
constexpr int kTsLdsCols = 384;   // A columns of the block + N
__global__ __launch_bounds__(512) void tsgemm_bf_lds_kernel(const float* __restrict__ A, int lda,
                                                            const float* __restrict__ B, int ldb, int64_t n_rows,
                                                            int M, int N, int ones, int64_t chunk, int mtb,
                                                            float* __restrict__ part) {
  constexpr int NTH = 512, KP = (kTsLdsCols * 4 + NTH - 1) / NTH;
  __shared__ u4v sp[2 * 3 * kTsLdsCols * 4];   // two buffers of [piece][column][row group]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int tiles_n = N / 64, AC = 64 * mtb, COLS = AC + N;
  const int mg0 = blockIdx.y * AC;   // the block's first A column
  const int mt = wave / tiles_n, nt = wave % tiles_n;
  const bool tile_ok = mt < mtb && mg0 + 64 * mt < M;
  const bool sums = ones && blockIdx.y == 0;
  const int64_t r0 = (int64_t)blockIdx.x * chunk;
  const int64_t r1 = std::min<int64_t>(n_rows, r0 + chunk);
  // the thread's (column, row group) pairs: p = tid + NTH k, row group p / COLS, column p % COLS
  const float* src[KP];
  int64_t ld[KP];
  int gp[KP];
  bool pok[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const int p = tid + NTH * k;
    const int col = p % COLS;
    gp[k] = p / COLS;
    pok[k] = p < 4 * COLS && (col >= AC || mg0 + col < M);
    src[k] = col < AC ? A + (pok[k] ? mg0 + col : 0) : B + (col - AC);
    ld[k] = col < AC ? lda : ldb;
  }
  float v[KP][8];
  auto load = [&](int64_t r) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < KP; ++k)
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int64_t rr = r + 8 * gp[k] + jj;
        v[k][jj] = (pok[k] && rr < r1) ? src[k][rr * ld[k]] : 0.f;
      }
  };
  float cs[KP] = {};
  f4 acc[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = f4{0, 0, 0, 0};
  // split the loaded pairs into buffer bo's fragments (and the bias column sums)
  auto split_store = [&](u4v* bo) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const int p = tid + NTH * k;
      if (p >= 4 * COLS) continue;
      const int col = p % COLS;
      u4v w0, w1, w2;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float a0, a1, a2, b0, b1, b2;
        split3(v[k][2 * q], a0, a1, a2);
        split3(v[k][2 * q + 1], b0, b1, b2);
        w0[q] = pack_hi16(a0, b0);
        w1[q] = pack_hi16(a1, b1);
        w2[q] = pack_hi16(a2, b2);
      }
      bo[(0 * COLS + col) * 4 + gp[k]] = w0;
      bo[(1 * COLS + col) * 4 + gp[k]] = w1;
      bo[(2 * COLS + col) * 4 + gp[k]] = w2;
      if (sums && col >= AC) {
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) cs[k] += v[k][jj];
      }
    }
  };
  auto contract = [&](const u4v* bi) __attribute__((always_inline)) {
    if (!tile_ok) return;
    const int ac = 64 * mt + c, bc = AC + 64 * nt + c;
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      bf8 bp[3];
#pragma unroll
      for (int pb = 0; pb < 3; ++pb) bp[pb] = __builtin_bit_cast(bf8, bi[(pb * COLS + bc + 16 * y) * 4 + g]);
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        bf8 ap[3];
#pragma unroll
        for (int pa = 0; pa < 3; ++pa) ap[pa] = __builtin_bit_cast(bf8, bi[(pa * COLS + ac + 16 * x) * 4 + g]);
#pragma unroll
        for (int pa = 2; pa >= 0; --pa)
#pragma unroll
          for (int pb = 2 - pa; pb >= 0; --pb) acc[x][y] = MFMA_BF(ap[pa], bp[pb], acc[x][y]);
      }
    }
  };
  // two buffers, one barrier per step: step s+1's pieces are split while step s's MFMAs run
  if (r0 < r1) {
    load(r0);
    split_store(sp);
  }
  __syncthreads();
  int cur = 0;
  for (int64_t r = r0; r < r1; r += 32) {
    const bool more = r + 32 < r1;
    if (more) load(r + 32);
    contract(sp + cur * (3 * kTsLdsCols * 4));
    if (more) split_store(sp + (cur ^ 1) * (3 * kTsLdsCols * 4));
    __syncthreads();
    cur ^= 1;
  }
  const int Mx = M + ones;
  float* P = part + (int64_t)blockIdx.x * Mx * N;
  if (tile_ok) {
    const int m0 = mg0 + 64 * mt, n0 = 64 * nt;
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int q = 0; q < 4; ++q) P[(int64_t)(m0 + 16 * x + 4 * g + q) * N + n0 + 16 * y + c] = acc[x][y][q];
  }
  if (sums) {   // (s0 + s1) + (s2 + s3) over the four row groups, as the old kernel's two shuffles
    float* cl = reinterpret_cast<float*>(sp);
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const int p = tid + NTH * k;
      const int col = p % COLS;
      if (p < 4 * COLS && col >= AC) cl[(col - AC) * 4 + gp[k]] = cs[k];
    }
    __syncthreads();
    for (int n = tid; n < N; n += NTH) P[(int64_t)M * N + n] = (cl[4 * n] + cl[4 * n + 1]) + (cl[4 * n + 2] + cl[4 * n + 3]);
  }
}

// ---------------------------------------------------------------------------------------------
// Fused readout MLP on the bf16 matrix path, fp32-exact operands (device_common.h, split-bf16):
// y = act2(act1(X W1 + b1) W2 + b2) . w3 + b3 with every contraction formed from exact 3-piece
// bf16 splits of both operands (PASSES = 6 or 9 piece products, fp32 accumulation).
// Weights: pack_dense_bf16 fragments (output tile u, k-step s, piece p), 1 KB each; a 16-unit
// chunk of W2 is contiguous (24 KB), staged through LDS per workgroup, double-buffered.  W1 (DIN
// = 32: 48 KB) stays in LDS for the block.  One wave = 16 rows: the layer-1 activations are
// split once into 3 x 8 B fragments (96 VGPRs, accumulator layout = chained k order) and feed
// all 16 chunks; layer 2 is contracted with w3 per chunk and never stored.
// trans: the packed matrix is W^T of a row-major W [OUT][IN] (element (k, n) = W[n][k])
__global__ void pack_dense_bf16_kernel(const float* __restrict__ W, uint16_t* __restrict__ out, int IN, int OUT,
                                       int chained, int trans) {
  const int KS = IN / 32;
  const int64_t total = (int64_t)(OUT / 16) * KS * 3 * 512;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(e & 7), lane = (int)((e >> 3) & 63);
    int64_t f = e >> 9;                       // (u * KS + s) * 3 + piece
    const int piece = (int)(f % 3); f /= 3;
    const int s = (int)(f % KS);
    const int u = (int)(f / KS);
    const int g = lane >> 4;
    const int k = chained ? 16 * (2 * s + (j >> 2)) + 4 * g + (j & 3) : 32 * s + 8 * g + j;
    float p[3];
    const int n = 16 * u + (lane & 15);
    split3(trans ? W[(int64_t)n * IN + k] : W[(int64_t)k * OUT + n], p[0], p[1], p[2]);
    out[e] = (uint16_t)(__float_as_uint(p[piece]) >> 16);
  }
}

// the three B fragments of 8 consecutive values v[0..7] (element j = v[j])
__device__ __forceinline__ void split_frag(const float (&v)[8], bf8 (&f)[3]) {
  u4v w0, w1, w2;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float a0, a1, a2, b0, b1, b2;
    split3(v[2 * q], a0, a1, a2);
    split3(v[2 * q + 1], b0, b1, b2);
    w0[q] = pack_hi16(a0, b0);
    w1[q] = pack_hi16(a1, b1);
    w2[q] = pack_hi16(a2, b2);
  }
  f[0] = __builtin_bit_cast(bf8, w0);
  f[1] = __builtin_bit_cast(bf8, w1);
  f[2] = __builtin_bit_cast(bf8, w2);
}

// acc += sum over piece pairs (A piece pu, B piece ph) of A_pu . B_ph, small products first
template <int PASSES>
__device__ __forceinline__ f4 split_mfma(const bf8* __restrict__ afrag, int stride, const bf8 (&b)[3], f4 acc) {
#pragma unroll
  for (int pu = 2; pu >= 0; --pu) {
    const bf8 w = afrag[pu * stride];
#pragma unroll
    for (int ph = 2; ph >= 0; --ph) {
      if (PASSES == 6 && pu + ph > 2) continue;
      acc = MFMA_BF(w, b[ph], acc);
    }
  }
  return acc;
}

// acc[t] += A . B_t for RT row tiles that share each A (weight) fragment read; b = hf[t][s]
template <int PASSES, int RT, int KS>
__device__ __forceinline__ void split_mfma_rt(const bf8* __restrict__ afrag, int stride, const bf8 (&b)[RT][KS][3],
                                              int s, f4 (&acc)[RT]) {
  bf8 w[3];
#pragma unroll
  for (int pu = 0; pu < 3; ++pu) w[pu] = afrag[pu * stride];
  // the row tiles innermost: consecutive MFMAs accumulate into different tiles (a dependent
  // MFMA waits for the previous one's result)
#pragma unroll
  for (int pu = 2; pu >= 0; --pu)
#pragma unroll
    for (int ph = 2; ph >= 0; --ph) {
      if (PASSES == 6 && pu + ph > 2) continue;
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = MFMA_BF(w[pu], b[t][s][ph], acc[t]);
    }
}

template <int DIN, int ACT, int WAVES, int PASSES, int CT, bool W1L = (DIN == 32), int RT = 1, bool PERSIST = false>
__global__ __launch_bounds__(64 * WAVES) void readout_bf_kernel(Readout3Args a, const bf8* __restrict__ W1f,
                                                                 const bf8* __restrict__ W2f) {
  constexpr int N1 = 256, U1 = N1 / 16, U2 = 256 / 16;
  constexpr int KS1 = DIN / 32, KS2 = N1 / 32;
  constexpr int NTH = 64 * WAVES;
  constexpr int CHF = CT * KS2 * 3 * 64;         // bf8 per W2 chunk of CT output tiles (24 KB each)
  constexpr int NCH = U2 / CT;
  constexpr bool W1_LDS = W1L;   // W1 pieces in LDS (DIN 32) or read from L2 per wave
  constexpr int W1F = W1_LDS ? U1 * KS1 * 3 * 64 : 1;
  static_assert(CT == 1 && CHF % NTH == 0, "chunk layout: one 16-unit tile, whole 1 KB pieces per wave");
  __shared__ bf8 sw2[2][CHF];
  __shared__ bf8 sw1[W1F];
  __shared__ f4 sbias[3 * 64];   // b1 | b2 | w3 (256 floats each): LDS reads, no vmcnt waits in the loops
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
  const int j = lane & 15, g = lane >> 4;
  const u4v* W2v = reinterpret_cast<const u4v*>(W2f);
  if constexpr (W1_LDS) {
    const u4v* W1v = reinterpret_cast<const u4v*>(W1f);
    for (int i = tid; i < W1F; i += NTH) reinterpret_cast<u4v*>(sw1)[i] = W1v[i];
  }
  for (int i = tid; i < CHF; i += NTH) reinterpret_cast<u4v*>(sw2[0])[i] = W2v[i];
  for (int i = tid; i < 3 * 64; i += NTH) sbias[i] = ld4((i < 64 ? a.b1 : i < 128 ? a.b2 : a.w3) + 4 * (i & 63));
  // PERSIST: the block loops over row groups with W1 staged once; the chunk loop's wrap-around
  // prefetch leaves chunk 0 in sw2[0] for the next group
  const int64_t n_groups = (a.n_rows + 16 * RT * WAVES - 1) / (16 * RT * WAVES);
  for (int64_t grp = blockIdx.x; grp < n_groups; grp += PERSIST ? (int64_t)gridDim.x : n_groups) {
  // RT row tiles of 16 per wave: tile t covers rows r0 + 16t .. +16
  const int64_t r0 = (grp * WAVES + wave) * (16 * RT) + j;
  // layer-1 input fragments: lane (row j, group g) holds x[row][32s + 8g .. +8) (natural k order)
  bf8 xf[RT][KS1][3];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int64_t r = r0 + 16 * t;
    const bool ok = r < a.n_rows;
    const float* xr = a.x + (ok ? r : 0) * (int64_t)a.x_stride;
#pragma unroll
    for (int s = 0; s < KS1; ++s) {
      const f4 lo = ok ? ld4(xr + 32 * s + 8 * g) : f4{0, 0, 0, 0};
      const f4 hi = ok ? ld4(xr + 32 * s + 8 * g + 4) : f4{0, 0, 0, 0};
      const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      split_frag(v, xf[t][s]);
    }
  }
  __syncthreads();
  // layer 1 -> activations in accumulator layout -> split once into the layer-2 B fragments
  bf8 hf[RT][KS2][3];
#pragma unroll
  for (int s2 = 0; s2 < KS2; ++s2) {
    float v[RT][8];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int u = 2 * s2 + half;
      f4 acc[RT];
      const f4 bias = sbias[4 * u + g];
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = bias;
#pragma unroll
      for (int s = 0; s < KS1; ++s) {
        const bf8* af = W1_LDS ? sw1 + ((u * KS1 + s) * 3) * 64 + lane : W1f + ((u * KS1 + s) * 3) * 64 + lane;
        split_mfma_rt<PASSES, RT, KS1>(af, 64, xf, s, acc);
      }
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) v[t][4 * half + q] = act_t<ACT>(acc[t][q]);
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) split_frag(v[t], hf[t][s2]);
  }
  float y[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) y[t] = 0.f;
#pragma unroll 1
  for (int v = 0; v < NCH; ++v) {
    const int cur = v & 1;
    const f4 b = sbias[64 + 4 * v + g];
    const int nv = (v + 1) % NCH;
    // chunk v+1 goes straight into the other buffer by LDS-DMA (its readers passed the previous
    // barrier).  Issued as asm: the compiler cannot tell the DMA's target from the buffer read
    // below and would hold every ds_read of this chunk behind vmcnt(0), i.e. behind the DMA.  M0
    // (the DMA's LDS base) has no other user in this kernel (checked in the ISA).
#pragma unroll
    for (int k = 0; k < CHF / NTH; ++k) {
      const int piece = wave + WAVES * k;   // 1 KB pieces, one per wave and k
      const uint32_t m0 = __builtin_amdgcn_readfirstlane(
          (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(sw2[cur ^ 1] + piece * 64));
      const u4v* src = W2v + (int64_t)nv * CHF + piece * 64 + lane;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"   // M0 is reserved: see above and tests/test_isa.py
      asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(m0) : "memory", "m0");
#pragma clang diagnostic pop
    }
    __builtin_amdgcn_sched_barrier(0);
    // opaque lane offset: the LDS reads must not be hoisted out of the chunk loop (registers)
    int lofs = lane;
    asm volatile("" : "+v"(lofs));
    const bf8* wbase = sw2[cur] + lofs;
    f4 acc[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[t] = b;
    // the three weight pieces of k-step s+1 are read while k-step s's MFMAs run
    bf8 wn[3];
#pragma unroll
    for (int pu = 0; pu < 3; ++pu) wn[pu] = wbase[pu * 64];
#pragma unroll
    for (int s = 0; s < KS2; ++s) {
      bf8 w[3];
#pragma unroll
      for (int pu = 0; pu < 3; ++pu) w[pu] = wn[pu];
      if (s + 1 < KS2) {
#pragma unroll
        for (int pu = 0; pu < 3; ++pu) wn[pu] = wbase[((s + 1) * 3 + pu) * 64];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int pu = 2; pu >= 0; --pu)
#pragma unroll
        for (int ph = 2; ph >= 0; --ph) {
          if (PASSES == 6 && pu + ph > 2) continue;
#pragma unroll
          for (int t = 0; t < RT; ++t) acc[t] = MFMA_BF(w[pu], hf[t][s][ph], acc[t]);
        }
      __builtin_amdgcn_sched_barrier(0);
    }
    const f4 w3 = sbias[128 + 4 * v + g];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) y[t] += w3[q] * act_t<ACT>(acc[t][q]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the DMA has landed (for every wave: barrier)
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    float yt = y[t];
    yt += __shfl_xor(yt, 16);
    yt += __shfl_xor(yt, 32);
    const int64_t r = r0 + 16 * t;
    if (g == 0 && r < a.n_rows) {
      const float b3 = a.b3 ? a.b3[0] : 0.f;
      a.y[r] = act_apply_base(yt + b3, a.act3);
    }
  }
  }  // row groups
}


// ---------------------------------------------------------------------------------------------
// Readout variant 4: readout_bf with both layers on scaled two-piece fp16 operands
// (device_common.h split2h, 3 products on v_mfma_f32_16x16x32_f16) instead of x6 bf16.
// Scales (powers of two, exact):
// - W1 by sigma1, W2 by sigma2 = 2^(15 - E(max |W|)) at pack time (pack_readout_h16_kernel);
// - the layer-1 input of row tile t by S1_t = 2^(15 - E(mx_t)), mx_t = the tile's max |x|;
// - the layer-2 input of row tile t by S_t, from an a-priori bound on the layer-1 activations:
//   |W1^T x + b1| <= A mx_t + B (A = max_u sum_k |W1[k][u]|, B = max |b1|, mx_t = the tile's
//   max |x|), and |act(z)| <= 1.0508 |z| + 1.7582 for linear / relu / selu / tanh / sigmoid,
//   so |S_t act(z)| < 2^15 (no fp16 overflow) whatever the input scale.
// The scales are applied where they are free: layer 1 accumulates S1_t sigma1 (W1^T x + b1) (the
// bias seeds the accumulator times S1_t sigma1), and the activation maps that scale to S_t
// (act_scaled); layer 2 accumulates S_t sigma2 (W2^T a + b2), its activation and the w3 dot
// product run on that scale and the row's output is unscaled once.
// Packed buffer: [W2 pieces (chained k) | 64-float header: e(sigma2), A, B | W1 pieces (natural
// k) | 64-float header: e(sigma1)]; floats: N1 N2 + 64 + IN1 N1 + 64.
// Scales of the packed buffer (one block): headers after the W2 and W1 pieces.  The pieces
// themselves are written by pack_readout_h16_frag_kernel over a full grid (the repack after every
// optimizer step must stay cheap).
__global__ __launch_bounds__(1024) void pack_readout_h16_kernel(const float* __restrict__ W1, const float* __restrict__ b1,
                                                               const float* __restrict__ W2, uint16_t* __restrict__ out,
                                                               int IN1, int N1, int N2) {
  __shared__ float red[4][1024];
  float m2 = 0.f, a1 = 0.f, bb = 0.f, m1 = 0.f;
  for (int e = threadIdx.x; e < N1 * N2; e += blockDim.x) m2 = fmaxf(m2, fabsf(W2[e]));
  for (int e = threadIdx.x; e < IN1 * N1; e += blockDim.x) m1 = fmaxf(m1, fabsf(W1[e]));
  for (int u = threadIdx.x; u < N1; u += blockDim.x) {
    float l1 = 0.f;
    for (int k = 0; k < IN1; ++k) l1 += fabsf(W1[(int64_t)k * N1 + u]);
    a1 = fmaxf(a1, l1);
    if (b1) bb = fmaxf(bb, fabsf(b1[u]));
  }
  red[0][threadIdx.x] = m2;
  red[1][threadIdx.x] = a1;
  red[2][threadIdx.x] = bb;
  red[3][threadIdx.x] = m1;
  __syncthreads();
  for (int o = blockDim.x / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int q = 0; q < 4; ++q) red[q][threadIdx.x] = fmaxf(red[q][threadIdx.x], red[q][threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    m2 = red[0][0];
    m1 = red[3][0];
    const int es2 = m2 > 0.f ? min(100, max(-100, 15 - ((__float_as_int(m2) >> 23) - 126))) : 0;
    const int es1 = m1 > 0.f ? min(60, max(-60, 15 - ((__float_as_int(m1) >> 23) - 126))) : 0;
    const int64_t total2 = (int64_t)N1 * N2 * 2;   // halves of the W2 pieces
    int* hdr = reinterpret_cast<int*>(out + total2);
    hdr[0] = es2;
    hdr[1] = __float_as_int(red[1][0] * 1.001f);   // A, rounded up
    hdr[2] = __float_as_int(red[2][0] * 1.001f);   // B
    reinterpret_cast<int*>(out + total2 + 128 + (int64_t)IN1 * N1 * 2)[0] = es1;
  }
}

// W2 pieces (chained k order, as readout_bf's layer 2) and W1 pieces (natural k order: layer 1
// reads its input rows from memory), each scaled by its header's power of two
__global__ __launch_bounds__(256) void pack_readout_h16_frag_kernel(const float* __restrict__ W1,
                                                                    const float* __restrict__ W2,
                                                                    uint16_t* __restrict__ out, int IN1, int N1,
                                                                    int N2) {
  const int64_t total2 = (int64_t)N1 * N2 * 2, total1 = (int64_t)IN1 * N1 * 2;
  uint16_t* o1 = out + total2 + 128;
  const float sigma2 = __int_as_float((127 + reinterpret_cast<const int*>(out + total2)[0]) << 23);
  const float sigma1 = __int_as_float((127 + reinterpret_cast<const int*>(o1 + total1)[0]) << 23);
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total2 + total1;
       e += (int64_t)gridDim.x * blockDim.x) {
    const bool l2 = e < total2;
    const int64_t ee = l2 ? e : e - total2;
    const int jj = (int)(ee & 7), lane = (int)((ee >> 3) & 63);
    int64_t f = ee >> 9;                       // (u * KS + s) * 2 + piece
    const int piece = (int)(f & 1); f >>= 1;
    const int KS = (l2 ? N1 : IN1) / 32;
    const int s = (int)(f % KS);
    const int u = (int)(f / KS);
    const int k = l2 ? 16 * (2 * s + (jj >> 2)) + 4 * (lane >> 4) + (jj & 3) : 32 * s + 8 * (lane >> 4) + jj;
    const float v = l2 ? sigma2 * W2[(int64_t)k * N2 + 16 * u + (lane & 15)]
                       : sigma1 * W1[(int64_t)k * N1 + 16 * u + (lane & 15)];
    const _Float16 hi = (_Float16)v;
    const _Float16 pc = piece == 0 ? hi : (_Float16)(v - (float)hi);
    (l2 ? out : o1)[ee] = __builtin_bit_cast(uint16_t, pc);
  }
}

// So act(zs c) for zs = z / c (c, So powers of two), at the cost of act(z) for selu:
// k = So c (lambda So c for selu), cl = c log2(e), laS = lambda alpha So
template <int ACT>
__device__ __forceinline__ float act_scaled(float zs, float c, float k, float cl, float laS, float So) {
  if constexpr (ACT == IGN_K_ACT_RELU) return zs > 0.f ? zs * k : 0.f;
  else if constexpr (ACT == IGN_K_ACT_SELU) {
    // zs > 0: e = 1, so the negative arm is laS - laS = 0 and k max(zs, 0) + 0 = k zs; zs <= 0:
    // k max(zs, 0) = 0.  The same bits as the select, without the compare and the select
    // min / max as v_med3_f32 clamps: fminf / fmaxf would first canonicalise the MFMA result
    // (an extra v_max_f32 x, x, x each, IEEE mode); the clamp bounds are never reached
    const float e = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f(zs, -3.0e38f, 0.f) * cl);
    return fmaf(k, __builtin_amdgcn_fmed3f(zs, 0.f, 3.0e38f), fmaf(laS, e, -laS));
  } else if constexpr (ACT == IGN_K_ACT_LINEAR) return zs * k;
  else return So * act_t<ACT>(zs * c);
}

// SAVE (the training forward): the layer-1 and layer-2 activations are also written (a.save1,
// a.save2; the unscaled values the layers used, 16 B per lane per 16-unit tile) for the backward
template <int DIN, int ACT, int WAVES, int RT, bool SAVE = false>
__global__ __launch_bounds__(64 * WAVES) void readout_h16_kernel(Readout3Args a, const h8* __restrict__ W2f) {
  constexpr int N1 = 256, U1 = N1 / 16, U2 = 256 / 16;
  constexpr int KS1 = DIN / 32, KS2 = N1 / 32;
  constexpr int NTH = 64 * WAVES;
  constexpr int CHF = KS2 * 2 * 64;              // h8 per W2 chunk of one 16-unit tile (16 KB)
  constexpr int NCH = U2;
  constexpr int W1F = U1 * KS1 * 2 * 64;
  static_assert(CHF % NTH == 0, "chunk layout: whole 1 KB pieces per wave");
  constexpr float LAM = 1.0507009873554805f, LA = LAM * 1.6732632423543772f, LOG2E = 1.4426950408889634f;
  __shared__ h8 sw2[2][CHF];
  __shared__ h8 sw1[W1F];
  __shared__ f4 sbias[3 * 64];   // b1 | b2 | w3
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
  const int j = lane & 15, g = lane >> 4;
  const u4v* W2v = reinterpret_cast<const u4v*>(W2f);
  const h8* W1f = reinterpret_cast<const h8*>(reinterpret_cast<const float*>(W2f) + N1 * 256 + 64);
  {
    const u4v* W1v = reinterpret_cast<const u4v*>(W1f);
    for (int i = tid; i < W1F; i += NTH) reinterpret_cast<u4v*>(sw1)[i] = W1v[i];
  }
  const int es1 = reinterpret_cast<const int*>(W1f + W1F)[0];
  for (int i = tid; i < CHF; i += NTH) reinterpret_cast<u4v*>(sw2[0])[i] = W2v[i];
  for (int i = tid; i < 3 * 64; i += NTH) sbias[i] = ld4((i < 64 ? a.b1 : i < 128 ? a.b2 : a.w3) + 4 * (i & 63));
  const int* hdr = reinterpret_cast<const int*>(W2f + (int64_t)NCH * CHF);
  const int es2 = hdr[0];
  const float A1 = __int_as_float(hdr[1]), B1 = __int_as_float(hdr[2]);
  const int64_t n_groups = (a.n_rows + 16 * RT * WAVES - 1) / (16 * RT * WAVES);
  // the layer-1 input rows of a row group (out-of-range rows read as zeros)
  f4 xl[RT][KS1][2];
  auto load_x = [&](int64_t grp) __attribute__((always_inline)) {
    const int64_t rr = (grp * WAVES + wave) * (16 * RT) + j;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int64_t r = rr + 16 * t;
      const bool ok = r < a.n_rows;
      const float* xr = a.x + (ok ? r : 0) * (int64_t)a.x_stride;
#pragma unroll
      for (int s = 0; s < KS1; ++s) {
        xl[t][s][0] = ok ? ld4(xr + 32 * s + 8 * g) : f4{0, 0, 0, 0};
        xl[t][s][1] = ok ? ld4(xr + 32 * s + 8 * g + 4) : f4{0, 0, 0, 0};
      }
    }
  };
  load_x(blockIdx.x);
  for (int64_t grp = blockIdx.x; grp < n_groups; grp += (int64_t)gridDim.x) {
  const int64_t r0 = (grp * WAVES + wave) * (16 * RT) + j;
  // per row tile: its max |x| and the scales derived from it (xl: loaded during the previous group).
  // The max is floored at 1 (as the ordered update's tile scale): every tile whose inputs lie in
  // [-1, 1] gets the same scales, so a row's bits do not depend on which rows share its tile (the
  // batch composition, an edge-cut partition's first row)
  float mx[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    mx[t] = 1.f;
#pragma unroll
    for (int s = 0; s < KS1; ++s)
#pragma unroll
      for (int q = 0; q < 4; ++q) mx[t] = fmaxf(mx[t], fmaxf(fabsf(xl[t][s][0][q]), fabsf(xl[t][s][1][q])));
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) mx[t] = wave_max_nonneg(mx[t]);
  float S[RT], S1S[RT], c1[RT], SS[RT], cSS[RT];
  h8 xf[RT][KS1][2];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const float bnd = fmaf(fmaf(A1, mx[t], B1), 1.0508f, 1.7582f);
    const int E = (__builtin_amdgcn_readfirstlane(__float_as_int(bnd)) >> 23) - 126;   // bnd < 2^E
    const int eS = 15 - E;
    S[t] = __int_as_float((127 + eS) << 23);
    SS[t] = __int_as_float((127 + eS + es2) << 23);
    cSS[t] = __int_as_float((127 - eS - es2) << 23);
    // layer-1 input scale: S1 = 2^(15 - E(mx)), |x S1| < 2^15
    const int E1 = (__builtin_amdgcn_readfirstlane(__float_as_int(fmaxf(mx[t], 1e-18f))) >> 23) - 126;
    const int eS1 = min(60, max(-60, 15 - E1));
    const float S1 = __int_as_float((127 + eS1) << 23);
    S1S[t] = __int_as_float((127 + eS1 + es1) << 23);
    c1[t] = __int_as_float((127 - eS1 - es1) << 23);
#pragma unroll
    for (int s = 0; s < KS1; ++s) {
      const f4 lo = xl[t][s][0] * S1, hi = xl[t][s][1] * S1;
      const hpair p0 = split2h(lo[0], lo[1]), p1 = split2h(lo[2], lo[3]);
      const hpair p2 = split2h(hi[0], hi[1]), p3 = split2h(hi[2], hi[3]);
      const u4v w0 = {p0.hi, p1.hi, p2.hi, p3.hi}, w1 = {p0.lo, p1.lo, p2.lo, p3.lo};
      xf[t][s][0] = __builtin_bit_cast(h8, w0);
      xf[t][s][1] = __builtin_bit_cast(h8, w1);
    }
  }
#ifndef IGN_RO_NOPREFETCH
  // the next row group's input rows load during this group's two layers (xl is dead from here on);
  // without it every group opened with an exposed global-load round trip
  if (grp + gridDim.x < n_groups) load_x(grp + gridDim.x);
#endif
  __syncthreads();
  // layer 1 (x3 fp16) -> S_t act(z) in accumulator layout -> the layer-2 fp16 B fragments
  h8 hf[RT][KS2][2];
#pragma unroll
  for (int s2 = 0; s2 < KS2; ++s2) {
    float v[RT][8];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int u = 2 * s2 + half;
      f4 acc[RT];
      const f4 bias = sbias[4 * u + g];
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = bias * S1S[t];
#pragma unroll
      for (int s = 0; s < KS1; ++s) {
        const h8 w1 = sw1[((u * KS1 + s) * 2 + 1) * 64 + lane];
        const h8 w0 = sw1[((u * KS1 + s) * 2 + 0) * 64 + lane];
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t] = MFMA_H(w1, xf[t][s][0], acc[t]);
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t] = MFMA_H(w0, xf[t][s][1], acc[t]);
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t] = MFMA_H(w0, xf[t][s][0], acc[t]);
      }
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const float k = (ACT == IGN_K_ACT_SELU ? LAM : 1.0f) * S[t] * c1[t];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          v[t][4 * half + q] = act_scaled<ACT>(acc[t][q], c1[t], k, c1[t] * LOG2E, LA * S[t], S[t]);
        if constexpr (SAVE) {
          const int64_t r = r0 + 16 * t;
          const float iS = __int_as_float(254 - ((__float_as_int(S[t]) >> 23) & 255) << 23);   // 1 / S, exact
          if (r < a.n_rows)
            st4(a.save1 + r * N1 + 16 * u + 4 * g,
                f4{v[t][4 * half], v[t][4 * half + 1], v[t][4 * half + 2], v[t][4 * half + 3]} * iS);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      u4v w0, w1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const hpair p = split2h(v[t][2 * q], v[t][2 * q + 1]);
        w0[q] = p.hi;
        w1[q] = p.lo;
      }
      hf[t][s2][0] = __builtin_bit_cast(h8, w0);
      hf[t][s2][1] = __builtin_bit_cast(h8, w1);
    }
  }
  float y[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) y[t] = 0.f;
#pragma unroll 1
  for (int v = 0; v < NCH; ++v) {
    const int cur = v & 1;
    const f4 b = sbias[64 + 4 * v + g];
    const int nv = (v + 1) % NCH;
    // chunk v+1 by LDS-DMA into the other buffer (readout_bf_kernel: why asm, and M0)
#pragma unroll
    for (int k = 0; k < CHF / NTH; ++k) {
      const int piece = wave + WAVES * k;
      const uint32_t m0 = __builtin_amdgcn_readfirstlane(
          (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(sw2[cur ^ 1] + piece * 64));
      const u4v* src = W2v + (int64_t)nv * CHF + piece * 64 + lane;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
#ifndef IGN_RO_ABL_NODMA   // timing ablation (wrong results): every chunk reuses chunk 0
      asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(m0) : "memory", "m0");
#else
      (void)src; (void)m0;
#endif
#pragma clang diagnostic pop
    }
    __builtin_amdgcn_sched_barrier(0);
    int lofs = lane;
    asm volatile("" : "+v"(lofs));
    const h8* wbase = sw2[cur] + lofs;
    f4 acc[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[t] = b * SS[t];
    h8 wn[2];
#pragma unroll
    for (int pu = 0; pu < 2; ++pu) wn[pu] = wbase[pu * 64];
#pragma unroll
    for (int s = 0; s < KS2; ++s) {
      h8 w[2];
#pragma unroll
      for (int pu = 0; pu < 2; ++pu) w[pu] = wn[pu];
      if (s + 1 < KS2) {
#pragma unroll
        for (int pu = 0; pu < 2; ++pu) wn[pu] = wbase[((s + 1) * 2 + pu) * 64];
      }
      __builtin_amdgcn_sched_barrier(0);
      // W2 lo x a hi, W2 hi x {a lo, a hi}
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = MFMA_H(w[1], hf[t][s][0], acc[t]);
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = MFMA_H(w[0], hf[t][s][1], acc[t]);
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = MFMA_H(w[0], hf[t][s][0], acc[t]);
      __builtin_amdgcn_sched_barrier(0);
    }
    const f4 w3 = sbias[128 + 4 * v + g];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      f4 av;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        av[q] = act_scaled<ACT>(acc[t][q], cSS[t], ACT == IGN_K_ACT_SELU ? LAM : 1.0f, cSS[t] * LOG2E, LA * SS[t],
                                SS[t]);
        // an explicit fma: a contractable multiply-add may be lowered fused for one row tile and
        // unfused for the other (it was, in the SAVE form), which made a row's bits depend on its tile
        y[t] = fmaf(w3[q], av[q], y[t]);
      }
      if constexpr (SAVE) {
        const int64_t r = r0 + 16 * t;
        if (r < a.n_rows) st4(a.save2 + r * 256 + 16 * v + 4 * g, av * cSS[t]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the DMA has landed (for every wave: barrier)
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    float yt = y[t];
    yt += __shfl_xor(yt, 16);
    yt += __shfl_xor(yt, 32);
    const int64_t r = r0 + 16 * t;
    if (g == 0 && r < a.n_rows) {
      const float b3 = a.b3 ? a.b3[0] : 0.f;
      a.y[r] = act_apply_base(fmaf(yt, cSS[t], b3), a.act3);
    }
  }
#ifdef IGN_RO_NOPREFETCH
  if (grp + gridDim.x < n_groups) load_x(grp + gridDim.x);
#endif
  }  // row groups
}

// ---------------------------------------------------------------------------------------------
// Row GEMM y[r] = act(x[r] . W + b) on the split-bf16 path (the training forward's Dense layers,
// whose activations are kept for the backward).  readout_bf's layer-2 loop with the input read
// from memory: W (packed non-chained, natural k) is staged through LDS in groups of G 16-unit
// tiles (<= 24 KB), double-buffered; each wave owns two 16-row tiles whose input pieces stay in
// registers (K / 32 x 3 fragments per tile) and writes act(acc) as 16 B per lane.
// BWD: the backward row GEMM instead, y[r] (+)= (x[r] . W^T) * act'(aprev[r]) with W^T packed
// (row_gemm_t's contract; bias unused, ACT = the activation whose derivative is applied).
// xo (BWD only, optional): the input rows are the backward of a 1-unit output layer, formed on the
// fly: x[r][k] = (0 + xo.s[r] * xo.w[k]) * act'(x_raw[r][k]) with x_raw the layer's output
// activations (row_outer_t's arithmetic), and written to xo.out for the layer's weight gradient
// (xo.out may be x_raw itself: each element is read and then written by the same lane, once)
template <int KS, int G, int ACT, bool BWD = false, int NP = 3, int RTT = 2>
__global__ __launch_bounds__(512) void dense_bf_kernel(const float* x, int64_t n, int x_stride,
                                                       const void* __restrict__ Wf, const float* __restrict__ bias,
                                                       int M, float* __restrict__ y, const float* __restrict__ aprev,
                                                       int accumulate, OuterRows xo) {
  constexpr int WAVES = 8, RT = RTT, NTH = 64 * WAVES;
  // NP = 3: split-bf16 x6; NP = 2: scaled split-fp16 x3 (W pieces carry sigma = 2^es after the
  // fragments, each 16-row tile of x its own S = 2^(15 - E(max |x|)); DESIGN.md §3b')
  constexpr int CHF = G * KS * NP * 64;   // 16-B fragments per stage
  constexpr int PER = (CHF + NTH - 1) / NTH;
  __shared__ u4v sw[2][CHF];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
  const int j = lane & 15, g = lane >> 4;
  const u4v* Wv = reinterpret_cast<const u4v*>(Wf);
  const int NV = M / (16 * G);
  for (int i = tid; i < CHF; i += NTH) sw[0][i] = Wv[i];
  const int64_t r0 = ((int64_t)blockIdx.x * WAVES + wave) * (16 * RT) + j;
  bf8 xf[RT][KS][3];
  h8 xh[RT][KS][2];
  float cS[RT], KSig[RT];   // NP = 2: 1 / (S sigma) and S sigma per row tile
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int64_t r = r0 + 16 * t;
    const bool ok = r < n;
    const float* xr = x + (ok ? r : 0) * (int64_t)x_stride;
    const float xsr = BWD && xo.s && ok ? xo.s[r] : 0.f;
    // the input's 4 values at column c0 (raw, or formed from the output layer's gradient)
    auto ldx = [&](int c0) __attribute__((always_inline)) -> f4 {
      if (!ok) return f4{0, 0, 0, 0};
      const f4 v = ld4(xr + c0);
      if (!BWD || !xo.s) return v;
      const f4 w = ld4(xo.w + c0);
      f4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float sq = 0.f;
        sq += xsr * w[q];
        o[q] = sq * act_grad_out_base(v[q], xo.act);
      }
      if (xo.out) st4(xo.out + r * (int64_t)x_stride + c0, o);   // for the weight gradient (may be x itself)
      return o;
    };
    if constexpr (NP == 3) {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const f4 lo = ldx(32 * s + 8 * g);
        const f4 hi = ldx(32 * s + 8 * g + 4);
        const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        split_frag(v, xf[t][s]);
      }
    } else {
      f4 xv[KS][2];
      float mx = 1e-18f;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        xv[s][0] = ldx(32 * s + 8 * g);
        xv[s][1] = ldx(32 * s + 8 * g + 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) mx = fmaxf(mx, fmaxf(fabsf(xv[s][0][q]), fabsf(xv[s][1][q])));
      }
      mx = wave_max_nonneg(mx);
      const int es = reinterpret_cast<const int*>(Wv + (int64_t)(M / 16) * KS * 2 * 64)[0];
      const int eS = min(60, max(-60, 15 - ((__builtin_amdgcn_readfirstlane(__float_as_int(mx)) >> 23) - 126)));
      const float S = __int_as_float((127 + eS) << 23);
      KSig[t] = __int_as_float((127 + eS + es) << 23);
      cS[t] = __int_as_float((127 - eS - es) << 23);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const f4 lo = xv[s][0] * S, hi = xv[s][1] * S;
        const hpair p0 = split2h(lo[0], lo[1]), p1 = split2h(lo[2], lo[3]);
        const hpair p2 = split2h(hi[0], hi[1]), p3 = split2h(hi[2], hi[3]);
        const u4v w0 = {p0.hi, p1.hi, p2.hi, p3.hi}, w1 = {p0.lo, p1.lo, p2.lo, p3.lo};
        xh[t][s][0] = __builtin_bit_cast(h8, w0);
        xh[t][s][1] = __builtin_bit_cast(h8, w1);
      }
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int v = 0; v < NV; ++v) {
    const int cur = v & 1;
    const bool more = v + 1 < NV;
    u4v stage[PER];
    if (more) {
#pragma unroll
      for (int q = 0; q < PER; ++q) {
        const int i = tid + NTH * q;
        if (CHF % NTH == 0 || i < CHF) stage[q] = Wv[(int64_t)(v + 1) * CHF + i];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    int lofs = lane;   // opaque: keeps the LDS reads inside the loop
    asm volatile("" : "+v"(lofs));
#pragma unroll
    for (int c = 0; c < G; ++c) {
      const int u = v * G + c;
      const f4 b = bias ? ld4(bias + 16 * u + 4 * g) : f4{0, 0, 0, 0};
      f4 acc[RT];
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = NP == 3 ? b : b * KSig[t];
      if constexpr (NP == 3) {
#pragma unroll
        for (int s = 0; s < KS; ++s)
          split_mfma_rt<6, RT, KS>(reinterpret_cast<const bf8*>(sw[cur]) + (c * KS + s) * 3 * 64 + lofs, 64, xf, s, acc);
      } else {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const h8* wb = reinterpret_cast<const h8*>(sw[cur]) + (c * KS + s) * 2 * 64 + lofs;
          const h8 w0 = wb[0], w1 = wb[64];
#pragma unroll
          for (int t = 0; t < RT; ++t) acc[t] = MFMA_H(w1, xh[t][s][0], acc[t]);
#pragma unroll
          for (int t = 0; t < RT; ++t) acc[t] = MFMA_H(w0, xh[t][s][1], acc[t]);
#pragma unroll
          for (int t = 0; t < RT; ++t) acc[t] = MFMA_H(w0, xh[t][s][0], acc[t]);
        }
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t] *= cS[t];
      }
#pragma unroll
      for (int t = 0; t < RT; ++t) {
        const int64_t r = r0 + 16 * t;
        if (r >= n) continue;
        float* po = y + r * M + 16 * u + 4 * g;
        f4 o;
        if constexpr (BWD) {
          const f4 av = aprev ? ld4(aprev + r * M + 16 * u + 4 * g) : f4{0, 0, 0, 0};
#pragma unroll
          for (int q = 0; q < 4; ++q) o[q] = aprev ? acc[t][q] * act_grad_out_base(av[q], ACT) : acc[t][q];
          if (accumulate) o += ld4(po);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) o[q] = act_t<ACT>(acc[t][q]);
        }
        st4(po, o);
      }
    }
    if (more) {
#pragma unroll
      for (int q = 0; q < PER; ++q) {
        const int i = tid + NTH * q;
        if (CHF % NTH == 0 || i < CHF) sw[cur ^ 1][i] = stage[q];
      }
    }
    __syncthreads();
  }
}

hipError_t launch_seq_gru_bf(const SeqGruArgs& args, int h, int passes, hipStream_t st) {
  if (args.n_dst == 0) return hipSuccess;
  if (!args.Ubf || (h != 32 && h != 64) || passes != 6) return hipErrorInvalidValue;
  const int64_t work = grid_for(args.n_dst, 64);
#define SEQ_BF(HH, P)                                                                              \
  {                                                                                                \
    auto k = args.hs_save ? seq_gru_bf_kernel<HH, true, P> : seq_gru_bf_kernel<HH, false, P>;      \
    hipLaunchKernelGGL(k, dim3(persistent_grid(k, work)), dim3(256), 0, st, args);                \
  }
  if (h == 32) SEQ_BF(32, 6)
  else SEQ_BF(64, 6)
#undef SEQ_BF
  return hipGetLastError();
}

template <int DIN, int ACT, int WAVES, int PASSES, int CT, bool W1L, int RT, bool PERSIST>
static void readout_bf_launch(const Readout3Args& args, const bf8* w1, const bf8* w2, hipStream_t st) {
  auto k = readout_bf_kernel<DIN, ACT, WAVES, PASSES, CT, W1L, RT, PERSIST>;
  const int64_t groups = (args.n_rows + 16 * RT * WAVES - 1) / (16 * RT * WAVES);
  const int64_t grid = PERSIST ? persistent_grid(k, groups, 64 * WAVES) : groups;
  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(64 * WAVES), 0, st, args, w1, w2);
}

template <int DIN, int WAVES, int PASSES, int CT, bool W1L = (DIN == 32), int RT = 1, bool PERSIST = false>
static hipError_t readout_bf_din(const Readout3Args& args, const void* W1f, const void* W2f, hipStream_t st) {
  const bf8* w1 = static_cast<const bf8*>(W1f);
  const bf8* w2 = static_cast<const bf8*>(W2f);
  switch (args.act1) {
    case IGN_K_ACT_SELU: readout_bf_launch<DIN, IGN_K_ACT_SELU, WAVES, PASSES, CT, W1L, RT, PERSIST>(args, w1, w2, st); break;
    case IGN_K_ACT_RELU: readout_bf_launch<DIN, IGN_K_ACT_RELU, WAVES, PASSES, CT, W1L, RT, PERSIST>(args, w1, w2, st); break;
    case IGN_K_ACT_TANH: readout_bf_launch<DIN, IGN_K_ACT_TANH, WAVES, PASSES, CT, W1L, RT, PERSIST>(args, w1, w2, st); break;
    case IGN_K_ACT_SIGMOID: readout_bf_launch<DIN, IGN_K_ACT_SIGMOID, WAVES, PASSES, CT, W1L, RT, PERSIST>(args, w1, w2, st); break;
    case IGN_K_ACT_LINEAR: readout_bf_launch<DIN, IGN_K_ACT_LINEAR, WAVES, PASSES, CT, W1L, RT, PERSIST>(args, w1, w2, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_readout_bf(const Readout3Args& args, const void* W1f, const void* W2f, int din, int passes,
                             hipStream_t st) {
  if (args.n_rows == 0) return hipSuccess;
  if (!readout_bf_supported(din, 256, 256, args.act1, args.act2, args.act3) || !W1f || !W2f || passes != 6)
    return hipErrorInvalidValue;
  // split-bf16 x6 (the x9 form was dropped in round 3: no caller after the precision study): two 16-row tiles per wave sharing every W2 fragment read, 8-wave blocks
  // (246 VGPRs, 2 waves/SIMD): 1.03-1.05 ms against 1.13-1.16 ms for one tile per wave in 12-wave
  // blocks, 1.18 ms with 32-unit W2 chunks, 1.39-1.41 ms with 4-wave blocks (512 x synth50, round 1)
  // persistent blocks (W1 staged once per block, W2 chunk 0 carried over): 3.54-3.56 vs 3.58-3.59
  // ms/step on one box (tools/ab_env.sh, round 2)
  // W2 chunks by LDS-DMA + weight pieces read one k-step ahead: 1.025-1.031 vs 1.079-1.109 ms per
  // launch, 3.51 vs 3.58-3.59 ms/step (same box, round 2); b1/b2/w3 read from LDS (no vmcnt wait in the
  // loops, which would also have waited for the DMA): 0.983-0.989 vs 1.020-1.042 ms
  if (din == 32)
    return readout_bf_din<32, 8, 6, 1, true, 2, true>(args, W1f, W2f, st);
  // DIN 64 (the 1M-node graph): W1's pieces (96 KB) in LDS beside the W2 double buffer (48 KB),
  // persistent blocks: 5.01-5.02 vs 5.14-5.25 ms/step with W1 read from L2 per wave (round 2)
  return readout_bf_din<64, 8, 6, 1, true, 2, true>(args, W1f, W2f, st);
}


template <int DIN, int ACT>
static void readout_h16_launch(const Readout3Args& args, const h8* w, hipStream_t st) {
// 4 waves per block (1 per SIMD): two blocks per CU (VGPR-bound: 212 each) that do not share
// barriers, so one block's layer-1 / selu phase runs beside the other's layer-2 MFMAs
// (0.64 -> 0.59-0.61 ms per launch against 8 waves, same box)
#ifndef IGN_READOUT_WAVES
#define IGN_READOUT_WAVES 4
#endif
#ifndef IGN_READOUT_RT
#define IGN_READOUT_RT 2
#endif
  constexpr int WAVES = IGN_READOUT_WAVES, RT = IGN_READOUT_RT;   // RT = 1 (8 or 4 waves) measured slower: 0.59 / 0.69 ms
  auto k = args.save1 ? readout_h16_kernel<DIN, ACT, WAVES, RT, true> : readout_h16_kernel<DIN, ACT, WAVES, RT>;
  const int64_t groups = (args.n_rows + 16 * RT * WAVES - 1) / (16 * RT * WAVES);
  hipLaunchKernelGGL(k, dim3((unsigned)persistent_grid(k, groups, 64 * WAVES)), dim3(64 * WAVES), 0, st, args, w);
}

template <int DIN>
static hipError_t readout_h16_din(const Readout3Args& args, const h8* w, hipStream_t st) {
  switch (args.act1) {
    case IGN_K_ACT_SELU: readout_h16_launch<DIN, IGN_K_ACT_SELU>(args, w, st); break;
    case IGN_K_ACT_RELU: readout_h16_launch<DIN, IGN_K_ACT_RELU>(args, w, st); break;
    case IGN_K_ACT_TANH: readout_h16_launch<DIN, IGN_K_ACT_TANH>(args, w, st); break;
    case IGN_K_ACT_SIGMOID: readout_h16_launch<DIN, IGN_K_ACT_SIGMOID>(args, w, st); break;
    case IGN_K_ACT_LINEAR: readout_h16_launch<DIN, IGN_K_ACT_LINEAR>(args, w, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_readout_h16(const Readout3Args& args, const void* Wh, int din, hipStream_t st) {
  if (args.n_rows == 0) return hipSuccess;
  if (!readout_bf_supported(din, 256, 256, args.act1, args.act2, args.act3) || !Wh || !args.b1 || !args.b2 ||
      !args.save1 != !args.save2)
    return hipErrorInvalidValue;
  const h8* w = static_cast<const h8*>(Wh);
  return din == 32 ? readout_h16_din<32>(args, w, st) : readout_h16_din<64>(args, w, st);
}

// the variant-4 / variant-5 headers alone (readout_h32.hip packs its own pieces)
hipError_t launch_pack_readout_h16_header(const float* W1, const float* b1, const float* W2, void* out, int in1, int n1,
                                          int n2, hipStream_t st) {
  hipLaunchKernelGGL(pack_readout_h16_kernel, dim3(1), dim3(1024), 0, st, W1, b1, W2, static_cast<uint16_t*>(out), in1,
                     n1, n2);
  return hipGetLastError();
}

hipError_t launch_pack_readout_h16(const float* W1, const float* b1, const float* W2, void* out, int in1, int n1,
                                   int n2, hipStream_t st) {
  if (n1 != 256 || n2 != 256 || in1 % 32) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pack_readout_h16_kernel, dim3(1), dim3(1024), 0, st, W1, b1, W2, static_cast<uint16_t*>(out), in1,
                     n1, n2);
  hipLaunchKernelGGL(pack_readout_h16_frag_kernel, dim3(128), dim3(256), 0, st, W1, W2, static_cast<uint16_t*>(out), in1,
                     n1, n2);
  return hipGetLastError();
}

template <int KS, int G, bool BWD, int NP>
static hipError_t dense_bf_ks(const float* x, int64_t n, int x_stride, const void* W, const float* bias, int M, int act,
                              float* y, const float* aprev, int accumulate, OuterRows xo, hipStream_t st) {
  // K = 256 split-fp16 (the training readout's 256-wide layer, forward and backward): one 16-row tile
  // per wave, 110 VGPRs, so two blocks share a CU and one's loads and stores run under the other's
  // MFMAs (two tiles per wave: 196 VGPRs, one block per CU).  Each tile keeps its own scale: the same
  // bits.  1.58 -> 1.38 ms per backward launch, 17.62 -> 17.42 ms per training step (r05_c37.sh)
  constexpr int RT = (KS == 8 && NP == 2) ? 1 : 2;
  const dim3 grid((unsigned)((n + 128 * RT - 1) / (128 * RT))), block(512);
#define DBF(A) hipLaunchKernelGGL((dense_bf_kernel<KS, G, A, BWD, NP, RT>), grid, block, 0, st, x, n, x_stride, W, bias, M, y, aprev, accumulate, xo)
  switch (act) {
    case IGN_K_ACT_SELU: DBF(IGN_K_ACT_SELU); break;
    case IGN_K_ACT_RELU: DBF(IGN_K_ACT_RELU); break;
    case IGN_K_ACT_TANH: DBF(IGN_K_ACT_TANH); break;
    case IGN_K_ACT_SIGMOID: DBF(IGN_K_ACT_SIGMOID); break;
    case IGN_K_ACT_LINEAR: DBF(IGN_K_ACT_LINEAR); break;
    default:
      // The other five are instantiated for the split-fp16 forward alone (dense_stack.cpp takes another
      // kernel, or applies the derivative after, elsewhere: DESIGN.md §3f).  Never the identity in their place.
      if constexpr (BWD || NP != 2) return hipErrorInvalidValue;
      else switch (act) {
        case IGN_K_ACT_ELU: DBF(IGN_K_ACT_ELU); break;
        case IGN_K_ACT_SOFTPLUS: DBF(IGN_K_ACT_SOFTPLUS); break;
        case IGN_K_ACT_SOFTSIGN: DBF(IGN_K_ACT_SOFTSIGN); break;
        // (no exponential: lower_plan keeps such a plan off the scaled split-fp16 Dense kernels)
        case IGN_K_ACT_HARD_SIGMOID: DBF(IGN_K_ACT_HARD_SIGMOID); break;
        default: return hipErrorInvalidValue;
      }
  }
#undef DBF
  return hipGetLastError();
}

template <bool BWD, int NP = 3>
static hipError_t dense_bf_any(const float* x, int64_t n, int K, int x_stride, const void* W, const float* bias, int M,
                               int act, float* y, const float* aprev, int accumulate, hipStream_t st,
                               OuterRows xo = OuterRows{}) {
  // G 16-unit tiles of K x 16 x NP pieces per stage (M % 128 == 0: G divides M / 16).  NP = 2: 32 KB
  // stages, so each pass writes >= 128 B (whole lines) of every row: 0.949 -> 0.877 ms for the
  // 256-wide training readout layer, 19.9 -> 19.8 ms per step; NP = 3: <= 24 KB
  if constexpr (NP == 2) {
    switch (K) {
      case 32: return dense_bf_ks<1, 8, BWD, NP>(x, n, x_stride, W, bias, M, act, y, aprev, accumulate, xo, st);
      case 64: return dense_bf_ks<2, 8, BWD, NP>(x, n, x_stride, W, bias, M, act, y, aprev, accumulate, xo, st);
      case 128: return dense_bf_ks<4, 4, BWD, NP>(x, n, x_stride, W, bias, M, act, y, aprev, accumulate, xo, st);
      default: return dense_bf_ks<8, 2, BWD, NP>(x, n, x_stride, W, bias, M, act, y, aprev, accumulate, xo, st);
    }
  } else {   // (else: the other NP's stage sizes are not instantiated)
    switch (K) {
      case 32: return dense_bf_ks<1, 8, BWD, NP>(x, n, x_stride, W, bias, M, act, y, aprev, accumulate, xo, st);
      case 64: return dense_bf_ks<2, 4, BWD, NP>(x, n, x_stride, W, bias, M, act, y, aprev, accumulate, xo, st);
      case 128: return dense_bf_ks<4, 2, BWD, NP>(x, n, x_stride, W, bias, M, act, y, aprev, accumulate, xo, st);
      default: return dense_bf_ks<8, 1, BWD, NP>(x, n, x_stride, W, bias, M, act, y, aprev, accumulate, xo, st);
    }
  }
}

hipError_t launch_dense_bf(const float* x, int64_t n, int K, int x_stride, const void* Wbf, const float* bias, int M,
                           int act, float* y, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!dense_bf_supported(K, M) || x_stride % 4 || !Wbf) return hipErrorInvalidValue;
  return dense_bf_any<false>(x, n, K, x_stride, Wbf, bias, M, act, y, nullptr, 0, st);
}

hipError_t launch_dense_h16(const float* x, int64_t n, int K, int x_stride, const void* Wh, const float* bias, int M,
                            int act, float* y, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!dense_bf_supported(K, M) || x_stride % 4 || !Wh) return hipErrorInvalidValue;
  return dense_bf_any<false, 2>(x, n, K, x_stride, Wh, bias, M, act, y, nullptr, 0, st);
}

hipError_t launch_dense_h16_t(const float* dz, int64_t n, int K, const void* Wth, int M, float* out, int accumulate,
                              int act, const float* aprev, hipStream_t st, OuterRows xo) {
  if (n == 0) return hipSuccess;
  if (!dense_bf_supported(K, M) || !Wth || (xo.s && !act_first_five(xo.act))) return hipErrorInvalidValue;
  return dense_bf_any<true, 2>(dz, n, K, K, Wth, nullptr, M, act < 0 ? IGN_K_ACT_LINEAR : act, out,
                               act < 0 ? nullptr : aprev, accumulate, st, xo);
}

// Scaled fp16 pieces of a Dense kernel for dense_bf_kernel<.., NP = 2> (natural k; trans: of W^T),
// layout (u * KS + s) * 2 + piece, then sigma's exponent: one block for the scale, a grid for the pieces
__global__ __launch_bounds__(1024) void dense_f16_scale_kernel(const float* __restrict__ W, int64_t nel,
                                                               int* __restrict__ hdr) {
  __shared__ float red[1024];
  float m = 0.f;
  for (int64_t e = threadIdx.x; e < nel; e += blockDim.x) m = fmaxf(m, fabsf(W[e]));
  red[threadIdx.x] = m;
  __syncthreads();
  for (int o = blockDim.x / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0)
    hdr[0] = red[0] > 0.f ? min(60, max(-60, 15 - ((__float_as_int(red[0]) >> 23) - 126))) : 0;
}

__global__ void pack_dense_f16_kernel(const float* __restrict__ W, uint16_t* __restrict__ out, int IN, int OUT,
                                      int trans) {
  const int KS = IN / 32;
  const int64_t total = (int64_t)(OUT / 16) * KS * 2 * 512;
  const float sigma = __int_as_float((127 + reinterpret_cast<const int*>(out + total)[0]) << 23);
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int jj = (int)(e & 7), lane = (int)((e >> 3) & 63);
    int64_t f = e >> 9;                       // (u * KS + s) * 2 + piece
    const int piece = (int)(f & 1); f >>= 1;
    const int s = (int)(f % KS);
    const int u = (int)(f / KS);
    const int k = 32 * s + 8 * (lane >> 4) + jj;
    const int nn = 16 * u + (lane & 15);
    const float v = sigma * (trans ? W[(int64_t)nn * IN + k] : W[(int64_t)k * OUT + nn]);
    const _Float16 hi = (_Float16)v;
    const _Float16 pc = piece == 0 ? hi : (_Float16)(v - (float)hi);
    out[e] = __builtin_bit_cast(uint16_t, pc);
  }
}

hipError_t launch_pack_dense_f16(const float* W, void* out, int IN, int OUT, int trans, hipStream_t st) {
  // trans: pieces of W^T for launch_dense_h16_t (W is [OUT][IN] as seen by the contraction)
  if (IN % 32 || OUT % 16) return hipErrorInvalidValue;
  uint16_t* o = static_cast<uint16_t*>(out);
  const int64_t total = (int64_t)(OUT / 16) * (IN / 32) * 2 * 512;
  hipLaunchKernelGGL(dense_f16_scale_kernel, dim3(1), dim3(1024), 0, st, W, (int64_t)IN * OUT,
                     reinterpret_cast<int*>(o + total));
  hipLaunchKernelGGL(pack_dense_f16_kernel, dim3(128), dim3(256), 0, st, W, o, IN, OUT, trans);
  return hipGetLastError();
}

hipError_t launch_dense_bf_t(const float* dz, int64_t n, int K, const void* Wtbf, int M, float* out, int accumulate,
                             int act, const float* aprev, hipStream_t st, OuterRows xo) {
  if (n == 0) return hipSuccess;
  if (!dense_bf_supported(K, M) || !Wtbf || (xo.s && !act_first_five(xo.act))) return hipErrorInvalidValue;
  return dense_bf_any<true>(dz, n, K, K, Wtbf, nullptr, M, act < 0 ? IGN_K_ACT_LINEAR : act,
                            out, act < 0 ? nullptr : aprev, accumulate, st, xo);
}

hipError_t launch_pack_dense_bf16_t(const float* W, void* out, int IN, int OUT, hipStream_t st) {
  // pieces of W^T ([OUT][IN] contraction over OUT) for launch_dense_bf_t; W is [IN][OUT]
  if (OUT % 32 || IN % 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pack_dense_bf16_kernel, dim3(128), dim3(256), 0, st, W, static_cast<uint16_t*>(out), OUT, IN, 0, 1);
  return hipGetLastError();
}

hipError_t launch_pack_dense_bf16(const float* W, void* out, int IN, int OUT, int chained, hipStream_t st) {
  if (IN % 32 || OUT % 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pack_dense_bf16_kernel, dim3(128), dim3(256), 0, st, W, static_cast<uint16_t*>(out), IN, OUT,
                     chained, 0);
  return hipGetLastError();
}

hipError_t launch_seq_gru_h16(const SeqGruArgs& args, int h, int passes, hipStream_t st) {
  if (args.n_dst == 0) return hipSuccess;
  if (!args.Uh || !args.hdr || (h != 32 && h != 64) || passes != 3 ||
      (args.hs_save && passes != 3))
    return hipErrorInvalidValue;
  const int64_t work = grid_for(args.n_dst, 64);
#define SEQ_H(HH, P, SV)                                                                           \
  {                                                                                                \
    auto k = seq_gru_h16_kernel<HH, P, SV>;                                                        \
    hipLaunchKernelGGL(k, dim3(persistent_grid(k, work)), dim3(256), 0, st, args);                \
  }
  if (args.hs_save) {
    if (h == 32) SEQ_H(32, 3, true)
    else SEQ_H(64, 3, true)
  } else if (h == 32) SEQ_H(32, 3, false)
  else SEQ_H(64, 3, false)
#undef SEQ_H
  return hipGetLastError();
}

// U [H][3H] (unscaled) -> sigma_t U as fp16 (hi, lo) A fragments over (rows: state unit m, k: gate
// unit in the chained order kperm(s, g, jj) = 16 (2 s + (jj >> 2)) + 4 g + (jj & 3)), the layout
// of du's accumulator registers read as the B operand; then sigma_t's exponent.  One block.
// Fragment f = (piece * NT + mt) * KS3 + s, KS3 = 3H / 32.
__global__ __launch_bounds__(1024) void pack_ut_f16_kernel(const float* __restrict__ U, uint16_t* __restrict__ out,
                                                          int H) {
  const int NT = H / 16, KS3 = 3 * H / 32, n = H * 3 * H;
  __shared__ float red[1024];
  float m = 0.f;
  for (int e = threadIdx.x; e < n; e += blockDim.x) m = fmaxf(m, fabsf(U[e]));
  red[threadIdx.x] = m;
  __syncthreads();
  for (int o = blockDim.x / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  m = red[0];
  int es = m > 0.f ? 15 - ((__float_as_int(m) >> 23) - 126) : 0;
  es = min(100, max(-100, es));
  const float sigma = __int_as_float((127 + es) << 23);
  const int64_t total = 2LL * NT * KS3 * 64 * 8;
  for (int64_t e = threadIdx.x; e < total; e += blockDim.x) {
    const int jj = (int)(e & 7), lane = (int)((e >> 3) & 63);
    int64_t f = e >> 9;
    const int s = (int)(f % KS3); f /= KS3;
    const int mt = (int)(f % NT);
    const int piece = (int)(f / NT);
    const int row = 16 * mt + (lane & 15);
    const int k = 16 * (2 * s + (jj >> 2)) + 4 * (lane >> 4) + (jj & 3);
    const float v = sigma * U[(int64_t)row * 3 * H + k];
    const _Float16 hi = (_Float16)v;
    const _Float16 pc = piece == 0 ? hi : (_Float16)(v - (float)hi);
    out[e] = __builtin_bit_cast(uint16_t, pc);
  }
  if (threadIdx.x == 0) reinterpret_cast<int*>(out)[total / 2] = es;
}

hipError_t launch_pack_ut_f16(const float* U, void* out, int H, hipStream_t st) {
  if (H != 32) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pack_ut_f16_kernel, dim3(1), dim3(1024), 0, st, U, static_cast<uint16_t*>(out), H);
  return hipGetLastError();
}

hipError_t launch_pack_u_f16(const float* U, void* out, int H, hipStream_t st) {
  if (H != 32 && H != 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pack_u_f16_kernel, dim3(1), dim3(1024), 0, st, U, static_cast<uint16_t*>(out), H, H);
  return hipGetLastError();
}

hipError_t launch_pack_w_f16(const float* W, void* out, int K, int H, hipStream_t st) {
  if ((H != 32 && H != 64) || K % 32) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pack_u_f16_kernel, dim3(1), dim3(1024), 0, st, W, static_cast<uint16_t*>(out), K, H);
  return hipGetLastError();
}

hipError_t launch_pack_u_bf16(const float* U, void* out, int H, hipStream_t st) {
  if (H != 32 && H != 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pack_u_bf16_kernel, dim3(64), dim3(256), 0, st, U, static_cast<uint16_t*>(out), H, H);
  return hipGetLastError();
}

hipError_t launch_pack_w_bf16(const float* W, void* out, int K, int H, hipStream_t st) {
  if ((H != 32 && H != 64) || K % 32) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pack_u_bf16_kernel, dim3(64), dim3(256), 0, st, W, static_cast<uint16_t*>(out), K, H);
  return hipGetLastError();
}


hipError_t launch_sum_gru_h16(const SumGruArgs& args, int din, int h, hipStream_t st) {
  if (args.n_dst == 0) return hipSuccess;
  if (din != 64 || h != 64 || !args.Wbf || !args.Ubf || args.msg_w || args.conv_kp) return hipErrorInvalidValue;
  constexpr int WV = 12;
  auto kern = sum_gru_h16_kernel<64, 64, WV, 4>;
  const int64_t work = (args.n_dst + 16 * WV - 1) / (16 * WV);
  hipLaunchKernelGGL(kern, dim3(persistent_grid(kern, work, 64 * WV)), dim3(64 * WV), 0, st, args);
  return hipGetLastError();
}

hipError_t launch_sum_gru_bf(const SumGruArgs& args, int din, int h, hipStream_t st) {
  if (args.n_dst == 0) return hipSuccess;
  if (din != 64 || h != 64 || !args.Wbf || !args.Ubf || args.msg_w || args.conv_kp) return hipErrorInvalidValue;
  constexpr int WV = 12;
  auto kern = sum_gru_bf_kernel<64, 64, WV, 4>;
  const int64_t work = (args.n_dst + 16 * WV - 1) / (16 * WV);
  hipLaunchKernelGGL(kern, dim3(persistent_grid(kern, work, 64 * WV)), dim3(64 * WV), 0, st, args);
  return hipGetLastError();
}

hipError_t launch_tsgemm_bf(const float* A, int lda, const float* B, int ldb, int64_t n_rows, int M, int N, int ones,
                            int64_t chunk, int64_t chunks, int tiles, int wpb, float* part, hipStream_t st) {
  // tsgemm_bf_lds where the pieces are shared by >= 4 tiles: 1.78 -> 1.51 ms for the readout's 256 x 256
  // weight gradient, bitwise the same partials
  if (M > 0 && N > 0 && M % 64 == 0 && N % 64 == 0 && N <= 256 && (M / 64) * (N / 64) >= 4) {
    const int tiles_m = M / 64, tiles_n = N / 64;
    const int mtb = std::min(std::min(tiles_m, 8 / tiles_n), (kTsLdsCols - N) / 64);
    const dim3 g2((unsigned)chunks, (unsigned)((tiles_m + mtb - 1) / mtb));
    hipLaunchKernelGGL(tsgemm_bf_lds_kernel, g2, dim3(512), 0, st, A, lda, B, ldb, n_rows, M, N, ones, chunk, mtb,
                       part);
    return hipGetLastError();
  }
  if (ones && M > 0 && M % 64 == 0) tiles = (M / 64) * ((N + 63) / 64);   // the ones row folded (kernel)
  dim3 grid((unsigned)chunks, (unsigned)((tiles + wpb - 1) / wpb));
  hipLaunchKernelGGL(tsgemm_bf_kernel, grid, dim3(64 * wpb), 0, st, A, lda, B, ldb, n_rows, M, N, ones, chunk, part);
  return hipGetLastError();
}
