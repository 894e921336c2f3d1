// gru_wide.hip — the GRU updates at DIN = H = 128 (gru_wide_supported, kernel_shapes.h), f32 MFMA
// (v_mfma_f32_16x16x4_f32), default cells only.  DESIGN.md §3l.
//
// At this width one wave cannot hold a 16-row state tile, three gates' accumulators and its share of
// the weights, and U ([128][384] floats, 192 KB) does not fit a CU's LDS.  So the work of one row tile is
// split over the waves of a workgroup by unit tile:
//
//   seq_gru_w128   ordered update.  8 waves own 16 length-sorted destinations; wave w owns units
//                  16w .. 16w + 15 of all three gates and keeps its [128][48] slice of U in 96 registers
//                  per lane as MFMA A fragments, loaded once per (persistent) workgroup.  The new state
//                  tile goes through LDS, [16][132] floats, double-buffered: one barrier per step.
//   gemm_w128      [rows][K] x [K][384] with the weights streamed through LDS in 16-row K chunks (24 KB,
//                  double-buffered).  4 waves own 64 rows; wave w owns unit tiles 2w, 2w + 1 of all three
//                  gates for the four 16-row blocks, so one A fragment read feeds four MFMAs.
//                  PROJECT (K = 128): the ordered MP's table rows x.W + b_in.  SUM_GRU (K = 256): the
//                  messages' sum and the destinations' states go to two LDS tiles, the contraction runs
//                  over [x | h] against [W ; U], the gates are formed in registers.
//
// The k order is kernels.hip's: k(s, g) = 16 (s >> 2) + 4 g + (s & 3), so a float4 of four consecutive
// units of a row, read back from LDS by lane (j, g), is the B operand of four consecutive k-steps, and a
// lane's four accumulator registers of one row are one 16-byte LDS store.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "kernels.h"

#include "device_common.h"

namespace {

constexpr int kH = 128, k3H = 384;
constexpr int kSeqWaves = 8;
constexpr int kSeqStride = kH + 4;     // LDS floats per state row: 33 float4s, odd, so the 16 rows that the
                                       // lanes of one g read at one column land in 16 different 16-B banks
constexpr int kChunkF4 = 16 * k3H / 4; // float4s of one K chunk: [24 gate-unit tiles][64 lanes]
constexpr int kTileF4 = 64 * kH / 4;   // float4s of one [64][128] row tile
constexpr size_t kProjectLds = (size_t)(2 * kChunkF4 + kTileF4) * sizeof(f4);       // 80 KB
constexpr size_t kSumGruLds = (size_t)(2 * kChunkF4 + 2 * kTileF4) * sizeof(f4);    // 112 KB

// float4 q of row r of a [64][128] LDS tile.  Rows are 32 float4s, a multiple of the bank count, so the
// column index is xor-ed with the row's low bits: the 16 rows a B-fragment read touches at one column
// land in 16 different 16-B banks, with no padding.
__device__ __forceinline__ int tile_at(int r, int q) { return r * 32 + (q ^ (r & 15)); }

__device__ __forceinline__ const float* wide_src(const SrcBases& sb, uint32_t code) {
  const uint32_t slot = code >> IGN_SLOT_SHIFT;
  const float* b = sb.base[0];
  if (slot == 1) b = sb.base[1];
  if (slot == 2) b = sb.base[2];
  if (slot == 3) b = sb.base[3];
  return b + (int64_t)(code & IGN_ROW_MASK) * kH;
}

// ---------------------------------------------------------------------------------------------
// Packing (the default cell's scaling: z, r columns by -log2 e, candidate columns by 2 log2 e).
//   IGN_PACK_WIDE_U   U [128][384] -> per wave w its slice: [w][gate][k-step / 4][lane][4],
//                     lane l, element q of k-step group c -> U[16c + 4 (l >> 4) + q][128 gate + 16w + (l & 15)]
//   IGN_PACK_WIDE_W / _WU   M = W, or [W ; U] (M2 = U, rows 128 ..) -> K chunks: [chunk][gate 8 + t][lane][4],
//                     element q of chunk c -> M[16c + 4 (l >> 4) + q][128 gate + 16t + (l & 15)]
//   IGN_PACK_WIDE_B   bias [2][384] -> [4][128]: bz_in + bz_rec, br_in + br_rec, bh_in, bh_rec (pack_gru's)
__global__ void pack_wide_kernel(const float* __restrict__ M, const float* __restrict__ M2, float* __restrict__ out,
                                 int what) {
  const int64_t total = what == IGN_PACK_WIDE_B ? 4 * kH : what == IGN_PACK_WIDE_WU ? 2LL * kH * k3H : (int64_t)kH * k3H;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (what == IGN_PACK_WIDE_B) {
      const int which = (int)(i / kH), u = (int)(i % kH);
      const float* bin = M;
      const float* brec = M + k3H;
      out[i] = which == 0 ? IGN_NLOG2E * (bin[u] + brec[u])
             : which == 1 ? IGN_NLOG2E * (bin[kH + u] + brec[kH + u])
             : which == 2 ? IGN_2LOG2E * bin[2 * kH + u] : IGN_2LOG2E * brec[2 * kH + u];
      continue;
    }
    const int q = (int)(i & 3), lane = (int)((i >> 2) & 63);
    const int64_t f = i >> 8;
    int gate, t, c;
    if (what == IGN_PACK_WIDE_U) {
      c = (int)(f % 8);
      gate = (int)((f / 8) % 3);
      t = (int)(f / 24);
    } else {
      t = (int)(f % 8);
      gate = (int)((f / 8) % 3);
      c = (int)(f / 24);
    }
    const int k = 16 * c + 4 * (lane >> 4) + q;
    const int col = gate * kH + 16 * t + (lane & 15);
    const float sc = gate == 2 ? IGN_2LOG2E : IGN_NLOG2E;
    const float* src = k < kH ? M + (int64_t)k * k3H : M2 + (int64_t)(k - kH) * k3H;
    out[i] = sc * src[col];
  }
}

// ---------------------------------------------------------------------------------------------
// Ordered / interleave / concat (axis 1) update at H = 128: seq_gru2_kernel's steps (the same table, step
// codes, masks and gate arithmetic), one workgroup of 8 waves per 16-destination tile.  Wave w forms
// units 16w .. 16w + 15 of z, r and the candidate from its own columns of the projected row and of
// h.U (reset_after: the candidate needs no other wave's gate), and publishes the new states through LDS.
__global__ __launch_bounds__(64 * kSeqWaves) void seq_gru_w128_kernel(SeqGruArgs a) {
  __shared__ f4 sh[2][16 * kSeqStride / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int u0 = 16 * wave + 4 * g;   // the lane's four accumulator units of row j

  f4 u[3][8];   // the wave's slice of U: 96 registers, resident across tiles
  {
    const f4* up = reinterpret_cast<const f4*>(a.Up) + (int64_t)wave * 24 * 64 + lane;
#pragma unroll
    for (int G = 0; G < 3; ++G)
#pragma unroll
      for (int c = 0; c < 8; ++c) u[G][c] = up[(G * 8 + c) * 64];
  }
  const f4 bh = ld4(a.bias + 3 * kH + u0);
  const float* tab = a.table + u0;
  const int rd = j * (kSeqStride / 4) + g;             // B-fragment read: row j, float4 4c + g
  const int wr = j * (kSeqStride / 4) + 4 * wave + g;  // the lane's own float4 of row j

  const int64_t n_tiles = (a.n_dst + 15) / 16;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t pos = tile * 16 + j;
    const bool valid = pos < a.n_dst;
    const int row = valid ? a.order[pos] : 0;
    const int L = valid ? a.len[pos] : 0;
    const uint32_t* codes = a.step_code + (valid ? a.step_ptr[pos] : 0);
    f4 h = valid ? ld4(a.h_in + (int64_t)row * kH + u0) : f4{0, 0, 0, 0};
    int Lmax = L;   // every wave holds the same 16 rows: the same trip count in all of them
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) Lmax = max(Lmax, __shfl_xor(Lmax, o));
    sh[0][wr] = h;
    __syncthreads();

    uint32_t code = codes[0];
    for (int t = 0; t < Lmax; ++t) {
      const f4* cur = sh[t & 1];
      const float* p = tab + (int64_t)code * k3H;
      const f4 xz = ld4(p), xr = ld4(p + kH), xh = ld4(p + 2 * kH);
      const uint32_t next = codes[t + 1];
      f4 az = f4{0, 0, 0, 0}, ar = f4{0, 0, 0, 0}, ah = bh;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const f4 hb = cur[rd + 4 * c];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          az = MFMA(u[0][c][q], hb[q], az);
          ar = MFMA(u[1][c][q], hb[q], ar);
          ah = MFMA(u[2][c][q], hb[q], ah);
        }
      }
      const bool act = t < L;
#pragma unroll
      for (int r = 0; r < 4; ++r) {   // the table rows carry the input-side biases (PROJECT below)
        const float z = sig2_(az[r] + xz[r]);
        const float rr = sig2_(ar[r] + xr[r]);
        const float c = tanh2_(xh[r] + rr * ah[r]);
        const float hn = c + z * (h[r] - c);
        h[r] = act ? hn : h[r];
      }
      // the other buffer: its last readers passed the barrier that ended the previous step
      sh[(t + 1) & 1][wr] = h;
      __syncthreads();
      code = next;
    }
    if (valid) st4(a.h_out + (int64_t)row * kH + u0, h);
  }
}

// ---------------------------------------------------------------------------------------------
struct GemmWideArgs {
  const float* Wk;         // K chunks (pack_wide W, or [W ; U])
  const float* bias;       // [4][128]
  // PROJECT
  const float* x;          // [n][128]
  float* out;              // [n][384]
  float* bias_row;         // the table's hole row (or null): the input-side biases alone
  // SUM_GRU
  SumGruArgs s;
  int64_t n;               // rows
};

// the 96 MFMAs of one K chunk: A fragments of the wave's two unit tiles of each gate from wb, the B
// fragments of the four row blocks from float4 column 4 kc + g of `tile`
__device__ __forceinline__ void chunk_mfma(const f4* __restrict__ wb, const f4* __restrict__ tile, int kc, int wave,
                                           int lane, f4 (&a0)[2][4], f4 (&a1)[2][4], f4 (&a2)[2][4]) {
  const int j = lane & 15, g = lane >> 4;
  f4 b[4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) b[rb] = tile[tile_at(16 * rb + j, 4 * kc + g)];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int t = 2 * wave + tt;
    const f4 w0 = wb[t * 64 + lane], w1 = wb[(8 + t) * 64 + lane], w2 = wb[(16 + t) * 64 + lane];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        a0[tt][rb] = MFMA(w0[q], b[rb][q], a0[tt][rb]);
        a1[tt][rb] = MFMA(w1[q], b[rb][q], a1[tt][rb]);
        a2[tt][rb] = MFMA(w2[q], b[rb][q], a2[tt][rb]);
      }
  }
}

enum { GW_PROJECT = 0, GW_SUM_GRU = 1 };

template <int MODE>
__global__ __launch_bounds__(256) void gemm_w128_kernel(GemmWideArgs a) {
  extern __shared__ f4 lds[];
  f4* const wbuf = lds;                    // [2][kChunkF4]
  f4* const xt = lds + 2 * kChunkF4;       // [64][128] x (PROJECT: the rows; SUM_GRU: the message sums)
  f4* const ht = xt + kTileF4;             // SUM_GRU: [64][128] the destinations' states
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * 64;
  constexpr int NK = MODE == GW_PROJECT ? 8 : 16;
  const f4* const wk = reinterpret_cast<const f4*>(a.Wk);

  f4 stage[6];   // the next chunk on its way from memory to LDS
#pragma unroll
  for (int i = 0; i < 6; ++i) stage[i] = wk[tid + 256 * i];

  if constexpr (MODE == GW_PROJECT) {
    if (a.bias_row && blockIdx.x == 0)
      for (int i = tid; i < k3H; i += 256) a.bias_row[i] = a.bias[i];
    for (int i = tid; i < kTileF4; i += 256) {
      const int r = i >> 5, q = i & 31;
      xt[tile_at(r, q)] = row0 + r < a.n ? ld4(a.x + (row0 + r) * kH + 4 * q) : f4{0, 0, 0, 0};
    }
  } else {
    // Phase 1.  Wave w sums destinations 16w .. 16w + 15 of the tile, one at a time: a load instruction
    // fetches two message rows (lanes 0-31 the even messages of the CSR range, 32-63 the odd ones, four
    // loads in flight), then the two halves are added.  The order is the destination's CSR order alone.
    const int half = lane >> 5, q = lane & 31;
    for (int d = 0; d < 16; ++d) {
      const int r = 16 * wave + d;
      const int64_t pos = row0 + r;
      const bool valid = pos < a.n;
      const int64_t m0 = valid ? a.s.msg_ptr[pos] : 0, m1 = valid ? a.s.msg_ptr[pos + 1] : 0;
      f4 acc = f4{0, 0, 0, 0};
      for (int64_t m = m0 + half; m < m1; m += 8) {
        f4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int64_t mk = m + 2 * k < m1 ? m + 2 * k : m;   // clamped: a loaded row that is not added
          v[k] = ld4(wide_src(a.s.src, a.s.msg_src[mk]) + 4 * q);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool on = m + 2 * k < m1;
          const f4 sum = acc + v[k];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = on ? sum[e] : acc[e];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += __shfl_xor(acc[e], 32);
      if (half == 0) xt[tile_at(r, q)] = acc;
      else ht[tile_at(r, q)] = valid ? ld4(a.s.h_in + (int64_t)a.s.order[pos] * kH + 4 * q) : f4{0, 0, 0, 0};
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) wbuf[tid + 256 * i] = stage[i];
  __syncthreads();

  // accumulators: z, r, the candidate's input side (ax) and, SUM_GRU, its recurrent side (ah)
  f4 az[2][4], ar[2][4], ax[2][4], ah[2][4];
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const float* bp = a.bias + 16 * (2 * wave + tt) + 4 * g;
    const f4 b0 = ld4(bp), b1 = ld4(bp + kH), b2 = ld4(bp + 2 * kH), b3 = ld4(bp + 3 * kH);
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      az[tt][rb] = b0;
      ar[tt][rb] = b1;
      ax[tt][rb] = b2;
      ah[tt][rb] = b3;
    }
  }
#pragma unroll 1
  for (int kc = 0; kc < NK; ++kc) {
    if (kc + 1 < NK) {
#pragma unroll
      for (int i = 0; i < 6; ++i) stage[i] = wk[(int64_t)(kc + 1) * kChunkF4 + tid + 256 * i];
    }
    const f4* wb = wbuf + (kc & 1) * kChunkF4;
    if (MODE == GW_PROJECT || kc < 8) chunk_mfma(wb, xt, kc, wave, lane, az, ar, ax);
    else chunk_mfma(wb, ht, kc - 8, wave, lane, az, ar, ah);
    if (kc + 1 < NK) {   // the other buffer: its last readers passed the barrier that ended chunk kc - 1
      f4* nb = wbuf + ((kc + 1) & 1) * kChunkF4;
#pragma unroll
      for (int i = 0; i < 6; ++i) nb[tid + 256 * i] = stage[i];
    }
    __syncthreads();
  }

#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
    const int r = 16 * rb + j;
    const int64_t pos = row0 + r;
    if (pos >= a.n) continue;
    if constexpr (MODE == GW_PROJECT) {
      float* o = a.out + pos * k3H + 4 * g;
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int c0 = 16 * (2 * wave + tt);
        st4(o + c0, az[tt][rb]);
        st4(o + kH + c0, ar[tt][rb]);
        st4(o + 2 * kH + c0, ax[tt][rb]);
      }
    } else {
      float* o = a.s.h_out + (int64_t)a.s.order[pos] * kH + 4 * g;
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int t = 2 * wave + tt;
        const f4 h = ht[tile_at(r, 4 * t + g)];
        f4 hn;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float z = sig2_(az[tt][rb][e]);
          const float rr = sig2_(ar[tt][rb][e]);
          const float c = tanh2_(ax[tt][rb][e] + rr * ah[tt][rb][e]);
          hn[e] = c + z * (h[e] - c);
        }
        st4(o + 16 * t, hn);
      }
    }
  }
}

// seq_gru_w128's persistent grid: one workgroup of 8 waves x up to 256 registers per CU (the CU count:
// gru_wide_prepare_device)
int g_seq_cus = 256;

}  // namespace

// the dynamic-LDS limit of gemm_w128's two forms (80 and 112 KB) and the CU count, once per device
hipError_t gru_wide_prepare_device() {
  static std::mutex mu;
  static std::vector<char> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(mu);
  if ((int)done.size() <= dev) done.resize(dev + 1, 0);
  if (done[dev]) return hipSuccess;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_w128_kernel<GW_PROJECT>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)kProjectLds);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_w128_kernel<GW_SUM_GRU>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSumGruLds);
  if (e != hipSuccess) return e;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) g_seq_cus = cus;
  done[dev] = 1;
  return hipSuccess;
}

hipError_t launch_pack_wide(const float* M, const float* M2, float* out, int what, hipStream_t st) {
  if (what < IGN_PACK_WIDE_U || what > IGN_PACK_WIDE_B || !M || !out || (what == IGN_PACK_WIDE_WU && !M2))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(pack_wide_kernel, dim3(what == IGN_PACK_WIDE_B ? 2 : 192), dim3(256), 0, st, M, M2, out, what);
  return hipGetLastError();
}

hipError_t launch_seq_gru_w128(const SeqGruArgs& args, hipStream_t st) {
  if (args.n_dst == 0) return hipSuccess;
  const int64_t n_tiles = (args.n_dst + 15) / 16;
  hipLaunchKernelGGL(seq_gru_w128_kernel, dim3((unsigned)std::min<int64_t>(n_tiles, g_seq_cus)), dim3(64 * kSeqWaves), 0, st, args);
  return hipGetLastError();
}

hipError_t launch_project_w128(const float* x, int64_t n, const float* Wk, const float* bp, float* out, float* bias_row,
                               hipStream_t st) {
  if (hipError_t e = gru_wide_prepare_device()) return e;
  GemmWideArgs a{};
  a.Wk = Wk;
  a.bias = bp;
  a.x = x;
  a.out = out;
  a.bias_row = bias_row;
  a.n = n;
  // (no rows: the hole row is still written)
  const unsigned grid = (unsigned)std::max<int64_t>((n + 63) / 64, bias_row ? 1 : 0);
  if (!grid) return hipSuccess;
  hipLaunchKernelGGL(gemm_w128_kernel<GW_PROJECT>, dim3(grid), dim3(256), kProjectLds, st, a);
  return hipGetLastError();
}

hipError_t launch_sum_gru_w128(const SumGruArgs& args, hipStream_t st) {
  if (args.n_dst == 0) return hipSuccess;
  if (args.msg_w || args.conv_kp || args.x_save || args.sum_save || args.proj_out) return hipErrorInvalidValue;
  if (hipError_t e = gru_wide_prepare_device()) return e;
  GemmWideArgs a{};
  a.Wk = args.Wp;
  a.bias = args.bias;
  a.s = args;
  a.n = args.n_dst;
  hipLaunchKernelGGL(gemm_w128_kernel<GW_SUM_GRU>, dim3((unsigned)((args.n_dst + 63) / 64)), dim3(256), kSumGruLds, st, a);
  return hipGetLastError();
}
