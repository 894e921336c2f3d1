// host_types.h — host-only plan types and helpers shared by the engine (engine_internal.h) and the
// batch lowering (batch_lower.h).  No HIP header: everything here compiles with a plain C++17 compiler.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ignmp.h"

// message code = slot << 29 | row (kernels.h defines the same three for the device code)
#ifndef IGN_SLOT_SHIFT
#define IGN_SLOT_SHIFT 29u
#define IGN_ROW_MASK ((1u << IGN_SLOT_SHIFT) - 1u)
#define IGN_MAX_SLOTS 4
#endif
static_assert(IGN_SLOT_SHIFT == 29u && IGN_MAX_SLOTS == 4, "kernels.h and host_types.h disagree");

namespace ign {

int fail(int code, const char* fmt, ...);

// devpool.cpp: process-wide cache of large host blocks (>= kHostBlockMin bytes) for the batch
// builders' index tables.  A batch touches ~10^8 bytes of fresh host memory; straight from malloc
// that is mmap + page faults on every batch and munmap on destroy, serialised on the process's
// address-space lock across the input workers.  Cached blocks keep their pages (transparent huge
// pages where the kernel allows) and are pinned for DMA uploads where the runtime allows.
constexpr size_t kHostBlockMin = (size_t)1 << 20;
void* host_block_alloc(size_t bytes);
void host_block_free(void* p, size_t bytes);
template <class T>
struct HostAlloc {
  using value_type = T;
  HostAlloc() = default;
  template <class U>
  HostAlloc(const HostAlloc<U>&) {}
  T* allocate(size_t n) {
    const size_t bytes = n * sizeof(T);
    void* p = bytes >= kHostBlockMin ? host_block_alloc(bytes) : std::malloc(std::max<size_t>(bytes, 1));
    if (!p) throw std::bad_alloc();
    return static_cast<T*>(p);
  }
  void deallocate(T* p, size_t n) {
    const size_t bytes = n * sizeof(T);
    if (bytes >= kHostBlockMin) host_block_free(p, bytes);
    else std::free(p);
  }
  template <class U>
  bool operator==(const HostAlloc<U>&) const { return true; }
  template <class U>
  bool operator!=(const HostAlloc<U>&) const { return false; }
};
template <class T>
using hvec = std::vector<T, HostAlloc<T>>;

constexpr double kMfmaBf16Flops = 2.0 * 16 * 16 * 32;   // v_mfma_f32_16x16x32_bf16
constexpr double kMfmaF32Flops = 2.0 * 16 * 16 * 4;     // v_mfma_f32_16x16x4_f32

struct CellP {
  int din, H;
  int64_t off_k, off_rk, off_b;   // raw Keras-layout params
  int64_t pk_w, pk_u, pk_b;       // packed fragments (in d_packed)
  int64_t pk_wt = -1, pk_ut = -1; // backward: unscaled W^T / U^T fragments (pack_a)
  int64_t pk_wbf = -1;            // split-bf16 input-kernel fragments (sum variant 7, DIN = H = 64)
  int64_t pk_ubf = -1;            // split-bf16 recurrent-kernel fragments (seq variants 4/5)
  int64_t pk_wh = -1;             // split-fp16 input-kernel fragments + scale (sum variant 8, DIN = H = 64)
  int64_t pk_uh = -1;             // split-fp16 recurrent-kernel fragments + scale (seq variants 6/7)
  int64_t pk_uth = -1;            // backward: split-fp16 U fragments for dh = du . U^T (H = 32)
  bool used = false;
  // ign_plan_set_cell_options (Keras GRUCell defaults).  A cell with any other value is a non-default
  // cell: unscaled pack_gru fragments, none of the split pieces above, the generalised kernels
  int act = IGN_ACT_TANH, ract = IGN_ACT_SIGMOID;
  bool use_bias = true, reset_after = true;
  bool is_default() const { return act == IGN_ACT_TANH && ract == IGN_ACT_SIGMOID && use_bias && reset_after; }
  int bias_rows() const { return !use_bias ? 0 : reset_after ? 2 : 1; }   // of [3H] in the raw layout
};

struct DenseP {
  int in, out, act, use_bias;
  float l2 = 0.f;
  int64_t off_w, off_b, pk_w = -1;   // pk_w: forward fragments (fused readout, training readout)
  int64_t pk_wt = -1;             // backward: A fragments of W [in][out] (row_gemm_t), if supported
  int64_t pk_bf = -1;             // fused readout: split-bf16 A fragments (readout variants 2/3)
  int64_t pk_h = -1;              // fused readout, layer 2: scaled split-fp16 fragments (readout variant 4)
  int64_t pk_h32 = -1;            // ... the same pieces in variant 5's order (readout_h32.hip)
  int64_t pk_bfn = -1;            // training forward: split-bf16 pieces, natural k (dense_bf)
  int64_t pk_bft = -1;            // training backward: split-bf16 pieces of W^T (dense_bf_t)
  int64_t pk_hn = -1, pk_ht = -1;  // training: scaled split-fp16 pieces of W / W^T (dense_h16)
};

struct MsgNN {                    // message-creation network of one MP source (GM:440-475)
  std::vector<int> inputs;        // enum ign_message_input, in order
  std::vector<int> widths;        // floats per edge of each input part
  int param_dim = 0;
  int din = 0, din_pad = 0;       // concatenated input width, padded to 16 for the MFMA layers
  std::vector<DenseP> layers;
  int dout() const { return layers.empty() ? 0 : layers.back().out; }
};

struct MPP {
  int dst, aggr, concat_axis, cell;
  std::vector<ign_source_desc> src;
  bool sorted;                    // sorted (sequence) update vs single-step update
  int din;
  int act = 0;                    // convolution activation (AUX:370-374)
  bool feature_concat = false;    // concat on axis 2 (AUX:443-456): step input = [src_1 | src_2 | ...]
  std::vector<int> slice_off;     // feature_concat: first kernel row of each source's slice
  std::vector<int64_t> pk_slice;  // feature_concat: packed W-slice fragments per source
  std::vector<MsgNN> nn;          // per source; no layers = direct_assignation
  bool dead_in_last_iter = false; // nothing reads the destination's states after the last iteration's
                                  // update (plan_lower.cpp mark_dead_last): the resident forward leaves it out
};

// one index array of an ign_batch_desc (adj_src / adj_dst / adj_seq / interleave_idx): int32
// elements when the desc's index_bytes is 4 (ABI 13), else int64
struct IdxArr {
  const void* p = nullptr;
  bool w32 = false;
  IdxArr() = default;
  IdxArr(const int64_t* q, int32_t index_bytes) : p(q), w32(index_bytes == 4) {}
  int64_t operator[](int64_t k) const {
    return w32 ? (int64_t) static_cast<const int32_t*>(p)[k] : static_cast<const int64_t*>(p)[k];
  }
};

// a sum MP's destinations with at least this many messages take the segmented sum (sum_seg_kernel,
// one wave per destination); the others the lane walk of the GRU-step kernel (IGN_SUM_WINDOW=2: every
// destination segmented).  Per destination, so a graph's rows take the same order alone and in any batch.
// IGN_SUM_WINDOW=0, the lane walk's A/B switch, refuses a batch with a destination of >= 64 messages
// (lower_sum_agg): a float32 chain that long leaves the fp32 class -- Q-size synth50's nodes as
// lane walks landed at 4.3x IEEE float32's error (all of them) and 1.8x (those below 128), DESIGN.md §4
constexpr int64_t kSegMinMessages = 64;
inline int64_t seg_min_messages(int sum_window) { return sum_window == 2 ? 0 : kSegMinMessages; }

// f(lo, hi) over [0, n) in contiguous chunks on up to IGN_BUILD_THREADS threads (default 2: a
// training loop already runs several builders), at least min_per items each; the caller's thread
// takes the first chunk
template <class F>
void parallel_ranges(int64_t n, int64_t min_per, F&& f) {
  static const int T = [] {
    const char* v = std::getenv("IGN_BUILD_THREADS");
    return v && *v ? std::max(1, std::atoi(v)) : 2;
  }();
  const int nt = (int)std::min<int64_t>(T, std::max<int64_t>(1, n / std::max<int64_t>(1, min_per)));
  if (nt <= 1) {
    f(0, n);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(nt - 1);
  for (int t = 1; t < nt; ++t) th.emplace_back([&f, n, nt, t] { f(n * t / nt, n * (t + 1) / nt); });
  f(0, n / nt);
  for (auto& x : th) x.join();
}

// Destination processing order: one global stable sort by message count, descending (tiles of
// equal length; the longest sequences start first).  Measured faster than per-graph orders with
// XCD-aware tiles for both the ordered and the sum updates (profiles/r02/seq_experiments).  A
// counting sort (counts are small): O(n), the same order as std::stable_sort.  (batch_lower.cpp)
void sort_order(hvec<int32_t>& order, const hvec<int64_t>& cnt);

// IGN_BUILD_PROF=1: named host sections of one batch build (the time since the previous mark),
// printed as one line at the end of the build
struct BuildMarks {
  bool on;
  double last = 0;
  std::string line;
  static double now() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
  }
  explicit BuildMarks(bool enabled) : on(enabled), last(enabled ? now() : 0.0) {}
  void mark(const char* what) {
    if (!on) return;
    const double t = now();
    char buf[96];
    snprintf(buf, sizeof buf, " %s %.2f", what, t - last);
    line += buf;
    last = t;
  }
  void print(const char* head) const {
    if (on) fprintf(stderr, "[ign-build] %s sections:%s\n", head, line.c_str());
  }
};

}  // namespace ign
