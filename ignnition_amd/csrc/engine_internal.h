// engine_internal.h — plan / batch structures shared by engine.cpp (inference) and the training
// units (train.cpp, train_alloc.cpp, mp_backward.cpp).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstdarg>
#include <cstdint>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/ignmp.h"
#include "kernels.h"
#include "dropout_kernels.h"
#include "layernorm_kernels.h"
#include "host_types.h"   // the host-only types (MPP, hvec, IdxArr, ...), shared with batch_lower.h
#include "plan_lower.h"   // PlanModel: the lowered plan without the device

struct TrainState;                 // train_state.h
void train_state_destroy(TrainState* t);   // train_alloc.cpp
// between ign_forward_train_begin and the end of that forward's backward (train.cpp)
bool train_step_open(const TrainState* t);

namespace ign {

// devpool.cpp: the plan's device-memory cache (batch and training buffers).  Blocks handed back by
// pool_release are reused once an event recorded on `after` has completed.  scratch: a block the
// caller does not fill on allocation (IGN_POOL_POISON=1 fills it with NaN, via the upload stream).
struct DevPool;
std::shared_ptr<DevPool> pool_create(int device);
hipError_t pool_alloc(DevPool* pool, void** out, size_t bytes, bool scratch);
void pool_release(DevPool* pool, const std::vector<void*>& blocks, hipStream_t after);
void pool_stats(DevPool* pool, int64_t* live_bytes, int64_t* idle_bytes);
bool pool_enabled(const DevPool* pool);
void pool_trim_idle(DevPool* pool);   // every idle block, waiting for its fence
void host_cache_trim();               // every idle host block (host_types.h: host_block_alloc / _free)

#define HIP_TRY(expr)                                                                             \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) return fail(IGN_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e));    \
  } while (0)

enum { K_INIT = 0, K_SEQ = 1, K_SUM = 2, K_READOUT = 3, K_PROJECT = 4, K_OTHER = 5, K_RESIDENT = 6, K_KINDS = 7 };

// per timed launch: algorithmic FLOPs / bytes and the FLOPs its MFMAs execute (bf16 / f32 pipe)
struct EvCost {
  double flops = 0, bytes = 0, mfma_bf16 = 0, mfma_f32 = 0;
};

struct MPB {
  bool sorted = false;
  int64_t n_dst = 0, n_steps = 0, n_msgs = 0, edges = 0;
  int64_t wave_steps = 0;          // sorted MPs: sum over 16-row tiles of the tile's longest sequence
  int32_t* d_order = nullptr;
  int32_t* d_len = nullptr;
  int32_t* d_step_ptr = nullptr;
  int32_t* d_msg_ptr = nullptr;
  uint32_t* d_msg_src = nullptr;
  uint32_t* d_step_code = nullptr;
  int32_t* d_seq_hdr = nullptr;   // sorted MPs: per order position {order, len, step_ptr, first code} (SeqGruArgs::hdr)
  float* d_table = nullptr;       // sorted MPs: [sources' rows | zero row | multi rows][3H]
  std::vector<int64_t> src_off;   // first table row of each source
  std::vector<int64_t> src_rows;
  int64_t zero_row = 0, n_multi = 0;
  int64_t n_interior = 0;         // sum MPs: order[0, n_interior) reads no halo row
  int32_t* d_multi_ptr = nullptr;
  uint32_t* d_multi_rows = nullptr;
  // attention (AUX:264-343): per-message softmax weights over dense (destination, position)
  // cells, grouped per (graph, position) for the axis-0 softmax
  int64_t n_cells = 0, n_groups = 0;
  float* d_msg_w = nullptr;       // [n_msgs] in CSR order
  int32_t* d_group_ptr = nullptr; // [n_groups + 1] cell ranges
  int32_t* d_group_empty = nullptr;
  int32_t* d_cell_dst = nullptr;
  int32_t* d_cell_ptr = nullptr;  // [n_cells + 1] ranges of d_cell_msgs
  int32_t* d_cell_msgs = nullptr; // CSR message positions
  float* d_ecell = nullptr;
  float* d_s_src[IGN_MAX_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
  float* d_s_dst = nullptr;
  // message networks: per source, the per-edge input, the layer outputs (last = the messages)
  int64_t n_edges[IGN_MAX_SLOTS] = {0, 0, 0, 0};
  int32_t* d_edge_src[IGN_MAX_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
  int32_t* d_edge_dst[IGN_MAX_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
  float* d_edge_params[IGN_MAX_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
  float* d_msg_in[IGN_MAX_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
  std::vector<float*> d_msg_layer[IGN_MAX_SLOTS];
  // windowed sum (SumWinArgs; single-source sums over graph-local rows): the aggregation runs per
  // (graph, destination chunk) from LDS windows, then the GRU step reads x through an identity CSR
  int64_t n_win_wg = 0;
  bool sum_seg = false;        // segmented sum (sum_seg_kernel) into d_xsum, then the GRU step
  int64_t n_seg = 0;           // ... for order positions [0, n_seg): destinations with >= 64 messages
                               // (seg_min_messages); the GRU step reads their x from d_xsum (slot 1)
  int64_t* d_win_wg = nullptr;
  int32_t* d_win_dst = nullptr;
  int32_t* d_win_ptr = nullptr;
  int32_t* d_win_src = nullptr;
  float* d_xsum = nullptr;
  int32_t* d_id_ptr = nullptr;
  uint32_t* d_id_src = nullptr;
  double flops = 0, bytes = 0;    // algorithmic, per launch
  // host copies of the index tables (the training path builds their transposes)
  hvec<int32_t> h_order, h_len, h_step_ptr, h_msg_ptr, h_multi_ptr;
  hvec<uint32_t> h_step_code, h_msg_src, h_multi_rows;
};

struct RoBatchOp {
  float* out[2] = {nullptr, nullptr};
  float* cat = nullptr;           // neural_network: concatenated input
  std::vector<float*> tmp;        // neural_network: hidden layer outputs
  int32_t* idx[2] = {nullptr, nullptr};   // extend: global source / destination rows per edge
  // pooling: chunks of <= POOL_CHUNK rows, per-graph chunk ranges, partial results
  int64_t n_chunks = 0;
  int64_t* d_chunk = nullptr;     // [n_chunks][2] global row ranges
  int32_t* d_chunk_ptr = nullptr; // [G + 1]
  int64_t* d_count = nullptr;     // [G] rows per graph
  float* d_partial = nullptr;     // [n_chunks][F]
  int64_t* d_seg = nullptr;       // product: [G + 1] row offsets of the output space
  int64_t* d_inoff = nullptr;     // pooling: [G + 1] row offsets of the input space (backward)
  std::vector<int32_t> h_idx[2];  // extend: host copies of idx (the backward's transposed CSRs)
};

// a training forward / backward's stream and the per-site buffers of its batch
struct DropRun {
  uint64_t seed = 0;
  uint32_t step = 0;
  float* const* buf = nullptr;   // per site: its output (a site before a layer) or its input (after the last)
};
// the LayerNormalization layers' buffers of a batch, per site of ign_plan::norms: buf as DropRun's;
// stats [rows][2] = (mean, rstd) of the training forward for its backward, null in inference
struct NormRun {
  float* const* buf = nullptr;
  float* const* stats = nullptr;
};

}  // namespace ign

using namespace ign;

// the lowered model, its layouts and switches (PlanModel), plus what needs a device or a run
struct ign_plan : PlanModel {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  bool external_stream = false;   // set by ign_plan_set_stream (may be the null stream)
  float* d_params = nullptr;
  float* d_packed = nullptr;
  bool params_set = false;
  // timing
  bool timing = false;
  uint32_t timing_kinds = ~0u;    // kernel kinds that get event pairs (ign_plan_set_timing_kinds)
  std::vector<hipEvent_t> ev;     // pairs
  std::vector<int> ev_kind;
  std::vector<EvCost> ev_cost;
  int ev_slot = 0;                // events recorded since ign_forward_begin
  double* d_red = nullptr;        // loss reductions (training)
  ign_stats_t stats{};
  std::shared_ptr<DevPool> pool;  // batch / training buffers (created with the stream, ensure_device)
  std::string describe;           // ign_plan_create_json: ign_plan_describe_json's document
  bool batch_made = false;        // ign_plan_add_dropout / _layernorm are refused from the first batch on
};

namespace ign {
// LayerNormalization site s on n rows of x (ldx floats apart) into y; stats: NormRun's, or null
inline hipError_t norm_fwd(const ign_plan* p, int s, const float* x, int ldx, int64_t n, float* y, float* stats,
                           hipStream_t st) {
  const NormSite& ns = p->norms[s];
  return launch_layernorm_fwd(x, ldx, n, ns.units, ns.off_gamma >= 0 ? p->d_params + ns.off_gamma : nullptr,
                              ns.off_beta >= 0 ? p->d_params + ns.off_beta : nullptr, ns.epsilon, y, stats, st);
}
}  // namespace ign

struct ign_batch {
  ign_plan* plan = nullptr;
  int G = 0;
  std::vector<int64_t> rows;                    // per entity (owned rows)
  std::vector<int64_t> halo;                    // per entity: peer rows after the owned ones (§8e)
  std::vector<std::vector<int64_t>> row_off;    // [entity][graph]
  std::vector<float*> d_feat;                   // per entity [rows][F] or null
  std::vector<float*> d_state[2];               // per entity ping-pong
  std::vector<int> cur;
  // per entity: the MP whose last-iteration update the resident ign_forward left out (MPP::dead_in_last_iter), so
  // the entity's states are one update behind until finish_entity runs it; -1: they are final
  std::vector<int> behind;
  std::vector<char> ext_state;                  // per entity: ign_batch_bind_state's buffers, read by others
                                                // who cannot ask for that update: its MPs always run
  std::vector<MPB> mp;
  // forward_body only: a sum update may project its new states for the next ordered MP that reads
  // them (fused_proj_target); proj_ready[m'] tells m' that its table is already filled
  bool fuse_ok = false, fuse_last_iter = false;
  // the graph-resident forward (resident.hip, plan->resident): per-graph offsets, the ordered MP's
  // per-graph tile headers, the sum MP's per-graph CSR (local rows); dynamic LDS of the largest graph
  bool resident = false;
  bool res_tried = false;         // resident_batch ran (lazily, at the first ign_forward)
  size_t res_lds = 0;
  int res_form = 0;               // IGN_RES_ALL_LDS / IGN_RES_PATH_GLOBAL / IGN_RES_PATH_CSR_GLOBAL
  int res_graphs = 0;             // resident workgroups per launch (graphs / IGN_RES_GROUP)
  ign_resident_info_t res_info{}; // per launch: bytes (compulsory, round trips, SURVEY B_stage), FLOPs,
                                  // MFMA FLOPs, tile-steps (ign_batch_resident_info): what ign_forward runs
  ign_resident_info_t res_info_full{};   // ... with every update of the last iteration (the training forward)
  int64_t* d_res_path_off = nullptr;
  int64_t* d_res_src_off[kResidentMaxSrc] = {nullptr, nullptr};
  int64_t* d_res_urow_off = nullptr;
  int32_t* d_res_ptile_off = nullptr;
  int32_t* d_res_hdr = nullptr;
  int32_t* d_res_lmsg_off = nullptr;
  int32_t* d_res_lmsg_ptr = nullptr;
  uint16_t* d_res_lmsg_src = nullptr;
  uint16_t* d_res_lorder = nullptr;
  int32_t* d_res_lnseg = nullptr;
  int32_t* d_res_gorder = nullptr;   // workgroup -> graph, by estimated cost, descending (IGN_RES_LPT)
  int32_t* d_res_lcode_off = nullptr;
  uint16_t* d_res_lcode = nullptr;
  int32_t* d_res_hsb = nullptr;   // per header: the training forward's hs_save row of the position
  int res_train_form = 0;         // the training forward's form (path states in global memory) ...
  size_t res_train_lds = 0;       // ... and its dynamic LDS
  std::vector<char> proj_ready;
  float* d_ro_in = nullptr;                     // concat scratch (multi-input readout)
  std::vector<float*> d_ro_tmp;                 // generic readout intermediates
  std::vector<RoBatchOp> ro;                    // readout ops
  std::vector<float*> ro_buf;                   // per readout tensor: op output buffer (null for states)
  std::vector<int64_t> adj_rows;                // per adjacency: edges in the batch
  std::vector<std::vector<int64_t>> adj_off;    // [adjacency][graph + 1] edge offsets
  std::vector<float*> d_norm;                   // per LayerNormalization site: its buffer in ign_forward (NormRun::buf)
  float* d_pred = nullptr;
  int64_t n_pred = 0, out_units = 1;
  int64_t edges_per_forward = 0, gru_steps = 0;
  std::vector<void*> allocs;                    // blocks of pool (returned on destroy)
  std::shared_ptr<DevPool> pool;                // the plan's (outlives the plan if need be)
  TrainState* train = nullptr;                  // ign_batch_enable_training
  uint64_t drop_seed = 0;                       // ign_batch_set_dropout: the next training forward's
  uint32_t drop_step = 0;                       // mask stream (never set: (0, 0))
  // captured ign_forward (init .. readout) for replay; the event slots it records
  hipGraphExec_t graph = nullptr;
  std::vector<int> graph_cur, graph_behind;     // cur / behind as the captured forward leaves them (each replay)
  bool graph_timing = false;
  std::vector<int> graph_kind;
  std::vector<EvCost> graph_cost;
};

namespace ign {
// the graph-resident forward (engine.cpp, resident.hip): save = the training forward's state versions
struct ResidentSave {
  float* const* path_ver;                    // [T + 1] the path entity's versions
  float* const* src_ver[kResidentMaxSrc];    // [T + 1] per source entity of the ordered MP
  float* const* hs_save;                     // [T] the ordered MP's per-step states
  float* const* x_save[kResidentMaxSrc];     // [T] per source entity: its sum MP's message sums
  float* const* tab_save = nullptr;          // [T] optional: the ordered MP's projected table per iteration
};
int resident_tables(ign_plan* p, ign_batch* b);   // once per batch; leaves b->resident false if not eligible
int resident_launch(ign_plan* p, ign_batch* b, const ResidentSave* save);
int resident_sum_mps(const ign_plan* p, int* sum_mp, int* n_src);   // 0: not a resident plan shape
// the resident ign_forward leaves MP mi out of its last iteration and marks its destination behind
inline bool skips_last(const ign_plan* p, const ign_batch* b, int mi) {
  return p->dead_last && p->mps[mi].dead_in_last_iter && !b->ext_state[p->mps[mi].dst];
}
bool env_flag(const char* name, bool dflt);   // a 0 / 1 environment switch (unset or empty: dflt)
int set_device(int dev);
int ensure_device(ign_plan* p);
int dev_alloc(ign_batch* b, float** out, int64_t n);
int repack(ign_plan* p);                      // runs p->packs: fragments from d_params (set_params, optimizer)
// what every forward / backward entry point checks first; train: the batch has its training state too
int check_pb(ign_plan* p, ign_batch* b, bool train = false);
// ign_batch_set_features / ign_batch_feature_gradients: ptr, the entity, its features, no halo rows
int check_feature_entity(const ign_plan* p, const ign_batch* b, int32_t e, const void* ptr);
// ign_batch_set_edge_params / ign_batch_edge_param_gradients: ptr, the MP, its source, a message
// network on it that reads edge_params
int check_edge_source(const ign_plan* p, const ign_batch* b, int32_t mi, int32_t s, const void* ptr);
// readout.cpp: the readout program (operations before predict, GM:611-655) and predict's head
int readout_batch(ign_plan* p, ign_batch* b, const ign_batch_desc* d);
// ent: entity-state tensors to read (training keeps every version); null = the batch's current states
// drop: the training forward's Dropout stream and buffers; null = inference (Dropout is identity)
// norm: the LayerNormalization buffers of the run; null = the batch's own (inference)
int readout_ops_run(ign_plan* p, ign_batch* b, hipStream_t st, const float* const* ent = nullptr,
                    const DropRun* drop = nullptr, const NormRun* norm = nullptr);
// the rows of readout stack `stack` (-1 predict, k readout operation k) in batch b: a site's buffer
// has that many rows of its units
int64_t stack_rows(const ign_plan* p, const ign_batch* b, int stack);
// ign_plan_add_dropout's routine (also called by ign_plan_create_json's lowering)
int plan_add_dropout(ign_plan* p, int stack, int before_layer, float rate, uint64_t layer_seed);
// ign_plan_add_layernorm's routine (likewise)
int plan_add_layernorm(ign_plan* p, int stack, int before_layer, float epsilon, int center, int scale);
// ign_plan_set_cell_options' routine (likewise)
int plan_set_cell_options(ign_plan* p, int cell, const ign_cell_options* o);
// readout tensor id (GM:660-675): an entity's final states (ent's, as readout_ops_run) or an operation's output
const float* readout_tensor(const ign_plan* p, const ign_batch* b, int id, const float* const* ent = nullptr);
// predict's input rows into *x: its one input tensor, or its inputs side by side in cat
int predict_input(const ign_plan* p, const ign_batch* b, const float* const* ent, float* cat, const float** x,
                  hipStream_t st);
// The fused readout (p->fused_readout: three Dense layers in one launch) on x into b->d_pred, on the
// kernel IGN_READOUT_VARIANT and the layers' fragments select.  save1 / save2: the hidden layers'
// activations for a backward (readout_h16 / readout_h32 only), null in inference.
struct Timer;   // mp_step.h
int readout_fused(ign_plan* p, const ign_batch* b, const float* x, float* save1, float* save2, Timer& tm,
                  hipStream_t st);
int64_t space_rows(const ign_plan* p, const ign_batch* b, const RoTensor& t);
// Batch construction (ign_batch_create, ign_batch_enable_training) copies and clears on a
// non-blocking stream of the calling host thread, never the legacy null stream: a batch built on a
// worker thread does not wait for, or serialise with, the GPU step running on the engine's stream
// (the training input pipeline overlaps them, ignnition_amd/training.py BatchPrefetcher).
hipStream_t upload_stream();
// Host -> device copies of the batch builders.  Inside an UploadScope (ign_batch_create,
// ign_batch_enable_training) a copy of up to 4 MiB goes through the thread's pinned staging arena
// and is not waited for: the scope waits once, at its end, for all of them (a builder used to wait
// for every one of ~10^2 small copies, and eight builders waiting on the runtime at once stretched
// each stage 2-4x).  Larger copies, and every copy outside a scope, are waited for at once (their
// source may die after the call).  IGN_UPLOAD_DEFER=0 waits for every copy.  IGN_BUILD_PROF=1
// prints each scope's copy count, bytes and time spent enqueueing and waiting to stderr.
hipError_t upload_bytes(void* dst, const void* src, size_t bytes);
void host_cache_stats(int64_t* live, int64_t* idle, int64_t* maps, int64_t* unmaps);
hipError_t upload_flush();   // wait for this thread's pending copies
struct UploadScope {
  explicit UploadScope(const char* what);
  ~UploadScope();
  const char* what;
  double t0;
};
template <typename T, typename A>
int dev_upload(ign_batch* b, T** out, const std::vector<T, A>& host) {
  size_t n = std::max<size_t>(host.size(), 1);
  void* p = nullptr;
  hipError_t e = pool_alloc(b->pool.get(), &p, n * sizeof(T), false);
  if (e != hipSuccess) return fail(IGN_ERR_OOM, "device alloc (%zu bytes): %s", n * sizeof(T), hipGetErrorString(e));
  b->allocs.push_back(p);
  if (!host.empty()) HIP_TRY(upload_bytes(p, host.data(), host.size() * sizeof(T)));
  else HIP_TRY(hipMemsetAsync(p, 0, sizeof(T), upload_stream()));
  *out = static_cast<T*>(p);
  return IGN_OK;
}
}  // namespace ign
