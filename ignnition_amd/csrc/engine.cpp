// engine.cpp — C ABI (include/ignmp.h), the plan's switches and repack (its lowering: plan_lower.cpp),
// native batch builder, forward driver: which states an MP instance reads and flips, the resident
// launch, capture and timing statistics.  The MP instance itself is mp_step.cpp's, predict's head
// readout.cpp's, both shared with the training forward (train.cpp).
//
// Reference behaviour restated here (generate_model.py = GM, auxilary_classes.py = AUX):
//  * hidden-state init per entity                                  GM:396-400, AUX:128-160
//  * T iterations x stages x MPs, destination state overwritten
//    after each MP (later MPs of a stage see it)                   GM:406-603
//  * per-graph dense padding semantics of the combine step:
//      lens = in-degree, Lmax = max(seq)+1 per graph and source,
//      source k's slots start after sources 0..k-1's Lmax           GM:477-543
//      interleave permutes slots through indices_<src>_to_<dst>    AUX:421-440, GM:507-519
//      sorted update consumes positions 0..final_len-1 (holes are
//      zero inputs, later positions dropped)                       AUX:767-796
//    These become per-destination step tables (CSR) built here on the host, once per batch.
//  * readout predict op (Dense stack)                              GM:611-629
// Errors the reference raises at run time (e.g. gather_nd(-1) when final_len = 0, scatter_nd
// with an out-of-range interleave index, an adjacency with no edges) are returned as
// IGN_ERR_INVALID with a message.

#include <hip/hip_runtime.h>

#include <atomic>
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ignmp.h"
#include "kernels.h"

#include "engine_internal.h"
#include "batch_lower.h"
#include "dense_stack.h"
#include "mp_step.h"
#include "train_kernels.h"

namespace ign {


thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}


int set_device(int dev) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    return fail(IGN_ERR_DEVICE, "no HIP device available (%s)", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
  if (dev < 0 || dev >= n) return fail(IGN_ERR_DEVICE, "device %d out of range (%d devices)", dev, n);
  HIP_TRY(hipSetDevice(dev));
  return IGN_OK;
}

int check_pb(ign_plan* p, ign_batch* b, bool train) {
  if (!p || !b) return fail(IGN_ERR_INVALID, "null argument");
  if (b->plan != p) return fail(IGN_ERR_INVALID, "batch was created for another plan");
  if (train && !b->train) return fail(IGN_ERR_INVALID, "training not enabled on this batch (ign_batch_enable_training)");
  if (!p->params_set) return fail(IGN_ERR_INVALID, "parameters not set (ign_plan_set_params)");
  return set_device(p->device);
}

// what ign_batch_set_features and ign_batch_feature_gradients refuse alike
int check_feature_entity(const ign_plan* p, const ign_batch* b, int32_t e, const void* ptr) {
  if (!ptr) return fail(IGN_ERR_INVALID, "null argument");
  if (e < 0 || e >= (int)p->ents.size()) return fail(IGN_ERR_INVALID, "entity %d out of range", e);
  if (p->ents[e].feature_total <= 0 || !b->d_feat[e]) return fail(IGN_ERR_INVALID, "entity %d has no features", e);
  for (int64_t h : b->halo)
    if (h)
      return fail(IGN_ERR_UNSUPPORTED, "a batch with halo rows (an edge-cut partition): a halo row's features and "
                  "their gradient belong to the partition that owns the row");
  return IGN_OK;
}

// what ign_batch_set_edge_params and ign_batch_edge_param_gradients refuse alike
int check_edge_source(const ign_plan* p, const ign_batch* b, int32_t mi, int32_t s, const void* ptr) {
  if (!ptr) return fail(IGN_ERR_INVALID, "null argument");
  if (mi < 0 || mi >= (int)p->mps.size()) return fail(IGN_ERR_INVALID, "mp index %d out of range", mi);
  const MPP& mp = p->mps[mi];
  if (s < 0 || s >= (int)mp.src.size()) return fail(IGN_ERR_INVALID, "mp %d has no source %d", mi, s);
  const MsgNN& nn = mp.nn[s];
  if (nn.layers.empty()) return fail(IGN_ERR_INVALID, "source %d of mp %d has no message network", s, mi);
  if (std::find(nn.inputs.begin(), nn.inputs.end(), (int)IGN_MSG_EDGE_PARAMS) == nn.inputs.end() ||
      !b->mp[mi].d_edge_params[s])
    return fail(IGN_ERR_INVALID, "the message network of source %d of mp %d does not read edge_params", s, mi);
  return IGN_OK;
}

int ensure_device(ign_plan* p) {
  int rc = set_device(p->device);
  if (rc) return rc;
  if (!p->stream && !p->external_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    p->own_stream = true;
  }
  if (!p->d_params) {
    HIP_TRY(hipMalloc(&p->d_params, std::max<int64_t>(p->n_params, 1) * sizeof(float)));
    HIP_TRY(hipMalloc(&p->d_packed, std::max<int64_t>(p->n_packed, 1) * sizeof(float)));
    // on the plan stream and waited for: a null-stream memset is not ordered with the
    // non-blocking plan stream and could land after ign_plan_set_params' copy
    HIP_TRY(hipMemsetAsync(p->d_params, 0, std::max<int64_t>(p->n_params, 1) * sizeof(float), p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
  }
  if (!p->pool) p->pool = pool_create(p->device);
  return IGN_OK;
}

// one non-blocking upload stream per host thread and device (a stream belongs to the device that
// was current when it was created; a thread may build batches for plans on several devices)
hipStream_t upload_stream() {
  thread_local std::vector<hipStream_t> streams;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
  if ((int)streams.size() <= dev) streams.resize(dev + 1, nullptr);
  hipStream_t& s = streams[dev];
  if (!s && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr;
  return s;
}

bool env_flag(const char* name, bool dflt) {
  const char* v = getenv(name);
  return v && *v ? atoi(v) != 0 : dflt;
}

namespace {
struct UploadState {   // per host thread and device
  char* stage = nullptr;
  size_t cap = 0, used = 0;
  int depth = 0;             // nested UploadScopes
  bool pending = false;
  int n = 0;                 // IGN_BUILD_PROF counters of the current scope
  size_t bytes = 0, staged = 0;
  double t_copy = 0, t_wait = 0;
  ~UploadState() {   // thread exit (a batch-builder thread): its copies were waited for by its scopes
    if (stage) hipHostFree(stage);
  }
};
UploadState& upload_state() {
  thread_local std::vector<std::unique_ptr<UploadState>> st;   // (owners: the arena is freed once)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
  if ((int)st.size() <= dev) st.resize(dev + 1);
  if (!st[dev]) st[dev] = std::make_unique<UploadState>();
  return *st[dev];
}
double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
constexpr size_t kStageMax = (size_t)4 << 20;   // larger copies come from pinned hvec blocks: direct DMA
}  // namespace

hipError_t upload_flush() {
  UploadState& u = upload_state();
  if (!u.pending) return hipSuccess;
  const double t = now_ms();
  const hipError_t e = hipStreamSynchronize(upload_stream());
  u.t_wait += now_ms() - t;
  u.pending = false;
  u.used = 0;
  return e;
}

hipError_t upload_bytes(void* dst, const void* src, size_t bytes) {
  const bool defer = env_flag("IGN_UPLOAD_DEFER", true);   // (read per call: tests switch it)
  UploadState& u = upload_state();
  hipStream_t us = upload_stream();
  u.n++;
  u.bytes += bytes;
  const double t = now_ms();
  hipError_t e;
  if (defer && u.depth > 0 && bytes <= kStageMax) {
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (u.used + need > u.cap) {
      if ((e = upload_flush()) != hipSuccess) return e;   // the arena's copies have landed: reuse it
      if (need > u.cap) {
        if (u.stage) hipHostFree(u.stage);
        u.stage = nullptr;
        u.cap = std::max(need, (size_t)32 << 20);
        if ((e = hipHostMalloc((void**)&u.stage, u.cap, hipHostMallocDefault)) != hipSuccess) {
          u.stage = nullptr;
          u.cap = 0;
          return e;
        }
      }
    }
    char* sp = u.stage + u.used;
    memcpy(sp, src, bytes);
    u.used += need;
    u.staged += bytes;
    u.pending = true;
    e = hipMemcpyAsync(dst, sp, bytes, hipMemcpyHostToDevice, us);
    u.t_copy += now_ms() - t;
    return e;
  }
  e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, us);
  if (e == hipSuccess) {
    u.pending = true;
    e = upload_flush();   // the source may die after the call (and the arena's copies land with it)
  }
  u.t_copy += now_ms() - t;
  return e;
}

UploadScope::UploadScope(const char* w) : what(w), t0(now_ms()) {
  UploadState& u = upload_state();
  if (u.depth++ == 0) {
    u.n = 0;
    u.bytes = u.staged = 0;
    u.t_copy = u.t_wait = 0;
  }
}

UploadScope::~UploadScope() {
  UploadState& u = upload_state();
  // every path out of a builder (errors included) leaves no copy in flight from the arena
  u.pending = true;
  upload_flush();
  if (--u.depth == 0 && env_flag("IGN_BUILD_PROF", false)) {
    int64_t live, idle, maps, unmaps;
    host_cache_stats(&live, &idle, &maps, &unmaps);
    fprintf(stderr,
            "[ign-build] %s: %.2f ms, %d copies, %.1f MB (%.1f MB staged), enqueue %.2f ms, wait %.2f ms; "
            "host blocks live %.0f MB idle %.0f MB, mapped %lld unmapped %lld\n",
            what, now_ms() - t0, u.n, u.bytes / 1e6, u.staged / 1e6, u.t_copy, u.t_wait, live / 1e6, idle / 1e6,
            (long long)maps, (long long)unmaps);
  }
}

int dev_alloc(ign_batch* b, float** out, int64_t n) {
  void* p = nullptr;
  // +256 floats of slack: kernels may read a whole (masked-off) row at index 0 of an empty table
  hipError_t e = pool_alloc(b->pool.get(), &p, (std::max<int64_t>(n, 0) + 256) * sizeof(float), true);
  if (e != hipSuccess) return fail(IGN_ERR_OOM, "device alloc (%lld floats): %s", (long long)n, hipGetErrorString(e));
  b->allocs.push_back(p);
  *out = static_cast<float*>(p);
  return IGN_OK;
}

// Per-launch algorithmic cost: one GRU application = 2*3H*(DIN+H) + 14H flops.
double gru_flops(int din, int H) { return 2.0 * 3 * H * (din + H) + 14.0 * H; }

}  // namespace ign


// Every plan-level IGN_* switch, read here once per ign_plan_create and nowhere else.
static PlanSwitches switches_from_env() {
  PlanSwitches s;
  auto flag = [](const char* name, bool* out) {
    if (const char* v = getenv(name)) *out = atoi(v) != 0;
  };
  flag("IGN_FUSE_PROJ", &s.fuse_proj);
  if (const char* v = getenv("IGN_SEQ_VARIANT")) {   // 6 (default), 4 or 2; anything else: 6
    const int sv = atoi(v);
    s.seq_variant = sv == 2 || sv == 4 ? sv : 6;
  }
  flag("IGN_HIP_GRAPH", &s.use_graph);
  flag("IGN_DEAD_LAST", &s.dead_last);
  if (const char* v = getenv("IGN_SUM_VARIANT")) s.sum_variant = atoi(v) == 7 || atoi(v) == 8 ? atoi(v) : 3;
  if (const char* v = getenv("IGN_SUM_WINDOW")) s.sum_window = atoi(v);
  if (const char* v = getenv("IGN_RESIDENT")) {   // 0 off; 1 default; 2 also force the global-path form
    s.resident = atoi(v) != 0;
    s.resident_path_global = atoi(v) == 2;
  }
  flag("IGN_RESIDENT_PG", &s.resident_pg);
  flag("IGN_RESIDENT_TRAIN", &s.resident_train);
  s.resident_eager = env_flag("IGN_RESIDENT_EAGER", true);   // (an empty value: the default)
  flag("IGN_RES_LPT", &s.res_lpt);
  if (const char* v = getenv("IGN_RES_GROUP")) s.res_group = std::max(0, atoi(v));
  flag("IGN_RESIDENT_SAVE_TABLE", &s.resident_save_table);
  flag("IGN_BWD_FUSE", &s.bwd_fuse);
  flag("IGN_SUM_BWD_FUSE", &s.sum_bwd_fuse);
  flag("IGN_DEFER_WGRAD", &s.defer_wgrad);
  flag("IGN_TRAIN_CSR_GPU", &s.train_csr_gpu);
  flag("IGN_TRAIN_DENSE_BF", &s.train_dense_bf);
  flag("IGN_TRAIN_DENSE_H16", &s.train_dense_h16);
  flag("IGN_TSGEMM_BF", &s.tsgemm_bf);
  flag("IGN_FUSE_OUTER_BWD", &s.fuse_outer_bwd);
  flag("IGN_TRAIN_FUSED_READOUT", &s.train_fused_readout);
  flag("IGN_BWD_BF", &s.bwd_bf);
  flag("IGN_TRAIN_SEQ_H16", &s.train_seq_h16);
  if (const char* v = getenv("IGN_READOUT_VARIANT")) {   // 4 (default), 5, 2 or 1; anything else: 4
    const int rv = atoi(v);
    s.readout_variant = rv == 1 || rv == 2 || rv == 5 ? rv : 4;
  }
  return s;
}

// p->packs (plan_lower.cpp's layout_packed) in order: one launch per record
int ign::repack(ign_plan* p) {
  const hipStream_t st = p->stream;
  const PackJob* const end = p->packs.data() + p->packs.size();
  for (const PackJob* j = p->packs.data(); j != end; ++j) {
    const float* s[3];
    for (int k = 0; k < 3; ++k) s[k] = j->src[k] >= 0 ? p->d_params + j->src[k] : nullptr;
    float* const dst = p->d_packed + j->dst;
    switch (j->kind) {
      case PK_GRU:   // the two records after it: its U and bias slots
        HIP_TRY(launch_pack_gru(s[0], s[1], s[2], dst, p->d_packed + j[1].dst, p->d_packed + j[2].dst, j->a, j->b, j->c, st));
        break;
      case PK_GRU_U:
      case PK_GRU_B: break;
      case PK_GRU_W: HIP_TRY(launch_pack_gru(s[0], nullptr, nullptr, dst, nullptr, nullptr, j->a, j->b, j->c, st)); break;
      case PK_U_BF16: HIP_TRY(launch_pack_u_bf16(s[0], dst, j->a, st)); break;
      case PK_U_F16: HIP_TRY(launch_pack_u_f16(s[0], dst, j->a, st)); break;
      case PK_UT_F16: HIP_TRY(launch_pack_ut_f16(s[0], dst, j->a, st)); break;
      case PK_W_F16: HIP_TRY(launch_pack_w_f16(s[0], dst, j->a, j->b, st)); break;
      case PK_W_BF16: HIP_TRY(launch_pack_w_bf16(s[0], dst, j->a, j->b, st)); break;
      case PK_A: HIP_TRY(launch_pack_a(s[0], j->a, j->b, dst, st)); break;
      case PK_DENSE_PAD: HIP_TRY(launch_pack_dense_pad(s[0], dst, j->a, j->b, j->c, st)); break;
      case PK_DENSE_BF16: HIP_TRY(launch_pack_dense_bf16(s[0], dst, j->a, j->b, j->c, st)); break;
      case PK_DENSE_BF16_T: HIP_TRY(launch_pack_dense_bf16_t(s[0], dst, j->a, j->b, st)); break;
      case PK_DENSE_F16: HIP_TRY(launch_pack_dense_f16(s[0], dst, j->a, j->b, j->c, st)); break;
      case PK_READOUT_H16: HIP_TRY(launch_pack_readout_h16(s[0], s[1], s[2], dst, j->a, j->b, j->c, st)); break;
      case PK_READOUT_H32: HIP_TRY(launch_pack_readout_h32(s[0], s[1], s[2], dst, j->a, j->b, j->c, st)); break;
      case PK_ATTN_VECTORS: HIP_TRY(launch_attn_vectors(s[0], s[1], s[2], j->a, dst, st)); break;
    }
  }
  return IGN_OK;
}

// =============================================================================================
extern "C" {

int ign_abi_version(void) { return IGN_ABI_VERSION; }

const char* ign_last_error(void) { return g_err.c_str(); }

int ign_device_count(int32_t* n) {
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (n) *n = (e == hipSuccess) ? c : 0;
  return IGN_OK;
}

int ign_plan_create(const ign_plan_desc* d, int32_t device, ign_plan** out) {
  if (!d || !out) return fail(IGN_ERR_INVALID, "null argument");
  *out = nullptr;
  std::unique_ptr<ign_plan> p(new ign_plan());
  p->device = device;
  if (int rc = lower_plan(d, switches_from_env(), p.get())) return rc;
  // Device resources are allocated on first use (ensure_device), so plan validation and the
  // parameter layout are available without a GPU.
  *out = p.release();
  return IGN_OK;
}

void ign_plan_destroy(ign_plan* p) {
  if (!p) return;
  if (!p->d_params && !p->stream) {
    delete p;
    return;
  }
  hipSetDevice(p->device);
  if (p->stream) hipStreamSynchronize(p->stream);
  for (auto e : p->ev) hipEventDestroy(e);
  if (p->d_params) hipFree(p->d_params);
  if (p->d_packed) hipFree(p->d_packed);
  if (p->d_red) hipFree(p->d_red);
  if (p->own_stream && p->stream) hipStreamDestroy(p->stream);
  delete p;
}

int ign_plan_num_params(const ign_plan* p, int64_t* n) {
  if (!p || !n) return fail(IGN_ERR_INVALID, "null argument");
  *n = p->n_params;
  return IGN_OK;
}

int ign_plan_num_param_tensors(const ign_plan* p, int32_t* n) {
  if (!p || !n) return fail(IGN_ERR_INVALID, "null argument");
  *n = (int32_t)p->tensors.size();
  return IGN_OK;
}

int ign_plan_param_tensor(const ign_plan* p, int32_t i, int32_t* kind, int32_t* owner, int64_t* offset,
                          int32_t* rows, int32_t* cols) {
  if (!p || i < 0 || i >= (int)p->tensors.size()) return fail(IGN_ERR_INVALID, "tensor index out of range");
  const Tensor& t = p->tensors[i];
  if (kind) *kind = t.kind;
  if (owner) *owner = t.owner;
  if (offset) *offset = t.offset;
  if (rows) *rows = t.rows;
  if (cols) *cols = t.cols;
  return IGN_OK;
}

int ign_plan_mp_dead_last(const ign_plan* p, int32_t mi, int32_t* dead) {
  if (!p || !dead) return fail(IGN_ERR_INVALID, "null argument");
  if (mi < 0 || mi >= (int)p->mps.size()) return fail(IGN_ERR_INVALID, "mp index %d out of range", mi);
  *dead = p->mps[mi].dead_in_last_iter;
  return IGN_OK;
}

int ign_plan_set_params(ign_plan* p, const float* params, int32_t on_device) {
  if (!p || !params) return fail(IGN_ERR_INVALID, "null argument");
  int rc = ensure_device(p);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(p->d_params, params, p->n_params * sizeof(float),
                         on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, p->stream));
  if ((rc = repack(p))) return rc;
  HIP_TRY(hipStreamSynchronize(p->stream));
  p->params_set = true;
  return IGN_OK;
}

namespace {
void drop_timing(ign_plan* p);
}  // namespace

int ign_plan_set_timing(ign_plan* p, int32_t enabled) {
  if (!p) return fail(IGN_ERR_INVALID, "null plan");
  drop_timing(p);
  p->timing = enabled != 0;
  p->stats = ign_stats_t{};
  return IGN_OK;
}

int ign_plan_set_timing_kinds(ign_plan* p, uint32_t kinds) {
  if (!p) return fail(IGN_ERR_INVALID, "null plan");
  drop_timing(p);
  p->timing_kinds = kinds;
  p->stats = ign_stats_t{};
  return IGN_OK;
}

int ign_plan_set_stream(ign_plan* p, void* s) {
  if (!p) return fail(IGN_ERR_INVALID, "null plan");
  int rc = ensure_device(p);
  if (rc) return rc;
  if ((rc = flush_timing(p))) return rc;   // pending event pairs were recorded on the old stream
  // Pooled blocks of destroyed batches carry a fence recorded on the plan's stream at destroy time;
  // from here on fences go to the new stream, so work still queued on the old one (own or external)
  // must finish before a block it reads can be handed out again.
  if (p->stream && p->stream != static_cast<hipStream_t>(s)) HIP_TRY(hipStreamSynchronize(p->stream));
  if (p->own_stream && p->stream) hipStreamDestroy(p->stream);
  p->own_stream = false;
  p->external_stream = true;
  p->stream = static_cast<hipStream_t>(s);
  return IGN_OK;
}

// ---------------------------------------------------------------------------------------------
// The graph-resident forward (resident.hip): one ordered MP into the "path" entity from S <= 2
// source entities (plain, one message per position) and, for each source entity, one sum MP from
// the paths back to it, every MP at H = DIN = 32 on the default split kernels (RouteNet: S = 1;
// Q-size: links and nodes interleaved, S = 2), on graphs whose states and projected table fit one
// workgroup's LDS.  Otherwise the batched path.
struct ResShape {
  int path = -1, n_src = 0;
  int src_ent[kResidentMaxSrc] = {-1, -1};
  int sum_mp[kResidentMaxSrc] = {-1, -1};
};

static bool resident_plan_shape(const ign_plan* p, ResShape* sh) {
  // the windowed sum (IGN_SUM_WINDOW=1) adds in another order: not restated here
  if (!p->resident || !p->fuse_proj || p->seq_variant != 6 || p->sum_variant < 7 || p->sum_window == 1) return false;
  const int n = (int)p->mps.size();
  if (n < 2 || n > kResidentMaxSrc + 1 || (int)p->ents.size() != n) return false;
  const MPP& a = p->mps[0];
  const int S = (int)a.src.size();
  if (!a.sorted || S + 1 != n || a.feature_concat || a.din != 32) return false;
  const CellP& ca = p->cells[a.cell];
  if (ca.H != 32 || ca.pk_uh < 0 || ca.pk_wbf < 0 || ca.pk_w < 0) return false;
  sh->path = a.dst;
  sh->n_src = S;
  for (int s = 0; s < S; ++s) {
    const int e = a.src[s].entity;
    if (e == a.dst || !a.nn[s].layers.empty()) return false;
    for (int t = 0; t < s; ++t)
      if (sh->src_ent[t] == e) return false;
    sh->src_ent[s] = e;
  }
  // MPs 1 .. S: one sum MP path -> each source entity, in any order (they read only the paths)
  for (int m = 1; m < n; ++m) {
    const MPP& q = p->mps[m];
    int s = -1;
    for (int t = 0; t < S; ++t)
      if (sh->src_ent[t] == q.dst) s = t;
    if (s < 0 || sh->sum_mp[s] >= 0) return false;
    if (q.sorted || q.aggr != IGN_AGGR_SUM || q.src.size() != 1 || q.src[0].entity != a.dst || q.feature_concat ||
        !q.nn[0].layers.empty() || q.din != 32)
      return false;
    const CellP& cq = p->cells[q.cell];
    if (cq.H != 32 || cq.pk_wbf < 0 || cq.pk_ubf < 0) return false;
    sh->sum_mp[s] = m;
  }
  for (int e = 0; e < n; ++e)
    if (p->ents[e].feature_total > 32 || p->ents[e].hidden_dim != 32) return false;
  return true;
}

// ---------------------------------------------------------------------------------------------
// ign_batch_create's per-MP steps: batch_lower.cpp builds an MP's host tables, these upload them (in
// a fixed order: the pool hands out its blocks by it) and keep the host copies train_alloc.cpp reads.

// message networks: per-edge rows and parameters (GM:440-475)
static int upload_message_nets(ign_batch* b, const MPP& mp, size_t mi, const BatchShape& sh, MPB& mb) {
  int rc;
  for (int s = 0; s < (int)mp.src.size(); ++s) {
    const MsgNN& nn = mp.nn[s];
    if (nn.layers.empty()) continue;
    const int a = mp.src[s].adjacency;
    hvec<int32_t> es, ed;
    if ((rc = lower_edge_rows(mp, mi, s, sh, &es, &ed))) return rc;
    const int64_t ne = (int64_t)es.size();
    mb.n_edges[s] = ne;
    if ((rc = dev_upload(b, &mb.d_edge_src[s], es)) || (rc = dev_upload(b, &mb.d_edge_dst[s], ed))) return rc;
    if (std::find(nn.inputs.begin(), nn.inputs.end(), (int)IGN_MSG_EDGE_PARAMS) != nn.inputs.end()) {
      hvec<float> prm(sh.d->adj_params[a], sh.d->adj_params[a] + ne * nn.param_dim);
      if ((rc = dev_upload(b, &mb.d_edge_params[s], prm))) return rc;
    }
    if ((rc = dev_alloc(b, &mb.d_msg_in[s], ne * nn.din_pad))) return rc;
    HIP_TRY(hipMemsetAsync(mb.d_msg_in[s], 0, ne * nn.din_pad * sizeof(float), upload_stream()));   // zero padding columns
    for (auto& dp : nn.layers) {
      float* f = nullptr;
      if ((rc = dev_alloc(b, &f, ne * dp.out))) return rc;
      mb.d_msg_layer[s].push_back(f);
    }
  }
  return IGN_OK;
}

static int build_ordered_mp(ign_batch* b, const MPP& mp, int H, const BatchShape& sh, const MsgLists& ml, BuildMarks& bm,
                            MPB& mb) {
  OrderedTables t;
  int rc = lower_ordered(mp, H, sh, ml, bm, &t);
  if (rc) return rc;
  mb.src_off = std::move(t.src_off);
  mb.src_rows = std::move(t.src_rows);
  mb.zero_row = t.zero_row;
  mb.n_multi = t.n_multi;
  mb.wave_steps = t.wave_steps;
  mb.n_steps = t.n_steps;
  mb.n_msgs = t.n_msgs;
  mb.flops = t.flops;
  mb.bytes = t.bytes;
  if ((rc = dev_upload(b, &mb.d_seq_hdr, t.hdr)) || (rc = dev_upload(b, &mb.d_order, t.order)) ||
      (rc = dev_upload(b, &mb.d_len, t.len)) || (rc = dev_upload(b, &mb.d_step_ptr, t.step_ptr)) ||
      (rc = dev_upload(b, &mb.d_step_code, t.step_code)) || (rc = dev_upload(b, &mb.d_multi_ptr, t.multi_ptr)) ||
      (rc = dev_upload(b, &mb.d_multi_rows, t.multi_rows)))
    return rc;
  mb.h_order = std::move(t.order);
  mb.h_len = std::move(t.len);
  mb.h_step_ptr = std::move(t.step_ptr);
  mb.h_step_code = std::move(t.step_code);
  mb.h_multi_ptr = std::move(t.multi_ptr);
  mb.h_multi_rows = std::move(t.multi_rows);
  const int64_t tfloats = (mb.zero_row + 1 + mb.n_multi) * 3LL * H;
  if ((rc = dev_alloc(b, &mb.d_table, tfloats))) return rc;
  HIP_TRY(hipMemsetAsync(mb.d_table, 0, (tfloats + 256) * sizeof(float), upload_stream()));   // zero row stays zero
  b->gru_steps += mb.n_steps * b->plan->T;
  bm.mark("uploads");
  return IGN_OK;
}

static int build_sum_mp(ign_batch* b, const MPP& mp, size_t mi, int H, const BatchShape& sh, const MsgLists& ml,
                        BuildMarks& bm, MPB& mb) {
  const int64_t ND = mb.n_dst;
  const int DIN = mp.din;
  int rc;
  SumCsr csr;
  lower_sum_csr(mp, sh, ml, bm, &csr);
  mb.n_interior = csr.n_interior;
  if (mp.aggr == IGN_AGGR_ATTENTION) {
    AttnTables at;
    lower_attention(mp, sh, ml, csr, &at);
    mb.n_groups = at.n_groups;
    mb.n_cells = at.n_cells;
    if ((rc = dev_upload(b, &mb.d_group_ptr, at.group_ptr)) || (rc = dev_upload(b, &mb.d_group_empty, at.group_empty)) ||
        (rc = dev_upload(b, &mb.d_cell_dst, at.cell_dst)) || (rc = dev_upload(b, &mb.d_cell_ptr, at.cell_ptr)) ||
        (rc = dev_upload(b, &mb.d_cell_msgs, at.cell_msgs)))
      return rc;
    if ((rc = dev_alloc(b, &mb.d_msg_w, (int64_t)ml.mdst.size())) || (rc = dev_alloc(b, &mb.d_ecell, mb.n_cells)) ||
        (rc = dev_alloc(b, &mb.d_s_dst, ND)))
      return rc;
    for (int s = 0; s < (int)mp.src.size(); ++s)
      if ((rc = dev_alloc(b, &mb.d_s_src[s], source_rows(mp, s, sh)))) return rc;
  }
  bm.mark("csr");
  SumAgg ag;
  if ((rc = lower_sum_agg(mp, mi, b->plan->sum_window, sh, ml, csr, &ag))) return rc;
  mb.n_win_wg = ag.n_win_wg;
  mb.sum_seg = ag.seg;
  mb.n_seg = ag.n_seg;
  if (ag.window && ((rc = dev_upload(b, &mb.d_win_wg, ag.wg)) || (rc = dev_upload(b, &mb.d_win_dst, ag.wdst)) ||
                    (rc = dev_upload(b, &mb.d_win_ptr, ag.wptr)) || (rc = dev_upload(b, &mb.d_win_src, ag.wsrc))))
    return rc;
  if ((ag.window || ag.seg) &&
      ((rc = dev_upload(b, &mb.d_id_ptr, ag.id_ptr)) || (rc = dev_upload(b, &mb.d_id_src, ag.id_src)) ||
       (rc = dev_alloc(b, &mb.d_xsum, std::max<int64_t>(ND, 1) * DIN))))
    return rc;
  mb.n_msgs = (int64_t)csr.msrc.size();
  if ((rc = dev_upload(b, &mb.d_order, csr.order)) || (rc = dev_upload(b, &mb.d_msg_ptr, csr.ptr)) ||
      (rc = dev_upload(b, &mb.d_msg_src, csr.msrc)))
    return rc;
  mb.h_order = std::move(csr.order);
  mb.h_msg_ptr = std::move(csr.ptr);
  mb.h_msg_src = std::move(csr.msrc);
  mb.flops = (double)ND * gru_flops(DIN, H) + (double)mb.n_msgs * DIN;
  mb.bytes = (double)mb.n_msgs * (4.0 * DIN + 4) + (double)ND * (8.0 * H + 8);
  b->gru_steps += ND * b->plan->T;
  return IGN_OK;
}

int ign_batch_create(ign_plan* p, const ign_batch_desc* d, ign_batch** out) {
  if (!p || !d || !out) return fail(IGN_ERR_INVALID, "null argument");
  *out = nullptr;
  p->batch_made = true;   // the plan's Dropout sites are final from this call on (ign_plan_add_dropout)
  const int G = d->num_graphs;
  const int E = (int)p->ents.size();
  if (G <= 0) return fail(IGN_ERR_INVALID, "num_graphs must be > 0");
  int rc = ensure_device(p);
  if (rc) return rc;
  UploadScope scope("ign_batch_create");
  std::unique_ptr<ign_batch, void (*)(ign_batch*)> b(new ign_batch(), ign_batch_destroy);
  b->plan = p;
  b->pool = p->pool;
  b->G = G;
  BatchShape sh;
  if ((rc = lower_batch_shape(E, p->n_adj, p->n_il, p->mps, d, &sh))) return rc;
  b->rows = sh.rows;
  b->halo = sh.halo;
  b->row_off = sh.row_off;

  // features + state buffers
  b->d_feat.assign(E, nullptr);
  b->d_state[0].assign(E, nullptr);
  b->d_state[1].assign(E, nullptr);
  b->cur.assign(E, 0);
  b->behind.assign(E, -1);
  b->ext_state.assign(E, 0);
  for (int e = 0; e < E; ++e) {
    const int H = p->ents[e].hidden_dim, F = p->ents[e].feature_total;
    if (F > 0) {
      if (!d->features || !d->features[e]) return fail(IGN_ERR_INVALID, "entity %d: features missing", e);
      hvec<float> f(d->features[e], d->features[e] + b->rows[e] * F);
      if ((rc = dev_upload(b.get(), &b->d_feat[e], f))) return rc;
    }
    const int64_t sr = (b->rows[e] + b->halo[e]) * H;
    for (int k = 0; k < 2; ++k) {
      if ((rc = dev_alloc(b.get(), &b->d_state[k][e], sr))) return rc;
      if (b->halo[e]) HIP_TRY(hipMemsetAsync(b->d_state[k][e], 0, sr * sizeof(float), upload_stream()));   // halo defined before use
    }
  }

  // per-MP CSR / step tables: each MP is lowered on the host (batch_lower.cpp), then uploaded, so
  // its staged copies run under the next MP's host work
  static const bool build_prof = env_flag("IGN_BUILD_PROF", false);
  std::vector<double> t_mp;   // IGN_BUILD_PROF: the time up to the end of each MP's tables
  const double t_mp0 = build_prof ? now_ms() : 0.0;
  BuildMarks bm(env_flag("IGN_BUILD_PROF_FINE", false));   // IGN_BUILD_PROF_FINE=1: finer sections of each MP
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {
    if (build_prof && mi > 0) t_mp.push_back(now_ms());
    const MPP& mp = p->mps[mi];
    MPB mb;
    mb.sorted = mp.sorted;
    mb.n_dst = b->rows[mp.dst];
    MsgLists ml;
    if ((rc = lower_messages(mp, sh, &ml)) || (rc = upload_message_nets(b.get(), mp, mi, sh, mb))) return rc;
    bm.mark("messages");
    mb.edges = ml.tot;
    b->edges_per_forward += ml.tot * p->T;
    const int H = p->cells[mp.cell].H;
    if ((rc = mp.sorted ? build_ordered_mp(b.get(), mp, H, sh, ml, bm, mb)
                        : build_sum_mp(b.get(), mp, mi, H, sh, ml, bm, mb)))
      return rc;
    b->mp.push_back(std::move(mb));
  }

  // readout buffers (the resident forward's tables are built by the first ign_forward: a batch that
  // only trains or steps MP by MP never pays for them)
  bm.mark("mp-rest");
  if ((rc = readout_batch(p, b.get(), d))) return rc;
  bm.mark("readout");
  const int64_t P = space_rows(p, b.get(), p->ro_t[p->ro_in[0]]);
  b->n_pred = P;
  b->out_units = p->dense.back().out;
  if (p->ro_in.size() > 1 && (rc = dev_alloc(b.get(), &b->d_ro_in, P * p->ro_width))) return rc;
  if (!p->fused_readout) {
    for (size_t l = 0; l + 1 < p->dense.size(); ++l) {
      float* t = nullptr;
      if ((rc = dev_alloc(b.get(), &t, P * p->dense[l].out))) return rc;
      b->d_ro_tmp.push_back(t);
    }
  }
  if ((rc = dev_alloc(b.get(), &b->d_pred, P * b->out_units))) return rc;
  for (size_t s = 0; s < p->norms.size(); ++s) {   // one buffer per LayerNormalization layer (readout ops and predict)
    float* t = nullptr;
    if ((rc = dev_alloc(b.get(), &t, std::max<int64_t>(1, stack_rows(p, b.get(), p->norms[s].stack) * p->norms[s].units))))
      return rc;
    b->d_norm.push_back(t);
  }
  // the resident tables here, on the building thread, not at the first forward: a training loop's
  // builders run ahead of the step, and the step's thread would otherwise build them inside the step
  // (fresh 512 x synth50 batches: 28 -> 56 ms per step once the training forward went resident)
  const double t_res0 = build_prof ? now_ms() : 0.0;
  if (p->resident_eager && (rc = resident_tables(p, b.get()))) return rc;
  if (build_prof) {
    std::string s;
    double prev = t_mp0;
    for (size_t i = 0; i < t_mp.size(); ++i) {
      s += " mp" + std::to_string(i) + " " + std::to_string(t_mp[i] - prev).substr(0, 6);
      prev = t_mp[i];
    }
    fprintf(stderr, "[ign-build] batch sections:%s mp%zu+readout %.2f, resident tables %.2f ms\n", s.c_str(),
            t_mp.size(), t_res0 - prev, now_ms() - t_res0);
  }
  bm.mark("alloc+resident");
  bm.print("ign_batch_create fine");
  HIP_TRY(hipStreamSynchronize(upload_stream()));   // every clear has landed before the batch is used
  HIP_TRY(upload_flush());                           // (and every staged copy)
  *out = b.release();
  return IGN_OK;
}

void ign_batch_destroy(ign_batch* b) {
  if (!b) return;
  static const bool prof = env_flag("IGN_BUILD_PROF", false);
  const double t0 = prof ? now_ms() : 0.0;
  if (b->plan) {
    hipSetDevice(b->plan->device);
    // With the block cache every released block carries an event recorded on the plan stream
    // (pool_release), so the host need not wait here and the next step can be queued behind this
    // one.  Without it (IGN_POOL=0) pool_release waits itself; a captured graph is destroyed only
    // once its launches have finished.
    if (b->plan->stream && (b->graph || !pool_enabled(b->pool.get()))) hipStreamSynchronize(b->plan->stream);
  }
  if (b->graph) hipGraphExecDestroy(b->graph);
  const double t1 = prof ? now_ms() : 0.0;
  if (b->train) train_state_destroy(b->train);
  const double t2 = prof ? now_ms() : 0.0;
  if (b->pool) pool_release(b->pool.get(), b->allocs, b->plan ? b->plan->stream : nullptr);
  const double t3 = prof ? now_ms() : 0.0;
  delete b;
  if (prof)
    fprintf(stderr, "[ign-build] ign_batch_destroy: %.2f ms (sync %.2f, training state %.2f, blocks %.2f, host %.2f)\n",
            now_ms() - t0, t1 - t0, t2 - t1, t3 - t2, now_ms() - t3);
}

int ign_plan_trim_cache(ign_plan* p) {
  if (!p) return fail(IGN_ERR_INVALID, "null argument");
  if (p->pool) pool_trim_idle(p->pool.get());
  host_cache_trim();
  return IGN_OK;
}

int ign_batch_info(const ign_batch* b, ign_batch_info_t* o) {
  if (!b || !o) return fail(IGN_ERR_INVALID, "null argument");
  std::memset(o, 0, sizeof(*o));
  o->num_graphs = b->G;
  o->predictions = b->n_pred;
  o->output_units = b->out_units;
  o->edges_per_forward = b->edges_per_forward;
  o->gru_steps_per_forward = b->gru_steps;
  for (size_t e = 0; e < b->rows.size() && e < 8; ++e) o->rows[e] = b->rows[e];
  return IGN_OK;
}

int ign_batch_resident_info(const ign_batch* b, ign_resident_info_t* o) {
  if (!b || !o) return fail(IGN_ERR_INVALID, "null argument");
  *o = b->resident ? b->res_info : ign_resident_info_t{};
  return IGN_OK;
}

int ign_batch_predictions(ign_batch* b, const float** ptr) {
  if (!b || !ptr) return fail(IGN_ERR_INVALID, "null argument");
  *ptr = b->d_pred;
  return IGN_OK;
}

// ---------------------------------------------------------------------------------------------
int ign_forward_begin(ign_plan* p, ign_batch* b) {
  int rc = check_pb(p, b);
  if (rc) return rc;
  Timer tm{p};
  for (int e = 0; e < (int)p->ents.size(); ++e) {   // GM:396-400 (owned rows; halo rows come from peers)
    const int H = p->ents[e].hidden_dim, F = p->ents[e].feature_total;
    tm.begin(K_INIT, 0, (double)b->rows[e] * (4.0 * F + 4.0 * H));
    HIP_TRY(launch_init_state(b->d_state[0][e], b->d_feat[e], b->rows[e], H, F, p->stream));
    tm.end();
    b->cur[e] = 0;
    b->behind[e] = -1;
  }
  return IGN_OK;
}

namespace {

// MP instance mi on the batch's current states (ign_forward_mp's work)
int forward_mp(ign_plan* p, ign_batch* b, int32_t mi, int32_t part) {
  const MPP& mp = p->mps[mi];
  const int dst = mp.dst;
  MpStates s;
  for (size_t k = 0; k < mp.src.size(); ++k) {
    const int se = mp.src[k].entity;
    s.src.base[k] = b->d_state[b->cur[se]][se];
  }
  s.hin = b->d_state[b->cur[dst]][dst];
  s.hout = b->d_state[1 - b->cur[dst]][dst];
  Timer tm{p};
  if (int rc = mp_forward(p, b, mi, part, s, MpSave{}, tm)) return rc;
  if (part != IGN_PART_INTERIOR) b->cur[dst] ^= 1;   // GM:602: the destination state is overwritten
  return IGN_OK;
}

// Entity e's states as a forward that runs every MP leaves them: where ign_forward left the last
// iteration's update of e out (b->behind), it runs now, once, on the plan's stream and outside any
// captured graph, through the same MP step from the same inputs -- nothing the MP reads has changed
// since (mark_dead_last) -- so the states are the eager forward's bits, on the batched and on the
// resident route (whose rows are the batched forward's bits).
int finish_entity(ign_plan* p, ign_batch* b, int e) {
  const int mi = b->behind[e];
  if (mi < 0) return IGN_OK;
  if (int rc = check_pb(p, b)) return rc;
  if (int rc = forward_mp(p, b, mi, IGN_PART_ALL)) return rc;
  b->behind[e] = -1;
  return IGN_OK;
}

}  // namespace

int ign_forward_mp(ign_plan* p, ign_batch* b, int32_t mi, int32_t part) {
  int rc = check_pb(p, b);
  if (rc) return rc;
  if (mi < 0 || mi >= (int)p->mps.size()) return fail(IGN_ERR_INVALID, "mp index %d out of range", mi);
  if (part < IGN_PART_ALL || part > IGN_PART_BOUNDARY) return fail(IGN_ERR_INVALID, "part %d", part);
  // stepping on after an ign_forward: from the states every MP of that forward leaves
  for (int e = 0; e < (int)p->ents.size(); ++e)
    if ((rc = finish_entity(p, b, e))) return rc;
  return forward_mp(p, b, mi, part);
}

namespace {

int accumulate_stats(ign_plan* p, int n, const int* kind, const EvCost* cost) {
  HIP_TRY(hipStreamSynchronize(p->stream));
  ign_stats_t& s = p->stats;
  s.kinds = K_KINDS;
  for (int i = 0; i < n; ++i) {
    float ms = 0;
    hipEventElapsedTime(&ms, p->ev[2 * i], p->ev[2 * i + 1]);
    s.launches[kind[i]] += 1;
    s.ms[kind[i]] += ms;
    s.flops[kind[i]] += cost[i].flops;
    s.bytes[kind[i]] += cost[i].bytes;
    s.mfma_bf16[kind[i]] += cost[i].mfma_bf16;
    s.mfma_f32[kind[i]] += cost[i].mfma_f32;
  }
  return IGN_OK;
}

// Forget the pending event pairs (the statistics are being reset).
void drop_timing(ign_plan* p) {
  if (p->ev_slot && p->stream) hipStreamSynchronize(p->stream);
  p->ev_slot = 0;
}

// readout launches (GM:611-629); no host synchronisation, so it can be captured
int readout(ign_plan* p, ign_batch* b) {
  hipStream_t st = p->stream;
  Timer tm{p};
  const int64_t P = b->n_pred;
  if (!p->ro_ops.empty()) {
    tm.begin(K_OTHER, 0, 0);
    int rc = readout_ops_run(p, b, st);
    tm.end();
    if (rc) return rc;
  }
  const float* x = nullptr;
  if (int rc = predict_input(p, b, nullptr, b->d_ro_in, &x, st)) return rc;
  const float* prm = p->d_params;
  if (p->fused_readout) {
    if (int rc = readout_fused(p, b, x, nullptr, nullptr, tm, st)) return rc;
  } else {
    const float* in = x;
    int in_stride = p->ro_width;
    // predict's layers in order, a Dropout being the identity here; the LayerNormalization layers
    // as dense_stack_forward runs them: each in front of a Dense layer writes its own buffer, and from
    // the last Dense layer on each layer writes the next one's buffer, the last d_pred
    const std::vector<StackLayer>& seq = p->seq;
    bool tail = false;
    for (size_t i = 0; i < seq.size(); ++i) {
      const StackLayer& e = seq[i];
      if (e.kind == SL_DROPOUT) continue;
      tail = tail || (e.kind == SL_DENSE && e.idx + 1 == (int)p->dense.size());
      size_t nx = i + 1;   // (tail) the next LayerNormalization
      while (tail && nx < seq.size() && seq[nx].kind != SL_LAYERNORM) ++nx;
      float* o = !tail ? (e.kind == SL_DENSE ? b->d_ro_tmp[e.idx] : b->d_norm[e.idx])
                       : nx < seq.size() ? b->d_norm[seq[nx].idx] : b->d_pred;
      if (e.kind == SL_DENSE) {
        const DenseP& dl = p->dense[e.idx];
        tm.begin(K_READOUT, 2.0 * P * dl.in * dl.out, (double)P * 4.0 * (dl.in + dl.out));
        HIP_TRY(launch_dense_generic(in, P, dl.in, in_stride, prm + dl.off_w, dl.use_bias ? prm + dl.off_b : nullptr,
                                     dl.out, dl.act, o, st));
        tm.end();
        in_stride = dl.out;
      } else {
        const int units = p->norms[e.idx].units;
        tm.begin(K_READOUT, 8.0 * P * units, 2.0 * (double)P * 4.0 * units);
        HIP_TRY(norm_fwd(p, e.idx, in, in_stride, P, o, nullptr, st));
        tm.end();
        in_stride = units;
      }
      in = o;
    }
  }
  return IGN_OK;
}

int copy_out(ign_plan* p, ign_batch* b, float* pred_out) {
  if (pred_out) {
    HIP_TRY(hipMemcpyAsync(pred_out, b->d_pred, b->n_pred * b->out_units * sizeof(float), hipMemcpyDeviceToHost,
                           p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
  }
  return IGN_OK;
}

}  // namespace

// Resolve the pending event pairs of timed launches into the statistics (one host wait).
extern "C++" int ign::flush_timing(ign_plan* p) {
  if (p->ev_slot == 0) return IGN_OK;
  const int n = p->ev_slot;
  p->ev_slot = 0;
  return accumulate_stats(p, n, p->ev_kind.data(), p->ev_cost.data());
}

// the whole MP loop of a resident batch in one launch; the final states land in
// buffer 0 of every entity, or (save: the training forward) in the state versions save names
extern "C++" int ign::resident_launch(ign_plan* p, ign_batch* b, const ResidentSave* save) {
  ResShape sh;
  if (!resident_plan_shape(p, &sh)) return fail(IGN_ERR_RUNTIME, "resident batch on a plan of another shape");
  const MPP& a = p->mps[0];
  const CellP& ca = p->cells[a.cell];
  const int path = sh.path;
  ResidentArgs r{};
  r.path_off = b->d_res_path_off;
  r.urow_off = b->d_res_urow_off;
  r.ptile_off = b->d_res_ptile_off;
  r.hdr = b->d_res_hdr;
  r.lcode_off = b->d_res_lcode_off;
  r.lcode = b->d_res_lcode;
  r.lmsg_off = b->d_res_lmsg_off;
  r.lmsg_ptr = b->d_res_lmsg_ptr;
  r.lmsg_src = b->d_res_lmsg_src;
  r.lorder = b->d_res_lorder;
  r.lnseg = b->d_res_lnseg;
  r.gorder = p->res_lpt ? b->d_res_gorder : nullptr;
  r.path_feat = b->d_feat[path];
  r.path_F = p->ents[path].feature_total;
  r.path_state = b->d_state[0][path];
  r.n_src = sh.n_src;
  for (int s = 0; s < sh.n_src; ++s) {
    const int e = sh.src_ent[s];
    const CellP& cs = p->cells[p->mps[sh.sum_mp[s]].cell];
    r.src_off[s] = b->d_res_src_off[s];
    r.src_feat[s] = b->d_feat[e];
    r.src_F[s] = p->ents[e].feature_total;
    r.src_state[s] = b->d_state[0][e];
    r.sWbf[s] = p->d_packed + cs.pk_wbf;
    r.sUbf[s] = p->d_packed + cs.pk_ubf;
    r.sum_bias[s] = p->d_packed + cs.pk_b;
  }
  r.Uh = p->d_packed + ca.pk_uh;
  r.seq_bias = p->d_packed + ca.pk_b;
  r.proj_W = p->d_packed + ca.pk_wbf;
  r.proj_b = p->d_packed + ca.pk_b;
  r.proj_Wf = p->d_packed + ca.pk_w;
  r.T = p->T;
  r.seg_on = save ? 0 : 1;   // the training forward's sums are all lane walks (sum_gru_g32 with x_save)
  // the last iteration's sum updates nothing reads (the training forward keeps them: its backward
  // reads every saved version)
  for (int s = 0; s < sh.n_src && !save; ++s)
    if (skips_last(p, b, sh.sum_mp[s])) r.dead_last |= 1 << s;
  if (save) {
    r.path_ver = save->path_ver;
    r.hs_save = save->hs_save;
    r.hsb = b->d_res_hsb;
    r.tab_save = save->tab_save;
    r.tab_hole = b->mp[0].zero_row;
    for (int s = 0; s < sh.n_src; ++s) r.tab_off[s] = b->mp[0].src_off[s];
    for (int s = 0; s < sh.n_src; ++s) {
      r.src_ver[s] = save->src_ver[s];
      r.x_save[s] = save->x_save[s];
    }
  }
  const ign_resident_info_t& ri = save ? b->res_info_full : b->res_info;
  Timer tm{p};
  tm.begin(K_RESIDENT, ri.flops, ri.bytes_stage, ri.mfma_bf16, ri.mfma_f32);
  HIP_TRY(launch_resident_forward(r, b->res_graphs, save ? b->res_train_lds : b->res_lds, save ? b->res_train_form : b->res_form,
                                  save != nullptr, p->stream));
  tm.end();
  if (!save) {
    b->cur[path] = 0;
    b->behind[path] = -1;
    for (int s = 0; s < sh.n_src; ++s) {
      b->cur[sh.src_ent[s]] = 0;
      b->behind[sh.src_ent[s]] = r.dead_last >> s & 1 ? sh.sum_mp[s] : -1;
    }
  }
  return IGN_OK;
}

static_assert(kResMaxSrc == kResidentMaxSrc && (int)kResAllLds == (int)IGN_RES_ALL_LDS &&
              (int)kResPathGlobal == (int)IGN_RES_PATH_GLOBAL && (int)kResPathCsrGlobal == (int)IGN_RES_PATH_CSR_GLOBAL,
              "batch_lower.h and kernels.h disagree");

static int resident_upload(ign_batch* b, const ResidentTables& t, int S) {
  HIP_TRY(resident_prepare_device());
  int rc;
  for (int s = 0; s < S; ++s)
    if ((rc = dev_upload(b, &b->d_res_src_off[s], t.src_off[s]))) return rc;
  if ((rc = dev_upload(b, &b->d_res_path_off, t.path_off)) || (rc = dev_upload(b, &b->d_res_urow_off, t.urow_off)) ||
      (rc = dev_upload(b, &b->d_res_ptile_off, t.ptile_off)) || (rc = dev_upload(b, &b->d_res_hdr, t.hdr)) ||
      (rc = dev_upload(b, &b->d_res_lmsg_off, t.lmsg_off)) || (rc = dev_upload(b, &b->d_res_lmsg_ptr, t.lmsg_ptr)) ||
      (rc = dev_upload(b, &b->d_res_lmsg_src, t.lmsg_src)) || (rc = dev_upload(b, &b->d_res_lorder, t.lorder)) ||
      (rc = dev_upload(b, &b->d_res_lnseg, t.lnseg)) || (rc = dev_upload(b, &b->d_res_lcode_off, t.lcode_off)) ||
      (rc = dev_upload(b, &b->d_res_hsb, t.hsb)) || (rc = dev_upload(b, &b->d_res_gorder, t.gorder)) ||
      (rc = dev_upload(b, &b->d_res_lcode, t.lcode)))
    return rc;
  b->res_train_form = t.train_form;
  b->res_train_lds = t.lds[t.train_form];
  b->res_lds = t.lds[t.form];
  b->res_form = t.form;
  b->res_graphs = t.G;
  b->res_info = t.info;
  b->res_info_full = t.info_full;
  b->resident = true;
  return IGN_OK;
}

// the per-graph tables of the resident forward; leaves b->resident false where it does not apply
// (built on the host for each K, and only the set that runs is uploaded.)  IGN_RES_GROUP=K: K graphs per workgroup.  Auto (0): two where the all-LDS form of a single graph fits
// twice (NSFNET x512: 0.248-0.257 -> 0.203-0.208 ms/step, r06_c07; GEANT2's path states need the
// path-global form at two per workgroup, measured slower: 0.548 -> 0.570), else one
static int resident_batch(ign_plan* p, ign_batch* b) {
  ResShape sh;
  if (!resident_plan_shape(p, &sh)) return IGN_OK;
  ResidentParams rp;
  rp.path = sh.path;
  rp.n_src = sh.n_src;
  rp.T = p->T;
  rp.sum_window = p->sum_window;
  rp.path_global_ok = p->resident_pg;
  rp.force_path_global = p->resident_path_global;
  rp.max_tiles = kResidentMaxTiles;
  rp.state_stride = kResidentStateStride;
  rp.table_stride = kResidentTableStride;
  rp.max_dyn_lds = kResidentMaxDynLds;
  for (auto& e : p->ents) rp.feature_total.push_back(e.feature_total);
  const MPB& a = b->mp[0];
  const ResOrderedIn ma{a.h_order, a.h_len, a.h_step_ptr, a.h_step_code, a.src_off, a.zero_row, a.n_multi, a.n_steps,
                        a.flops, a.bytes};
  std::vector<ResSumIn> sums;
  for (int s = 0; s < sh.n_src; ++s) {
    rp.src_ent[s] = sh.src_ent[s];
    rp.dead_last[s] = skips_last(p, b, sh.sum_mp[s]);
    const MPB& m = b->mp[sh.sum_mp[s]];
    sums.push_back(ResSumIn{m.h_order, m.h_msg_ptr, m.h_msg_src, m.flops, m.bytes});
  }
  const BatchRows rows{b->G, b->row_off, b->rows, b->halo};
  ResidentTables one;
  lower_resident(rp, p->res_group > 0 ? p->res_group : 1, rows, ma, sums, &one);
  if (!one.eligible) return IGN_OK;
  if (p->res_group == 0 && one.form == IGN_RES_ALL_LDS && b->G >= 2 && 2 * one.lds[one.form] <= kResidentMaxDynLds) {
    // two graphs per workgroup, where they lower; a failed upload falls back to the single-graph
    // tables (its blocks stay with the batch until it goes)
    ResidentTables two;
    lower_resident(rp, 2, rows, ma, sums, &two);
    if (two.eligible && resident_upload(b, two, sh.n_src) == IGN_OK) return IGN_OK;
  }
  return resident_upload(b, one, sh.n_src);
}

// the batch's resident tables, built once (the first ign_forward or training forward)
extern "C++" int ign::resident_tables(ign_plan* p, ign_batch* b) {
  if (b->res_tried) return IGN_OK;
  b->res_tried = true;
  return resident_batch(p, b);
}

// MPs 1 .. S of a resident plan: the sum MP back to each source entity of MP 0 (s order)
extern "C++" int ign::resident_sum_mps(const ign_plan* p, int* sum_mp, int* n_src) {
  ResShape sh;
  if (!resident_plan_shape(p, &sh)) return 0;
  *n_src = sh.n_src;
  for (int s = 0; s < sh.n_src; ++s) sum_mp[s] = sh.sum_mp[s];
  return 1;
}

namespace {

int forward_body(ign_plan* p, ign_batch* b) {
  if (b->resident) {
    const int rc = resident_launch(p, b, nullptr);
    return rc ? rc : readout(p, b);
  }
  int rc = ign_forward_begin(p, b);
  if (rc) return rc;
  b->proj_ready.assign(p->mps.size(), 0);
  b->fuse_ok = p->fuse_proj;
  for (int it = 0; it < p->T && !rc; ++it) {            // GM:406
    b->fuse_last_iter = it + 1 == p->T;
    // every MP of every iteration, a dead last update included (the resident launch alone leaves
    // those out): T launches per MP is what the per-kind launch statistics of this route state
    for (int mi = 0; mi < (int)p->mps.size() && !rc; ++mi)   // GM:410-414 (stages flattened in order)
      rc = forward_mp(p, b, mi, IGN_PART_ALL);
  }
  b->fuse_ok = false;
  return rc ? rc : readout(p, b);
}

// Capture the whole forward (init, T x MPs, readout; HIP event records included when timing is
// on) into one hipGraph per batch.  The null stream cannot be captured: no graph there.
int capture(ign_plan* p, ign_batch* b) {
  if (b->graph) {
    hipGraphExecDestroy(b->graph);
    b->graph = nullptr;
  }
  if (!p->stream) return IGN_ERR_UNSUPPORTED;
  hipGraph_t g = nullptr;
  HIP_TRY(hipStreamBeginCapture(p->stream, hipStreamCaptureModeThreadLocal));
  int rc = forward_body(p, b);
  hipError_t e = hipStreamEndCapture(p->stream, &g);
  if (rc || e != hipSuccess || !g) {
    if (g) hipGraphDestroy(g);
    hipGetLastError();
    return rc ? rc : fail(IGN_ERR_DEVICE, "hipStreamEndCapture: %s", hipGetErrorString(e));
  }
  e = hipGraphInstantiate(&b->graph, g, nullptr, nullptr, 0);
  hipGraphDestroy(g);
  if (e != hipSuccess) {
    b->graph = nullptr;
    return fail(IGN_ERR_DEVICE, "hipGraphInstantiate: %s", hipGetErrorString(e));
  }
  b->graph_timing = p->timing;
  b->graph_cur = b->cur;
  b->graph_behind = b->behind;
  const int n = p->timing ? p->ev_slot : 0;
  b->graph_kind.assign(p->ev_kind.begin(), p->ev_kind.begin() + n);
  b->graph_cost.assign(p->ev_cost.begin(), p->ev_cost.begin() + n);
  p->ev_slot = 0;
  return IGN_OK;
}

}  // namespace

int ign_forward_end(ign_plan* p, ign_batch* b, float* pred_out) {
  int rc = check_pb(p, b);
  if (rc) return rc;
  if ((rc = readout(p, b))) return rc;
  return copy_out(p, b, pred_out);   // timed launches stay pending until ign_stats (flush_timing)
}

int ign_forward(ign_plan* p, ign_batch* b, float* pred_out) {
  int rc = check_pb(p, b);
  if (rc) return rc;
  if ((rc = resident_tables(p, b))) return rc;   // before any capture: the tables are uploaded here
  // HIP event records captured into a graph report 0 ms on this runtime, so timed forwards
  // launch directly; untimed ones replay the captured graph
  if (p->use_graph && p->stream && !p->timing) {
    if (!b->graph) {
      if ((rc = capture(p, b))) {
        p->use_graph = false;        // not capturable here: run the launches directly from now on
        b->graph = nullptr;
        return ign_forward(p, b, pred_out);
      }
    }
    HIP_TRY(hipGraphLaunch(b->graph, p->stream));
    b->cur = b->graph_cur;   // where the captured launches leave the states (a finish_entity since
    b->behind = b->graph_behind;   // the capture moved an entity's slot), and which are behind again
    if ((rc = copy_out(p, b, pred_out))) return rc;
    if (p->timing)
      return accumulate_stats(p, (int)b->graph_kind.size(), b->graph_kind.data(), b->graph_cost.data());
    return IGN_OK;
  }
  if ((rc = forward_body(p, b))) return rc;
  // the event pairs stay pending (no host wait per forward, so the next forward queues behind
  // this one); ign_stats resolves them
  return copy_out(p, b, pred_out);
}

int ign_batch_read_predictions(ign_plan* p, ign_batch* b, float* host_out) {
  int rc = check_pb(p, b);
  if (rc) return rc;
  if (!host_out) return fail(IGN_ERR_INVALID, "null argument");
  return copy_out(p, b, host_out);
}

int ign_batch_set_features(ign_plan* p, ign_batch* b, int32_t e, const float* rows) {
  int rc = check_pb(p, b);
  if (rc || (rc = check_feature_entity(p, b, e, rows))) return rc;
  if (b->train && train_step_open(b->train))
    return fail(IGN_ERR_INVALID, "ign_batch_set_features between a training forward and the end of its backward "
                "(the saved states belong to the old values)");
  // Nothing else of the batch is derived from feature values: every forward builds h0 from this buffer
  // (launch_init_state, the resident forward's path_feat / src_feat), the captured graph included, which
  // holds the pointer.  One copy in the plan's stream order; a device source is not waited for
  const size_t bytes = (size_t)b->rows[e] * p->ents[e].feature_total * sizeof(float);
  hipPointerAttribute_t at{};
  const bool dev = hipPointerGetAttributes(&at, rows) == hipSuccess &&
                   (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged);
  if (!dev) (void)hipGetLastError();   // (an unregistered host pointer is an error to the query)
  HIP_TRY(hipMemcpyAsync(b->d_feat[e], rows, bytes, hipMemcpyDefault, p->stream));
  if (!dev) HIP_TRY(hipStreamSynchronize(p->stream));   // the caller's host rows may die after the call
  return IGN_OK;
}

int ign_batch_set_edge_params(ign_plan* p, ign_batch* b, int32_t mi, int32_t s, const float* rows) {
  int rc = check_pb(p, b);
  if (rc || (rc = check_edge_source(p, b, mi, s, rows))) return rc;
  if (b->train && train_step_open(b->train))
    return fail(IGN_ERR_INVALID, "ign_batch_set_edge_params between a training forward and the end of its backward "
                "(the saved states belong to the old values)");
  // Nothing else of the batch is derived from parameter values: every forward gathers the network's
  // input rows from this buffer (mp_message_nets), the captured graph included, which holds the
  // pointer.  A halo batch too: a partition owns its in-edges and their rows whole.  One copy in the
  // plan's stream order; a device source is not waited for
  const MPB& mb = b->mp[mi];
  const size_t bytes = (size_t)mb.n_edges[s] * p->mps[mi].nn[s].param_dim * sizeof(float);
  if (!bytes) return IGN_OK;
  hipPointerAttribute_t at{};
  const bool dev = hipPointerGetAttributes(&at, rows) == hipSuccess &&
                   (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged);
  if (!dev) (void)hipGetLastError();   // (an unregistered host pointer is an error to the query)
  HIP_TRY(hipMemcpyAsync(mb.d_edge_params[s], rows, bytes, hipMemcpyDefault, p->stream));
  if (!dev) HIP_TRY(hipStreamSynchronize(p->stream));   // the caller's host rows may die after the call
  return IGN_OK;
}

int ign_batch_mp_split(const ign_batch* b, int32_t mi, int64_t* interior, int64_t* boundary) {
  if (!b || !interior || !boundary) return fail(IGN_ERR_INVALID, "null argument");
  if (mi < 0 || mi >= (int)b->mp.size()) return fail(IGN_ERR_INVALID, "mp index %d out of range", mi);
  const MPB& mb = b->mp[mi];
  *interior = mb.sorted ? mb.n_dst : mb.n_interior;
  *boundary = mb.n_dst - *interior;
  return IGN_OK;
}

int ign_batch_bind_state(ign_plan* p, ign_batch* b, int32_t e, float* dev0, float* dev1, int64_t capacity) {
  if (!p || !b || !dev0 || !dev1) return fail(IGN_ERR_INVALID, "null argument");
  if (b->plan != p) return fail(IGN_ERR_INVALID, "batch was created for another plan");
  if (e < 0 || e >= (int)p->ents.size()) return fail(IGN_ERR_INVALID, "entity index");
  const int64_t need = (b->rows[e] + b->halo[e]) * p->ents[e].hidden_dim + 256;
  if (capacity < need) return fail(IGN_ERR_INVALID, "state buffers hold %lld floats, need %lld",
                                   (long long)capacity, (long long)need);
  if ((reinterpret_cast<uintptr_t>(dev0) | reinterpret_cast<uintptr_t>(dev1)) & 15)
    return fail(IGN_ERR_INVALID, "state buffers must be 16-byte aligned");
  b->d_state[0][e] = dev0;
  b->d_state[1][e] = dev1;
  b->cur[e] = 0;
  // the caller reads these buffers itself and cannot ask for a left-out update: from here on every
  // MP into e runs in every iteration (skips_last)
  b->ext_state[e] = 1;
  b->behind[e] = -1;
  return IGN_OK;
}

int ign_batch_state_slot(const ign_batch* b, int32_t e, int32_t* slot) {
  if (!b || !slot) return fail(IGN_ERR_INVALID, "null argument");
  if (e < 0 || e >= (int)b->cur.size()) return fail(IGN_ERR_INVALID, "entity index");
  *slot = b->cur[e];
  return IGN_OK;
}

int ign_gather_rows(ign_plan* p, const float* src, int64_t ld, const int32_t* idx, int64_t n, int32_t cols,
                    float* dst) {
  if (!p) return fail(IGN_ERR_INVALID, "null plan");
  if (n < 0 || cols <= 0 || cols % 4 || ld < cols || ld % 4) return fail(IGN_ERR_INVALID, "gather_rows shape");
  if (n && (!src || !idx || !dst)) return fail(IGN_ERR_INVALID, "null argument");
  int rc = ensure_device(p);
  if (rc) return rc;
  HIP_TRY(launch_gather_rows(src, ld, idx, n, cols, dst, p->stream));
  return IGN_OK;
}

int ign_synchronize(ign_plan* p) {
  if (!p) return fail(IGN_ERR_INVALID, "null plan");
  int rc = ensure_device(p);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(p->stream));
  return IGN_OK;
}

int ign_batch_state(ign_plan* p, ign_batch* b, int32_t e, float* host_out) {
  if (!p || !b || !host_out) return fail(IGN_ERR_INVALID, "null argument");
  if (e < 0 || e >= (int)p->ents.size()) return fail(IGN_ERR_INVALID, "entity index");
  int rc = set_device(p->device);
  if (rc) return rc;
  if (b->plan != p) return fail(IGN_ERR_INVALID, "batch was created for another plan");
  if ((rc = finish_entity(p, b, e))) return rc;   // the last iteration's update, if ign_forward left it out
  HIP_TRY(hipMemcpyAsync(host_out, b->d_state[b->cur[e]][e], b->rows[e] * p->ents[e].hidden_dim * sizeof(float),
                         hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return IGN_OK;
}

int ign_stats(const ign_plan* p, ign_stats_t* out) {
  if (!p || !out) return fail(IGN_ERR_INVALID, "null argument");
  int rc = flush_timing(const_cast<ign_plan*>(p));   // the plan's own bookkeeping; the ABI keeps const
  if (rc) return rc;
  *out = p->stats;
  return IGN_OK;
}

}  // extern "C"
