// jacobian_common.h — what the two passes over the linearised forward share on the host
// (jacobian.cpp: K feature directions, adjoint.cpp: K prediction cotangents): the scratch of one call
// and the scope of the linearising kernels; and what the scenario passes (scenario.cpp, scenario_adjoint.cpp)
// share with them: the scenario kernels' scope, the adjoints' layout check and index upload.  `what` names
// the pass in every message.
#pragma once
#include "jacobian.h"
#include "mp_step.h"

namespace ign {

// scratch of one call (IGN_POOL_POISON=1 fills the blocks with NaN): no kernel of the pass may read what
// no kernel of the pass wrote
struct JacScratch {
  ign_batch* b;
  hipStream_t st;
  const char* what;
  std::vector<void*> blocks;
  ~JacScratch() {
    if (!blocks.empty()) pool_release(b->pool.get(), blocks, st);
  }
  // n floats (+ slack: a masked-off row 0 of an empty table may be read)
  int get(float** out, int64_t n) {
    void* q = nullptr;
    const size_t bytes = (size_t)(std::max<int64_t>(n, 0) + 256) * sizeof(float);
    const hipError_t e = pool_alloc(b->pool.get(), &q, bytes, true);
    if (e != hipSuccess) return fail(IGN_ERR_OOM, "%s: device alloc (%zu bytes): %s", what, bytes, hipGetErrorString(e));
    blocks.push_back(q);
    *out = static_cast<float*>(q);
    return IGN_OK;
  }
};

// what the linearised kernels do not cover, by name
inline int jac_check_scope(const ign_plan* p, const ign_batch* b, const char* what) {
  auto refuse = [&](const char* text) { return fail(IGN_ERR_UNSUPPORTED, "%s: %s", what, text); };
  for (int64_t h : b->halo)
    if (h) return refuse("a batch with halo rows (an edge-cut partition)");
  if (b->train && train_step_open(b->train))
    return refuse("a training step is open (between a training forward and the end of its backward)");
  for (const MPP& mp : p->mps) {
    if (mp.aggr == IGN_AGGR_ATTENTION) return refuse("attention aggregation");
    if (mp.aggr == IGN_AGGR_CONVOLUTION) return refuse("convolution aggregation");
    if (mp.feature_concat) return refuse("concat on axis 2");
    for (const MsgNN& nn : mp.nn)
      if (!nn.layers.empty()) return refuse("a message network (message-creation layers on an MP source)");
    const CellP& cp = p->cells[mp.cell];
    if (!cp.reset_after) return refuse("a GRU cell with reset_after = false (its candidate needs a second dependent sweep)");
    if (gru_wide_supported(mp.din, cp.H)) return refuse("the 128/128 GRU shape");
    if (mp.din != cp.din || !jacobian_shape_supported(mp.din, cp.H) || (mp.sorted && !jacobian_shape_supported(cp.H, cp.H)))
      return fail(IGN_ERR_UNSUPPORTED, "%s: GRU shape %d / %d", what, mp.din, cp.H);
  }
  if (!p->ro_ops.empty()) return refuse("a readout operation before predict");
  if (!p->norms.empty()) return refuse("LayerNormalization");
  return IGN_OK;
}

// what the scenario-major kernels do not cover, by name (scenario.cpp, scenario_adjoint.cpp): default cells only
inline int scen_check_scope(const ign_plan* p, const ign_batch* b, const char* what) {
  auto refuse = [&](const char* text) { return fail(IGN_ERR_UNSUPPORTED, "%s: %s", what, text); };
  for (int64_t h : b->halo)
    if (h) return refuse("a batch with halo rows (an edge-cut partition)");
  if (b->train && train_step_open(b->train))
    return refuse("a training step is open (between a training forward and the end of its backward)");
  for (const MPP& mp : p->mps) {
    if (mp.aggr == IGN_AGGR_ATTENTION) return refuse("attention aggregation");
    if (mp.aggr == IGN_AGGR_CONVOLUTION) return refuse("convolution aggregation");
    if (mp.feature_concat) return refuse("concat on axis 2");
    for (const MsgNN& nn : mp.nn)
      if (!nn.layers.empty()) return refuse("a message network (message-creation layers on an MP source)");
    const CellP& cp = p->cells[mp.cell];
    if (!cp.is_default()) return refuse("a GRU cell with options (ign_plan_set_cell_options)");
    if (gru_wide_supported(mp.din, cp.H)) return refuse("the 128/128 GRU shape");
    if (mp.din != cp.din || !scen_sum_supported(mp.din, cp.H) || (mp.sorted && !scen_seq_supported(cp.H)))
      return fail(IGN_ERR_UNSUPPORTED, "%s: GRU shape %d / %d", what, mp.din, cp.H);
  }
  if (!p->ro_ops.empty()) return refuse("a readout operation before predict");
  if (!p->norms.empty()) return refuse("LayerNormalization");
  return IGN_OK;
}

// what the flat layouts of the two adjoint passes assume of a plan inside their scope
inline int adj_check_layout(const ign_plan* p, const ign_batch* b, const char* what) {
  const int n_ents = (int)p->ents.size();
  for (const MPP& mp : p->mps)
    for (const auto& src : mp.src)
      if (p->ents[src.entity].hidden_dim != mp.din)
        return fail(IGN_ERR_UNSUPPORTED, "%s: a source %d wide on an MP input of %d", what, p->ents[src.entity].hidden_dim, mp.din);
  for (int id : p->ro_in)
    if (id < 0 || id >= n_ents || b->rows[id] != b->n_pred || p->ro_t[id].width != p->ents[id].hidden_dim)
      return fail(IGN_ERR_UNSUPPORTED, "%s: predict does not read one row of entity states per prediction", what);
  if (!p->dense.empty() && p->dense[0].in != p->ro_width)
    return fail(IGN_ERR_UNSUPPORTED, "%s: predict's first layer reads %d of %d input columns", what, p->dense[0].in, p->ro_width);
  return IGN_OK;
}

// a host index table into a scratch block
inline int jac_upload_i32(JacScratch& sc, const hvec<int32_t>& h, int32_t** out) {
  float* f = nullptr;
  if (int rc = sc.get(&f, (int64_t)h.size())) return rc;
  *out = reinterpret_cast<int32_t*>(f);
  if (!h.empty()) HIP_TRY(upload_bytes(f, h.data(), h.size() * sizeof(int32_t)));
  return IGN_OK;
}

struct JacRawCell {   // pack_gru's unscaled form of one cell, packed once per call from the live parameters
  float *W = nullptr, *U = nullptr, *b = nullptr;
};

}  // namespace ign
