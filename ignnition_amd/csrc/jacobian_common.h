// jacobian_common.h — what the two passes over the linearised forward share on the host
// (jacobian.cpp: K feature directions, adjoint.cpp: K prediction cotangents): the scratch of one call
// and the scope of the linearising kernels.  `what` names the pass in every message.
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

struct JacRawCell {   // pack_gru's unscaled form of one cell, packed once per call from the live parameters
  float *W = nullptr, *U = nullptr, *b = nullptr;
};

}  // namespace ign
