// train.cpp — the training step behind the C ABI: model_fn's TRAIN branch
// (code/utils/generate_model.py:697-830 = GM).
//
//   ign_forward_train   the forward of ComnetModel.call (GM:384-658), keeping what the backward
//                       needs: every hidden-state version (no ping-pong), the per-step states of
//                       each ordered update, the aggregated messages of each sum update, and
//                       the readout activations.  Each MP instance is the inference forward's
//                       routine (mp_step.cpp's mp_forward) given the buffers to save into, and
//                       predict's head readout.cpp's; here are the versions and the records
//   ign_backward        tf.gradients(total_loss, trainable_variables) (GM:790) for a given
//                       dLoss/dpredictions, plus the Dense l2 regularizer terms (AUX:833-834)
// The loss, the regularizer's value and the optimizer update around them are learn.cpp; the state
// these entry points run on is train_state.h's, built by train_alloc.cpp (ign_batch_enable_training).
//
// Backward schedule: readout Dense stack in reverse, then the MP instances of the forward in
// reverse order (mp_backward.cpp).  Per entity one gradient buffer tracks dLoss/d(current version);
// an MP turns the gradient of its output version into that of its input version (GRU backward) and
// adds the message gradients to its sources.  Weight gradients are row-contractions
// (tsgemm_add) reduced in a fixed order: the result is deterministic.

#include <hip/hip_runtime.h>

#include <vector>

#include "dense_stack.h"
#include "mp_backward.h"
#include "mp_step.h"
#include "readout_kernels.h"
#include "train_kernels.h"
#include "train_state.h"

bool train_step_open(const TrainState* t) { return t->f_open || t->forward_done || t->b_open; }

int ign::check_train(ign_plan* p, ign_batch* b) { return check_pb(p, b, true); }

namespace {

// the gradient of readout tensor id (GM:660-675): an entity's final states or an operation's output
float* ro_grad(TrainState* t, int id) { return id < (int)t->ver.size() ? t->dS[0][id] : t->dT[id]; }

// Backward of a readout Dense stack r (predict's, an operation's) from d(y) in dy: d(x) is added to
// the one input's gradient, or written to cat_grad and split by columns over the inputs (concat axis 1)
int ro_stack_backward(ign_plan* p, TrainState* t, DenseStackRun r, const float* dy, float* const* gz,
                      const std::vector<int>& in, float* cat_grad, hipStream_t st) {
  r.dy = dy;
  r.gz = gz;
  r.part = t->part;
  r.grads = t->grads;
  r.l2_scale = &t->l2_scale;
  r.dx_acc = in.size() == 1;
  r.dx = r.dx_acc ? ro_grad(t, in[0]) : cat_grad;
  if (int rc = dense_stack_backward(p, r, st)) return rc;
  int col = 0;
  for (size_t q = 0; !r.dx_acc && q < in.size(); ++q) {
    const int w = p->ro_t[in[q]].width;
    HIP_TRY(launch_split_cols_add(ro_grad(t, in[q]), r.n, w, cat_grad, r.ldx, col, st));
    col += w;
  }
  return IGN_OK;
}

// predict's Dense stack (p->dense) on input x, for the training forward and its backward
DenseStackRun predict_stack(const ign_plan* p, const ign_batch* b, TrainState* t, const float* x) {
  return {p->dense.data(), (int)p->dense.size(), b->n_pred, x, p->ro_width, t->act.data(), b->d_pred, &t->drop, &p->seq,
          &t->norm};
}

// Backward of the readout operations before predict (GM:605-655), last first: each turns the
// gradient of its output tensors (t->dT) into additions to its inputs' gradients
int readout_ops_backward(ign_plan* p, ign_batch* b, TrainState* t, hipStream_t st) {
  int rc;
  const float* const* ent = t->ent.data();   // the forward's entity tensors
  int xi = (int)t->rx_ptr.size();   // extend CSRs are stored in op order, two per op
  for (int k = (int)p->ro_ops.size() - 1; k >= 0; --k) {
    const RoOp& op = p->ro_ops[k];
    const RoBatchOp& bo = b->ro[k];
    const RoTensor& t0 = p->ro_t[op.in[0]];
    const int64_t n = space_rows(p, b, t0);
    switch (op.type) {
      case IGN_RO_NEURAL_NETWORK: {   // Readout_nn (AUX:1188-1211): Dense stack on concat(inputs)
        const float* x = op.in.size() > 1 ? bo.cat : readout_tensor(p, b, op.in[0], ent);
        const DenseStackRun r{op.layers.data(), (int)op.layers.size(), n, x, op.in_width, bo.tmp.data(), bo.out[0],
                              &t->drop, &op.seq, &t->norm};
        if ((rc = ro_stack_backward(p, t, r, t->dT[op.out], t->rz, op.in, t->rcat, st))) return rc;
        break;
      }
      case IGN_RO_POOLING:   // Pooling_operation (AUX:1165-1185)
        HIP_TRY(launch_pool_bwd(readout_tensor(p, b, op.in[0], ent), bo.out[0], t->dT[op.out], t->rties, t0.width,
                                bo.d_inoff, b->G, op.mode, n, ro_grad(t, op.in[0]), st));
        break;
      case IGN_RO_PRODUCT: {   // element_wise (AUX:1081-1088)
        const RoTensor& t1 = p->ro_t[op.in[1]];
        const RoTensor& to = p->ro_t[op.out];
        const int ag = t0.space == RS_GRAPH && to.space != RS_GRAPH, bg = t1.space == RS_GRAPH && to.space != RS_GRAPH;
        HIP_TRY(launch_product_bwd(t->dT[op.out], readout_tensor(p, b, op.in[1], ent), t0.width, t1.width, to.width, ag,
                                   bg, bo.d_seg, b->G, n, ro_grad(t, op.in[0]), st));
        HIP_TRY(launch_product_bwd(t->dT[op.out], readout_tensor(p, b, op.in[0], ent), t1.width, t0.width, to.width, bg,
                                   ag, bo.d_seg, b->G, space_rows(p, b, t1), ro_grad(t, op.in[1]), st));
        break;
      }
      case IGN_RO_EXTEND: {   // Extend_adjacencies (AUX:1236-1265): gathers, so scatter back per row
        xi -= 2;
        for (int j = 0; j < 2; ++j) {
          const RoTensor& tj = p->ro_t[op.in[j]];
          HIP_TRY(launch_csr_gather_cols_add(ro_grad(t, op.in[j]), space_rows(p, b, tj), t->rx_ptr[xi + j],
                                             t->rx_idx[xi + j], t->dT[op.out + j], tj.width, 0, tj.width, 1, st));
        }
        break;
      }
    }
  }
  return IGN_OK;
}

}  // namespace

extern "C" {

int ign_forward_train_begin(ign_plan* p, ign_batch* b) {
  int rc = check_train(p, b);
  if (rc) return rc;
  TrainState* t = b->train;
  hipStream_t st = p->stream;
  const int E = (int)p->ents.size();
  for (int e = 0; e < E; ++e) {   // GM:396-400 (owned rows; an edge-cut driver fills the halo rows)
    HIP_TRY(launch_init_state(t->ver[e][0], b->d_feat[e], b->rows[e], p->ents[e].hidden_dim,
                              p->ents[e].feature_total, st));
    t->cur[e] = 0;
  }
  t->recs.clear();
  t->tab_saved = false;
  t->f_it = t->f_mi = 0;
  t->f_open = true;
  t->forward_done = false;
  t->b_open = false;   // (a backward left unfinished is abandoned with its forward)
  t->backward_done = false;
  return IGN_OK;
}

int ign_forward_train_mp(ign_plan* p, ign_batch* b) {
  int rc = check_train(p, b);
  if (rc) return rc;
  TrainState* t = b->train;
  if (!t->f_open || t->f_it >= p->T) return fail(IGN_ERR_INVALID, "ign_forward_train_mp outside begin .. end");
  const int it = t->f_it, mi = t->f_mi;
  const MPP& mp = p->mps[mi];
  const MPTrain& mt = t->mp[mi];
  MPRec rec{mi, it, t->cur[mp.dst], {0, 0, 0, 0}};
  MpStates s;
  for (size_t k = 0; k < mp.src.size(); ++k) {
    const int se = mp.src[k].entity;
    rec.src_v[k] = t->cur[se];
    s.src.base[k] = t->ver[se][t->cur[se]];
  }
  s.hin = t->ver[mp.dst][rec.v_in];
  s.hout = t->ver[mp.dst][rec.v_in + 1];
  MpSave save;   // what ign_backward_mp reads of this instance
  if (mp.sorted) save.hs = mt.hs[it];
  else save.x = mt.xs[it];
  if (!mp.sorted && mp.aggr == IGN_AGGR_CONVOLUTION) save.sum = mt.ss[it];   // AUX:384-401
  Timer untimed{nullptr};
  if ((rc = mp_forward(p, b, mi, IGN_PART_ALL, s, save, untimed))) return rc;
  t->cur[mp.dst] = rec.v_in + 1;
  t->recs.push_back(rec);
  if (++t->f_mi == (int)p->mps.size()) {
    t->f_mi = 0;
    ++t->f_it;
  }
  return IGN_OK;
}

int ign_forward_train_end(ign_plan* p, ign_batch* b, float* pred_out) {
  int rc = check_train(p, b);
  if (rc) return rc;
  TrainState* t = b->train;
  if (!t->f_open || t->f_it != p->T) return fail(IGN_ERR_INVALID, "ign_forward_train_end before every MP ran");
  t->f_open = false;
  hipStream_t st = p->stream;
  // readout operations, then the predict stack with every activation kept (GM:605-629)
  for (size_t e = 0; e < t->ent.size(); ++e) t->ent[e] = t->ver[e][t->cur[e]];
  // this forward's Dropout masks (ign_batch_set_dropout), kept for the backward that regenerates them
  t->drop = DropRun{b->drop_seed, b->drop_step, t->dbuf.data()};
  t->norm = NormRun{t->nbuf.data(), t->nstats.data()};
  if (!p->ro_ops.empty() && (rc = readout_ops_run(p, b, st, t->ent.data(), &t->drop, &t->norm))) return rc;
  const int64_t P = b->n_pred;
  const float* x = nullptr;
  if ((rc = predict_input(p, b, t->ent.data(), t->ro_x, &x, st))) return rc;
  // the inference readout kernel (readout_h16 / _h32, as readout_fused picks it) with its activations
  // written out: one launch, no re-read of layer 1's output; its two saving kernels, three Dense layers only
  // (a stack with a Dropout site runs layer by layer: the mask sits between two of its launches)
  // A plan with a cell with options keeps forward's bits in its training forward: where its
  // inference readout is the f32 readout3 (no split pieces: a predict input of 16 columns, or
  // IGN_READOUT_VARIANT=1), that kernel's saving form runs here too.  A plan of default cells keeps its
  // layer-by-layer stack there.
  const bool split = p->dense.size() == 3 && p->readout_variant >= 2 && p->dense[0].pk_bf >= 0 && p->dense[1].pk_bf >= 0;
  const bool fused = p->train_fused_readout && p->fused_readout && p->dense.size() == 3 &&
                     ((p->readout_variant >= 4 && p->dense[1].pk_h >= 0 && split) || (p->any_cell_options && !split)) &&
                     p->dense[0].use_bias && p->dense[1].use_bias && p->seq.size() == p->dense.size();
  Timer untimed{nullptr};
  if ((rc = fused ? readout_fused(p, b, x, t->act[0], t->act[1], untimed, st)
                  : dense_stack_forward(p, predict_stack(p, b, t, x), st)))
    return rc;
  if (pred_out) {
    HIP_TRY(hipMemcpyAsync(pred_out, b->d_pred, P * b->out_units * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  t->forward_done = true;
  return IGN_OK;
}

// The training forward's whole MP loop as one graph-resident launch (resident.hip's SAVE form,
// DESIGN.md §3d) where the plan and batch allow it: the same states, per-step saves, message sums and
// versions as ign_forward_train_mp's launches, and the same MP-instance records for the backward
static int resident_train_forward(ign_plan* p, ign_batch* b, bool* done) {
  *done = false;
  int sum_mp[kResidentMaxSrc] = {-1, -1}, S = 0;
  // the resident form computes the ordered update with seq_gru_h16's arithmetic and leaves each
  // sequence's first and final state rows unsaved (the path versions hold them): only under the
  // backward that recomputes those gates and reads neither row (the fused split-fp16 one; the unfused
  // one contracts every hs row)
  // (the training form keeps its path states in global memory: IGN_RESIDENT_PG=0 turns it off too)
  if (!p->resident_train || !p->resident_pg || !resident_sum_mps(p, sum_mp, &S) || train_seq_variant(p, 32) != 6)
    return IGN_OK;
  int rc = resident_tables(p, b);
  if (rc || !b->resident) return rc;
  TrainState* t = b->train;
  const int path = p->mps[0].dst, T = p->T;
  int src_ent[kResidentMaxSrc] = {-1, -1};
  for (int s = 0; s < S; ++s) src_ent[s] = p->mps[0].src[s].entity;
  if ((int)t->ver[path].size() != T + 1) return IGN_OK;
  for (int s = 0; s < S; ++s)
    if ((int)t->ver[src_ent[s]].size() != T + 1) return IGN_OK;
  // pointer arrays: path versions [T + 1] | per source: versions [T + 1] | hs_save [T] | per source:
  // x_save [T] | the ordered MP's projected tables [T] (saved for the backward: no recompute)
  const int64_t n_ptr = (T + 1) * (1 + S) + T * (1 + S) + T;
  const MPB& m0 = b->mp[0];
  const bool save_tab = p->resident_save_table && m0.n_multi == 0;
  if (!t->res_ptrs) {
    for (int k = 0; k < T && save_tab; ++k) {
      float* f = nullptr;
      if ((rc = talloc(t, &f, (m0.zero_row + 1) * 3 * p->cells[p->mps[0].cell].H))) return rc;
      t->tsave.push_back(f);
    }
    hvec<float*> v;
    for (int k = 0; k <= T; ++k) v.push_back(t->ver[path][k]);
    for (int s = 0; s < S; ++s)
      for (int k = 0; k <= T; ++k) v.push_back(t->ver[src_ent[s]][k]);
    for (int k = 0; k < T; ++k) v.push_back(t->mp[0].hs[k]);
    for (int s = 0; s < S; ++s)
      for (int k = 0; k < T; ++k) v.push_back(t->mp[sum_mp[s]].xs[k]);
    for (int k = 0; k < T; ++k) v.push_back(save_tab ? t->tsave[k] : nullptr);
    if ((int64_t)v.size() != n_ptr) return fail(IGN_ERR_RUNTIME, "resident training pointers");
    if ((rc = tupload(t, &t->res_ptrs, v))) return rc;
  }
  ResidentSave sv{};
  sv.path_ver = t->res_ptrs;
  for (int s = 0; s < S; ++s) sv.src_ver[s] = t->res_ptrs + (T + 1) * (1 + s);
  sv.hs_save = t->res_ptrs + (T + 1) * (1 + S);
  for (int s = 0; s < S; ++s) sv.x_save[s] = t->res_ptrs + (T + 1) * (1 + S) + T * (1 + s);
  if (!t->tsave.empty()) sv.tab_save = t->res_ptrs + (T + 1) * (1 + S) + T * (1 + S);
  if ((rc = resident_launch(p, b, &sv))) return rc;
  t->tab_saved = !t->tsave.empty();
  // the records ign_forward_train_mp would have left (GM:404-603 order)
  for (int it = 0; it < T; ++it)
    for (int mi = 0; mi < (int)p->mps.size(); ++mi) {
      const MPP& mp = p->mps[mi];
      MPRec rec{mi, it, t->cur[mp.dst], {0, 0, 0, 0}};
      for (size_t s = 0; s < mp.src.size(); ++s) rec.src_v[s] = t->cur[mp.src[s].entity];
      t->cur[mp.dst] = rec.v_in + 1;
      t->recs.push_back(rec);
    }
  t->f_it = T;
  t->f_mi = 0;
  *done = true;
  return IGN_OK;
}

int ign_forward_train(ign_plan* p, ign_batch* b, float* pred_out) {
  int rc = ign_forward_train_begin(p, b);
  bool done = false;
  if (!rc) rc = resident_train_forward(p, b, &done);
  for (int k = 0; !rc && !done && k < p->T * (int)p->mps.size(); ++k) rc = ign_forward_train_mp(p, b);
  return rc ? rc : ign_forward_train_end(p, b, pred_out);
}

int ign_backward_begin(ign_plan* p, ign_batch* b, const float* dpred, float* grads, float l2_scale) {
  int rc = check_train(p, b);
  if (rc) return rc;
  if (!dpred || !grads) return fail(IGN_ERR_INVALID, "null argument");
  TrainState* t = b->train;
  if (!t->forward_done)
    return fail(IGN_ERR_INVALID, "ign_backward needs a preceding ign_forward_train (a backward consumes the "
                "forward's saved activations: one backward per forward)");
  // the readout backward below may write gradient rows over the saved activations (fuse_outer_bwd):
  // a second backward of the same forward would read them as activations
  t->forward_done = false;
  t->backward_done = false;
  hipStream_t st = p->stream;
  const int E = (int)p->ents.size();
  set_tsgemm_bf(p->tsgemm_bf);
  HIP_TRY(hipMemsetAsync(grads, 0, p->n_params * sizeof(float), st));
  t->grads = grads;
  t->l2_scale = l2_scale;
  for (auto& d : t->defer) d.used = 0;   // (a backward that failed part-way leaves no stale partials)
  for (auto& d : t->defer_seq) d.used = 0;
  t->dcur.assign(E, 0);
  for (int e = 0; e < E; ++e)   // owned and halo rows (edge-cut: peers' gradients arrive in the owned rows)
    HIP_TRY(hipMemsetAsync(t->dS[0][e], 0, (b->rows[e] + b->halo[e]) * p->ents[e].hidden_dim * sizeof(float), st));
  for (size_t id = 0; id < t->dT.size(); ++id)
    if (t->dT[id])
      HIP_TRY(hipMemsetAsync(t->dT[id], 0, space_rows(p, b, p->ro_t[id]) * p->ro_t[id].width * sizeof(float), st));
  t->edge_grads_live = t->edge_grads;
  if (t->edge_grads_live)
    for (size_t mi = 0; mi < p->mps.size(); ++mi)
      for (size_t s = 0; s < p->mps[mi].src.size(); ++s)
        if (t->mp[mi].dprm[s] && b->mp[mi].n_edges[s])
          HIP_TRY(hipMemsetAsync(t->mp[mi].dprm[s], 0,
                                 b->mp[mi].n_edges[s] * p->mps[mi].nn[s].param_dim * sizeof(float), st));

  // ---- readout (GM:605-629) in reverse: predict, then the operations before it
  const float* x = p->ro_in.size() > 1 ? t->ro_x : readout_tensor(p, b, p->ro_in[0], t->ent.data());
  if ((rc = ro_stack_backward(p, t, predict_stack(p, b, t, x), dpred, t->dz, p->ro_in, t->dro, st)) ||
      (rc = readout_ops_backward(p, b, t, st)))
    return rc;
  t->b_ri = (int)t->recs.size() - 1;
  t->b_open = true;
  return IGN_OK;
}

// the backward of the forward's last MP instance not yet undone (mp_backward.cpp): dLoss/d(its output
// version) in the destination's current gradient buffer becomes dLoss/d(its input version) in the other
int ign_backward_mp(ign_plan* p, ign_batch* b) {
  int rc = check_train(p, b);
  if (rc) return rc;
  TrainState* t = b->train;
  if (!t->b_open || t->b_ri < 0) return fail(IGN_ERR_INVALID, "ign_backward_mp outside begin .. end");
  const MPRec& rec = t->recs[t->b_ri--];
  if ((rc = mp_backward(p, b, t, rec))) return rc;
  const int dst = p->mps[rec.mi].dst;
  t->dcur[dst] = 1 - t->dcur[dst];
  return IGN_OK;
}

int ign_backward_end(ign_plan* p, ign_batch* b) {
  int rc = check_train(p, b);
  if (rc) return rc;
  TrainState* t = b->train;
  if (!t->b_open || t->b_ri >= 0) return fail(IGN_ERR_INVALID, "ign_backward_end before every MP instance ran");
  t->b_open = false;
  hipStream_t st = p->stream;
  float* grads = t->grads;
  if ((rc = tsgemm_deferred_flush(p, t, st))) return rc;
  for (auto& mp : p->mps)   // message-network l2 terms (AUX:833-834), once per step
    for (auto& nn : mp.nn)
      for (auto& d : nn.layers)
        if ((rc = add_l2_grad(p, d, grads, t->l2_scale, st))) return rc;
  t->backward_done = true;
  return IGN_OK;
}

// dLoss/d(feature values) of entity e after a completed backward.  Every MP instance of the backward
// turns the gradient of its destination's output version into that of its input version (dh_out, all
// H columns, whether or not a parameter gradient needs it) and adds its message gradients to its
// sources' buffers, down to iteration 0: at ign_backward_end the entity's current gradient buffer
// is dLoss/dh0, and h0 = [features | zeros] (launch_init_state), so its first F columns are the answer
int ign_batch_feature_gradients(ign_plan* p, ign_batch* b, int32_t e, float* dev_out) {
  int rc = check_train(p, b);
  if (rc || (rc = check_feature_entity(p, b, e, dev_out))) return rc;
  const TrainState* t = b->train;
  if (!t->backward_done)
    return fail(IGN_ERR_INVALID, "ign_batch_feature_gradients needs a completed backward of this batch (ign_backward "
                "or ign_backward_end after its ign_forward_train)");
  HIP_TRY(launch_slice_cols(t->dS[t->dcur[e]][e], b->rows[e], p->ents[e].hidden_dim, p->ents[e].feature_total, dev_out,
                            p->stream));
  return IGN_OK;
}

// dLoss/d(edge_params) of source s of MP mi after a completed backward: msg_net_backward added the
// edge_params columns of every instance's d(network input) into MPTrain::dprm, in instance order
int ign_batch_edge_param_gradients(ign_plan* p, ign_batch* b, int32_t mi, int32_t s, float* dev_out) {
  int rc = check_train(p, b);
  if (rc || (rc = check_edge_source(p, b, mi, s, dev_out))) return rc;
  const TrainState* t = b->train;
  if (!t->edge_grads)
    return fail(IGN_ERR_INVALID, "ign_batch_edge_param_gradients needs ign_batch_enable_edge_param_gradients (a default "
                "backward does not keep them)");
  if (!t->backward_done || !t->edge_grads_live)
    return fail(IGN_ERR_INVALID, "ign_batch_edge_param_gradients needs a completed backward of this batch that began after "
                "the opt-in (ign_backward or ign_backward_end after its ign_forward_train)");
  const size_t bytes = (size_t)b->mp[mi].n_edges[s] * p->mps[mi].nn[s].param_dim * sizeof(float);
  if (bytes) HIP_TRY(hipMemcpyAsync(dev_out, t->mp[mi].dprm[s], bytes, hipMemcpyDeviceToDevice, p->stream));
  return IGN_OK;
}

int ign_batch_train_buffers(const ign_batch* b, int32_t e, float** state, float** grad) {
  if (!b || !b->train) return fail(IGN_ERR_INVALID, "training not enabled on this batch");
  const TrainState* t = b->train;
  if (e < 0 || e >= (int)t->ver.size()) return fail(IGN_ERR_INVALID, "entity %d out of range", e);
  if (state) *state = t->ver[e][t->cur[e]];
  if (grad) *grad = t->dS[t->dcur.empty() ? 0 : t->dcur[e]][e];
  return IGN_OK;
}

int ign_backward(ign_plan* p, ign_batch* b, const float* dpred, float* grads) {
  int rc = ign_backward_begin(p, b, dpred, grads, 1.f);
  while (!rc && b->train->b_ri >= 0) rc = ign_backward_mp(p, b);
  return rc ? rc : ign_backward_end(p, b);
}

int ign_plan_get_params(ign_plan* p, float* host_out) {
  if (!p || !host_out) return fail(IGN_ERR_INVALID, "null argument");
  if (!p->params_set) return fail(IGN_ERR_INVALID, "parameters not set (ign_plan_set_params)");
  int rc = ensure_device(p);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(host_out, p->d_params, p->n_params * sizeof(float), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return IGN_OK;
}

}  // extern "C"
