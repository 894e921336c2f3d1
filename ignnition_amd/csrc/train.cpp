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
// The loss, the regularizer's value and the optimizer update around them are learn.cpp.
//
// Backward schedule: readout Dense stack in reverse, then the MP instances of the forward in
// reverse order.  Per entity one gradient buffer tracks dLoss/d(current version); an MP turns
// the gradient of its output version into that of its input version (GRU backward) and adds
// the message gradients to its sources.  Weight gradients are row-contractions
// (tsgemm_add) reduced in a fixed order: the result is deterministic.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "dense_stack.h"
#include "mp_step.h"
#include "readout_kernels.h"
#include "train_kernels.h"
#include "train_lower.h"

struct MPTrain {
  std::vector<float*> hs;     // sorted MPs: per iteration [(n_steps + n_dst)][H]
  std::vector<float*> xs;     // sum MPs: per iteration [rows][DIN]
  std::vector<float*> ss;     // convolution MPs: per iteration, message sums before K [rows][DIN]
  float* deg = nullptr;       // convolution MPs: messages per destination row (float)
  int32_t* amdst = nullptr;   // attention MPs: destination row of every CSR message
  std::vector<int32_t*> asptr, asidx;   // attention MPs, per slot: source row -> CSR messages
  int64_t hs_rows = 0;
  int32_t* hdrb = nullptr;    // sorted MPs: the ordered backward's tile headers (launch_seq_bwd_hdr)
  std::vector<int32_t*> tptr, tidx;   // per source slot: source row -> steps (sorted) / dst rows (sum)
  hvec<int64_t> trows;         // (a source with a message network: its rows are the edges)
  // message networks, per source slot: state row -> its edges (ascending), for the hs_source /
  // hs_dest columns of the network's input gradient
  int32_t* nsrc_ptr[IGN_MAX_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
  int32_t* nsrc_idx[IGN_MAX_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
  int32_t* ndst_ptr[IGN_MAX_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
  int32_t* ndst_idx[IGN_MAX_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
  // ign_batch_enable_edge_param_gradients: per source slot whose network reads edge_params, the
  // backward's sum over this MP's instances of d(network input)'s edge_params columns [edges][param_dim]
  float* dprm[IGN_MAX_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
};

struct MPRec {
  int mi, it, v_in;
  int src_v[IGN_MAX_SLOTS];
};

struct TrainState {
  std::vector<std::vector<float*>> ver;   // [entity][version] hidden states
  hvec<int> cur;                   // current version per entity (after the forward)
  std::vector<const float*> ent;   // ver[e][cur[e]] as of ign_forward_train_end: the readout's entity tensors
  std::vector<MPTrain> mp;
  std::vector<MPRec> recs;
  float* ga = nullptr;
  float* gu = nullptr;
  float* dx = nullptr;
  float* dtab = nullptr;
  float* gu2 = nullptr;       // a reset_after = false cell's backward: gu's second half and r * h_prev
  float* rh = nullptr;        //   (CellBwdExtra), rows as gu's
  float* rsrc = nullptr;      // convolution plans: an ordered MP's source rows, the unread ones as zeros
  std::vector<float*> dS[2];
  std::vector<float*> act;                // readout activations of layers 0 .. L-2
  float* dz[2] = {nullptr, nullptr};
  float* part = nullptr;
  float* bsum = nullptr;                  // [(H + 1) 3H], H <= 32: fused ordered backward's reduction
  float* ro_x = nullptr;                  // concatenated readout input (several input entities)
  float* dro = nullptr;
  float* dmsg = nullptr;                  // message networks: d(messages) [edges][out]
  float* mz[2] = {nullptr, nullptr};      // ... layer gradients (ping-pong) [edges][widest]
  float* mdin = nullptr;                  // ... d(network input) [edges][din]
  float* adw = nullptr;                   // attention: d(weight) and d(score input) per message,
  float* adv = nullptr;                   //   d(score) per source / destination row, d(w1 | w2)
  float* ads_src = nullptr;
  float* ads_dst = nullptr;
  float* adw12 = nullptr;
  // readout operations before predict (GM:605-655): d(tensor) per op output, Dense scratch
  std::vector<float*> dT;                 // per readout tensor id (null for entity states)
  float* rz[2] = {nullptr, nullptr};
  float* rcat = nullptr;
  float* rties = nullptr;
  std::vector<int32_t*> rx_ptr, rx_idx;   // extend ops: per op 2 transposed CSRs (input row -> edges)
  // Dropout sites of the readout stacks, per site [rows][units]: the masked input z of the layer it
  // precedes (the backward's weight gradient reads it; the unmasked y stays where the layer below
  // wrote it, for its activation derivative), or, after a stack's last layer, that layer's output y
  std::vector<float*> dbuf;
  DropRun drop;                           // the forward's mask stream: its backward regenerates the masks
  // LayerNormalization layers of the readout stacks, per site: its output [rows][units] (after a
  // stack's last layer: its input), apart from the batch's inference buffers, and its rows' (mean, rstd)
  std::vector<float*> nbuf, nstats;
  NormRun norm;
  bool forward_done = false;
  bool backward_done = false;   // ign_backward_end ran for the last forward: dS holds dLoss/d(initial states)
  bool edge_grads = false;      // ign_batch_enable_edge_param_gradients: MPTrain::dprm are allocated
  bool edge_grads_live = false; // ... and the backward that began last zeroed them and adds to them
  // stepped forward / backward (ign_forward_train_begin .. _end, ign_backward_begin .. _end): the
  // edge-cut driver exchanges halo rows between the steps
  int f_it = 0, f_mi = 0;
  bool f_open = false;
  float** res_ptrs = nullptr;   // the graph-resident training forward's version / save pointer arrays
  std::vector<float*> tsave;    // its saved projected tables of the ordered MP, per iteration
  bool tab_saved = false;       // this forward saved them (the backward skips mp_project)
  // weight gradients formed once per MP instance (T of them per backward) keep their partial tiles
  // here and are reduced once, at ign_backward_end, in instance order (IGN_DEFER_WGRAD=0: per instance)
  struct DeferredGrad {
    int64_t off_c, off_cb;   // gradient offsets in the parameter layout (off_cb -1: no bias column)
    int M, N, ones;
    float* part;
    int64_t cap, used;   // chunk slots (plus the reduction's scratch after cap)
  };
  std::vector<DeferredGrad> defer;
  struct DeferredSeq {   // the fused ordered backward's per-wave dU / bias partials, per cell
    int cell, H;
    float* part;
    int64_t cap, used;   // partial slots (plus the reduction's scratch after cap)
  };
  std::vector<DeferredSeq> defer_seq;
  int b_ri = -1;
  bool b_open = false;
  hvec<int> dcur;                          // backward: current gradient buffer per entity
  float* grads = nullptr;                  // backward: the caller's gradient vector
  float l2_scale = 1.f;                    // backward: weight of the l2 terms (1/ranks under edge-cut)
  std::vector<void*> allocs;               // blocks of pool
  DevPool* pool = nullptr;                 // the batch's (outlives this state)
  hipStream_t stream = nullptr;            // the plan stream, for the release fence
};

bool train_step_open(const TrainState* t) { return t->f_open || t->forward_done || t->b_open; }

void train_state_destroy(TrainState* t) {
  if (!t) return;
  if (t->pool) pool_release(t->pool, t->allocs, t->stream);
  delete t;
}

namespace {

int talloc(TrainState* t, float** out, int64_t n) {
  void* p = nullptr;
  hipError_t e = pool_alloc(t->pool, &p, (std::max<int64_t>(n, 0) + 256) * sizeof(float), true);
  if (e != hipSuccess) return fail(IGN_ERR_OOM, "training buffers: device alloc (%lld floats): %s", (long long)n,
                                   hipGetErrorString(e));
  t->allocs.push_back(p);
  *out = static_cast<float*>(p);
  return IGN_OK;
}

// The transposed CSRs of MP mb on the GPU (train_csr.hip; IGN_TRAIN_CSR_GPU=0: build_csrs on the
// host): a stable radix sort of the step (seq) or message keys on the upload stream, the same
// arrays as the host's.  ptr[s]: row pointers of source slot s into idx, the sorted values every
// slot shares.  The keys and the sort's scratch go back to the pool behind a fence.
int tcsr_gpu(TrainState* t, const MPB& mb, int S, const int64_t* tkeys, bool seq, std::vector<int32_t*>& ptr,
             int32_t*& idx) {
  hipStream_t st = upload_stream();
  const int64_t n = seq ? mb.n_steps : mb.n_msgs;
  int rc;
  float* f = nullptr;
  if ((rc = talloc(t, &f, std::max<int64_t>(n, 1)))) return rc;
  idx = reinterpret_cast<int32_t*>(f);
  ptr.assign(S, nullptr);
  for (int s = 0; s < S; ++s) {
    if ((rc = talloc(t, &f, tkeys[s] + 1))) return rc;
    ptr[s] = reinterpret_cast<int32_t*>(f);
  }
  const size_t nb = (size_t)std::max<int64_t>(n, 1) * 4, tb = tcsr_temp_bytes(std::max<int64_t>(n, 1));
  std::vector<void*> scratch(4, nullptr);
  for (int k = 0; k < 4; ++k) {
    const hipError_t e = pool_alloc(t->pool, &scratch[k], k < 3 ? nb : std::max<size_t>(tb, 256), false);
    if (e != hipSuccess) {
      scratch.resize(k);
      pool_release(t->pool, scratch, st);
      return fail(IGN_ERR_OOM, "training CSR scratch: device alloc: %s", hipGetErrorString(e));
    }
  }
  uint32_t* keys_in = static_cast<uint32_t*>(scratch[0]);
  uint32_t* keys_out = static_cast<uint32_t*>(scratch[1]);
  int32_t* vals_in = static_cast<int32_t*>(scratch[2]);
  uint32_t max_key = 0;
  hipError_t e;
  if (seq) {
    e = launch_tcsr_keys_seq(mb.d_step_code, n, (uint32_t)mb.zero_row, keys_in, vals_in, st);
    max_key = (uint32_t)mb.zero_row;
  } else {
    e = launch_tcsr_keys_sum(mb.d_msg_ptr, mb.d_order, mb.n_dst, mb.d_msg_src, keys_in, vals_in, st);
    // one slot: the codes are the rows (radix passes over the row bits only); else slot bits above
    max_key = S == 1 ? (uint32_t)std::max<int64_t>(tkeys[0], 1) : ((uint32_t)(S - 1) << IGN_SLOT_SHIFT) | IGN_ROW_MASK;
  }
  if (e == hipSuccess) e = launch_tcsr_sort(scratch[3], tb, keys_in, keys_out, vals_in, idx, n, max_key, st);
  for (int s = 0; s < S && e == hipSuccess; ++s) {
    const uint32_t key0 = seq ? (uint32_t)mb.src_off[s] : (uint32_t)s << IGN_SLOT_SHIFT;
    e = launch_tcsr_ptr(keys_out, n, key0, tkeys[s], ptr[s], st);
  }
  pool_release(t->pool, scratch, st);
  if (e != hipSuccess) return fail(IGN_ERR_DEVICE, "training CSR sort: %s", hipGetErrorString(e));
  return IGN_OK;
}

template <typename T, typename A>
int tupload(TrainState* t, T** out, const std::vector<T, A>& h) {
  void* p = nullptr;
  size_t n = std::max<size_t>(h.size(), 1);
  hipError_t e = pool_alloc(t->pool, &p, n * sizeof(T), h.empty());
  if (e != hipSuccess) return fail(IGN_ERR_OOM, "training buffers: device alloc: %s", hipGetErrorString(e));
  t->allocs.push_back(p);
  if (!h.empty()) HIP_TRY(upload_bytes(p, h.data(), h.size() * sizeof(T)));
  *out = static_cast<T*>(p);
  return IGN_OK;
}

// C (+ Cb) += A^T B over n_rows rows, its partial tiles parked for ign_backward_end's reduction
// when C has a deferred slot with room (else reduced now, as launch_tsgemm_add)
int tsgemm_deferred(TrainState* t, const float* A, int lda, const float* B, int ldb, int64_t n_rows, int M, int N,
                    float* C, float* Cb, hipStream_t st) {
  const int ones = Cb != nullptr;
  const int64_t ch = tsgemm_chunks(n_rows, M, N, ones);
  for (auto& d : t->defer)
    if (t->grads + d.off_c == C && (d.off_cb < 0 ? Cb == nullptr : Cb == t->grads + d.off_cb) && d.M == M &&
        d.N == N && d.used + ch <= d.cap) {
      HIP_TRY(launch_tsgemm_partials(A, lda, B, ldb, n_rows, M, N, ones, d.part + d.used * (int64_t)(M + ones) * N, st));
      d.used += ch;
      return IGN_OK;
    }
  HIP_TRY(launch_tsgemm_add(A, lda, B, ldb, n_rows, M, N, t->part, C, Cb, st));
  return IGN_OK;
}

int tsgemm_deferred_flush(const ign_plan* p, TrainState* t, hipStream_t st) {
  for (auto& d : t->defer_seq)
    if (d.used) {
      const CellP& cp = p->cells[d.cell];
      SeqBwdArgs a{};
      a.part = d.part;
      a.scratch = t->bsum;
      a.dU = t->grads + cp.off_rk;
      a.db_rec = t->grads + cp.off_b + 3 * cp.H;
      a.db_in = t->grads + cp.off_b;
      HIP_TRY(launch_seq_bwd_reduce(a, d.used, d.H, st));
      d.used = 0;
    }
  for (auto& d : t->defer)
    if (d.used) {
      HIP_TRY(launch_partials_reduce_add(d.part, d.used, d.M, d.N, d.ones, t->grads + d.off_c,
                                         d.off_cb < 0 ? nullptr : t->grads + d.off_cb, st));
      d.used = 0;
    }
  return IGN_OK;
}

int check_train(ign_plan* p, ign_batch* b) { return check_pb(p, b, true); }

// Backward of MP source s's message-creation network (GM:440-475), given d(messages) in t->dmsg:
// Dense stack in reverse (weight / bias gradients; the l2 terms are added once per step by
// ign_backward, not per MP instance), then the hs_source / hs_dest column
// slices of d(input) gathered back to the state rows they were read from.  The layer activations
// are the ones mp_message_nets left in mb (recomputed for this MP instance by the caller).
int msg_net_backward(ign_plan* p, ign_batch* b, TrainState* t, const MPP& mp, const MPB& mb, const MPTrain& mt,
                     int s, float* dsrc, float* ddst, float* grads, hipStream_t st) {
  const MsgNN& nn = mp.nn[s];
  DenseStackRun r{nn.layers.data(), (int)nn.layers.size(), mb.n_edges[s], mb.d_msg_in[s], nn.din_pad,
                  mb.d_msg_layer[s].data(), mb.d_msg_layer[s].back()};
  r.dy = t->dmsg;
  r.gz = t->mz;
  r.part = t->part;
  r.grads = grads;
  r.dx = t->mdin;   // overwritten: gathered below
  if (int rc = dense_stack_backward(p, r, st)) return rc;
  int col = 0;
  for (size_t q = 0; q < nn.inputs.size(); ++q) {
    const int w = nn.widths[q];
    if (nn.inputs[q] == IGN_MSG_HS_SOURCE)
      HIP_TRY(launch_csr_gather_cols_add(dsrc, b->rows[mp.src[s].entity] + b->halo[mp.src[s].entity], mt.nsrc_ptr[s],
                                         mt.nsrc_idx[s], t->mdin,
                                         nn.din, col, w, 1, st));
    else if (nn.inputs[q] == IGN_MSG_HS_DEST)
      HIP_TRY(launch_csr_gather_cols_add(ddst, b->rows[mp.dst], mt.ndst_ptr[s], mt.ndst_idx[s], t->mdin, nn.din,
                                         col, w, 1, st));
    else if (nn.inputs[q] == IGN_MSG_EDGE_PARAMS && t->edge_grads_live)   // input data: its gradient only on request
      HIP_TRY(launch_slice_cols_add(t->mdin, mb.n_edges[s], nn.din, col, w, mt.dprm[s], st));
    col += w;
  }
  return IGN_OK;
}

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

// ---------------------------------------------------------------------------------------------
// ign_batch_enable_training, step by step

// every used GRU cell has its backward fragments
int check_train_shapes(const ign_plan* p) {
  for (size_t c = 0; c < p->cells.size(); ++c) {
    const CellP& cp = p->cells[c];
    if (!cp.used) continue;
    bool concat_only = true;   // W^T is not needed by a cell fed only by axis-2 concat MPs
    for (auto& mp : p->mps)
      if (mp.cell == (int)c && !mp.feature_concat) concat_only = false;
    if (cp.pk_ut < 0 || (cp.pk_wt < 0 && !concat_only))
      return fail(IGN_ERR_UNSUPPORTED, "no backward kernel for GRU shape (input %d, units %d)", cp.din, cp.H);
  }
  return IGN_OK;
}

// per entity: the hidden-state versions, 1 + T x (MPs updating the entity), and the two dS buffers
int alloc_states(const ign_plan* p, const ign_batch* b, TrainState* t) {
  const int E = (int)p->ents.size();
  int rc;
  hvec<int> nver(E, 1);
  for (auto& mp : p->mps) nver[mp.dst] += p->T;
  t->ver.resize(E);
  t->cur.assign(E, 0);
  t->ent.assign(E, nullptr);
  for (int e = 0; e < E; ++e) {
    const int64_t n = (b->rows[e] + b->halo[e]) * p->ents[e].hidden_dim;   // owned rows, then halo rows
    for (int v = 0; v < nver[e]; ++v) {
      float* f = nullptr;
      if ((rc = talloc(t, &f, n))) return rc;
      t->ver[e].push_back(f);
    }
    for (int k = 0; k < 2; ++k) {
      float* f = nullptr;
      if ((rc = talloc(t, &f, n))) return rc;
      t->dS[k].push_back(f);
    }
  }
  return IGN_OK;
}

TrainMpIn host_tables(const MPB& mb) {
  return {mb.h_order, mb.h_len, mb.h_step_ptr, mb.h_msg_ptr, mb.h_multi_ptr, mb.h_step_code,
          mb.h_msg_src, mb.h_multi_rows, mb.src_off, mb.zero_row, mb.n_dst, mb.n_msgs};
}

// message network of source s (GM:440-475): the state row -> edge CSRs of its backward, from the
// edge rows the batch keeps on the device
int enable_msg_net(const ign_batch* b, TrainState* t, const MPP& mp, const MPB& mb, int s, MPTrain& mt) {
  const int se = mp.src[s].entity;
  const int64_t ne = mb.n_edges[s];
  int rc;
  hvec<int32_t> es(ne), ed(ne);
  HIP_TRY(hipMemcpyAsync(es.data(), mb.d_edge_src[s], ne * sizeof(int32_t), hipMemcpyDeviceToHost, upload_stream()));
  HIP_TRY(hipMemcpyAsync(ed.data(), mb.d_edge_dst[s], ne * sizeof(int32_t), hipMemcpyDeviceToHost, upload_stream()));
  HIP_TRY(hipStreamSynchronize(upload_stream()));
  HIP_TRY(upload_flush());
  hvec<int32_t> p1, i1, p2, i2;
  lower_row_edges(b->rows[se] + b->halo[se], es.data(), ne, &p1, &i1);   // sources may be halo rows (edge-cut)
  lower_row_edges(b->rows[mp.dst], ed.data(), ne, &p2, &i2);
  if ((rc = tupload(t, &mt.nsrc_ptr[s], p1)) || (rc = tupload(t, &mt.nsrc_idx[s], i1)) ||
      (rc = tupload(t, &mt.ndst_ptr[s], p2)) || (rc = tupload(t, &mt.ndst_idx[s], i2)))
    return rc;
  return IGN_OK;
}

// MP mi: the buffers its forward saves into and the tables its backward walks.  The transposed
// CSRs (source row -> steps / destinations reading it) are built on the GPU (mt.tptr, gidx) or on
// the host (tptr, tidx, uploaded with the slots)
int enable_mp(const ign_plan* p, const ign_batch* b, TrainState* t, size_t mi, bool tcsr_on) {
  const MPP& mp = p->mps[mi];
  const MPB& mb = b->mp[mi];
  const int H = p->cells[mp.cell].H, DIN = mp.din, S = (int)mp.src.size();
  const TrainMpIn in = host_tables(mb);
  int rc;
  MPTrain mt;
  std::vector<hvec<int32_t>> tptr, tidx;
  int32_t* gidx = nullptr;
  int64_t tkeys[IGN_MAX_SLOTS] = {0, 0, 0, 0};
  for (int s = 0; s < S; ++s) tkeys[s] = train_keys(mp, s, b->rows, b->halo, mb.n_edges);
  if (mb.sorted) {
    mt.hs_rows = mb.n_steps + mb.n_dst;
    for (int it = 0; it < p->T; ++it) {
      float* f = nullptr;
      // + one pad row: the resident training forward's tile headers point padding positions there
      // (resident.hip, hsb; its stores skip them, so the row stays unwritten)
      if ((rc = talloc(t, &f, (mt.hs_rows + 1) * H))) return rc;
      mt.hs.push_back(f);
    }
    {
      const int64_t n_pos = (mb.n_dst + 15) / 16 * 16;
      float* f = nullptr;
      if ((rc = talloc(t, &f, 4 * n_pos))) return rc;
      mt.hdrb = reinterpret_cast<int32_t*>(f);
      // on the upload stream, behind the block's IGN_POOL_POISON fill (pool_alloc) and before the
      // synchronisation at the end of this call: a launch on the plan stream could land first
      HIP_TRY(launch_seq_bwd_hdr(mb.d_seq_hdr, mb.d_step_code, n_pos, mt.hdrb, upload_stream()));
    }
    // a pre-summed row expands into its source rows on the host only
    if (tcsr_on && mb.n_multi == 0) {
      if ((rc = tcsr_gpu(t, mb, S, tkeys, true, mt.tptr, gidx))) return rc;
    } else lower_train_ordered(S, tkeys, in, tptr, tidx);
  } else {
    for (int it = 0; it < p->T; ++it) {
      float* f = nullptr;
      if ((rc = talloc(t, &f, mb.n_dst * DIN))) return rc;
      mt.xs.push_back(f);
      if (mp.aggr == IGN_AGGR_CONVOLUTION) {
        if ((rc = talloc(t, &f, mb.n_dst * DIN))) return rc;
        mt.ss.push_back(f);
      }
    }
    if (mp.aggr == IGN_AGGR_ATTENTION) {
      // (no halo rows under attention; a message network's codes address its edges, the per-edge message rows)
      TrainAttn at;
      lower_train_attention(S, tkeys, in, &at);
      if ((rc = tupload(t, &mt.amdst, at.mdst))) return rc;
      for (int s = 0; s < S; ++s) {
        int32_t *dp = nullptr, *di = nullptr;
        if ((rc = tupload(t, &dp, at.ptr[s])) || (rc = tupload(t, &di, at.idx[s]))) return rc;
        mt.asptr.push_back(dp);
        mt.asidx.push_back(di);
      }
    }
    if (mp.aggr == IGN_AGGR_CONVOLUTION) {
      hvec<float> deg;
      lower_train_degree(in, &deg);
      if ((rc = tupload(t, &mt.deg, deg))) return rc;
    }
    if (tcsr_on) {
      if ((rc = tcsr_gpu(t, mb, S, tkeys, false, mt.tptr, gidx))) return rc;
    } else lower_train_sum(S, tkeys, in, tptr, tidx);
  }
  for (int s = 0; s < S; ++s) {
    if (gidx) {
      mt.tidx.push_back(gidx);   // (mt.tptr[s] set by tcsr_gpu)
    } else {
      int32_t *dp = nullptr, *di = nullptr;
      if ((rc = tupload(t, &dp, tptr[s])) || (rc = tupload(t, &di, tidx[s]))) return rc;
      mt.tptr.push_back(dp);
      mt.tidx.push_back(di);
    }
    mt.trows.push_back(tkeys[s]);
    if (!mp.nn[s].layers.empty() && (rc = enable_msg_net(b, t, mp, mb, s, mt))) return rc;
  }
  t->mp.push_back(std::move(mt));
  return IGN_OK;
}

// floats of the scratch buffers the MP instances / readout layers of a backward share: the largest need of each
struct TrainScratch {
  int64_t ga = 0, gu = 0, dx = 0, dtab = 0, part = 0, rsrc = 0, gu2 = 0, rh = 0;
  int64_t dmsg = 0, mz = 0, mdin = 0;            // message networks
  int64_t amsg = 0, arows = 0;                   // attention
  int64_t dz = 0, rz = 0, rcat = 0, ties = 0;    // readout
  std::vector<int64_t> drop;                     // per Dropout site: rows x units
  std::vector<int64_t> norm, norm_rows;          // per LayerNormalization site: rows x units, rows
};
TrainScratch train_scratch(const ign_plan* p, const ign_batch* b) {
  TrainScratch z;
  auto need_part = [&](int64_t rows, int M, int N) { z.part = std::max(z.part, tsgemm_partial_floats(rows, M, N)); };
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {
    const MPP& mp = p->mps[mi];
    const MPB& mb = b->mp[mi];
    const int H = p->cells[mp.cell].H, DIN = mp.din, S = (int)mp.src.size();
    if (mb.sorted) {
      const int64_t hs_rows = mb.n_steps + mb.n_dst;
      z.ga = std::max(z.ga, (mb.n_steps + 1) * 3 * H);   // + the pad slot row (seq_gru_bwd_kernel)
      z.gu = std::max(z.gu, hs_rows * 3 * H);
      if (!p->cells[mp.cell].reset_after) {
        z.gu2 = std::max(z.gu2, hs_rows * 3 * H);
        z.rh = std::max(z.rh, hs_rows * H);
      }
      need_part(hs_rows, H, 3 * H);
      if (p->bwd_fuse && seq_bwd_fused_supported(H)) z.part = std::max(z.part, seq_bwd_partial_floats(H));
      for (int s = 0; s < S; ++s) {
        z.dtab = std::max(z.dtab, mb.src_rows[s] * 3 * H);
        if (p->conv_F && mp.nn[s].layers.empty())
          z.rsrc = std::max(z.rsrc, train_keys(mp, s, b->rows, b->halo, mb.n_edges) *
                                        (mp.feature_concat ? p->ents[mp.src[s].entity].hidden_dim : DIN));
        need_part(mb.src_rows[s], mp.feature_concat ? p->ents[mp.src[s].entity].hidden_dim : DIN, 3 * H);
      }
    } else {
      if (mp.aggr == IGN_AGGR_ATTENTION) {
        for (int s = 0; s < S; ++s) {
          const int64_t rows_s = train_keys(mp, s, b->rows, b->halo, mb.n_edges);
          z.arows = std::max(z.arows, rows_s);
          need_part(rows_s, DIN, 1);
        }
        z.amsg = std::max(z.amsg, mb.n_msgs);
        z.arows = std::max(z.arows, mb.n_dst);
        need_part(mb.n_dst, H, 1);
      }
      if (mp.aggr == IGN_AGGR_CONVOLUTION) {
        z.dtab = std::max(z.dtab, 2 * mb.n_dst * DIN);   // du and d(sum) of the convolution
        need_part(mb.n_dst, DIN, DIN);
      }
      z.ga = std::max(z.ga, mb.n_dst * 3 * H);
      z.gu = std::max(z.gu, mb.n_dst * 3 * H);
      if (!p->cells[mp.cell].reset_after) {
        z.gu2 = std::max(z.gu2, mb.n_dst * 3 * H);
        z.rh = std::max(z.rh, mb.n_dst * H);
      }
      z.dx = std::max(z.dx, mb.n_dst * DIN);
      need_part(mb.n_dst, std::max(DIN, H), 3 * H);
    }
    need_part(std::max<int64_t>(mb.n_steps, mb.n_dst), 1, 3 * H);   // colsum
    for (int s = 0; s < S; ++s) {
      const MsgNN& nn = mp.nn[s];
      if (nn.layers.empty()) continue;
      const int64_t ne = mb.n_edges[s];
      int widest = nn.din_pad;
      for (size_t l = 0; l < nn.layers.size(); ++l) {
        widest = std::max(widest, nn.layers[l].out);
        need_part(ne, l == 0 ? nn.din : nn.layers[l].in, nn.layers[l].out);
      }
      z.dmsg = std::max(z.dmsg, ne * nn.dout());
      z.mz = std::max(z.mz, ne * widest);
      z.mdin = std::max(z.mdin, ne * nn.din);
    }
  }
  const int64_t P = b->n_pred;
  int64_t widest = p->ro_width;
  for (auto& d : p->dense) {
    widest = std::max<int64_t>(widest, d.out);
    need_part(P, d.in, d.out);
  }
  z.dz = P * widest;
  for (auto& op : p->ro_ops) {   // readout operations (GM:605-655)
    const int64_t n = space_rows(p, b, p->ro_t[op.in[0]]);
    if (op.type == IGN_RO_NEURAL_NETWORK) {
      int widest = op.in_width, K = op.in_width;
      for (auto& d : op.layers) {
        widest = std::max(widest, d.out);
        need_part(n, K, d.out);
        K = d.out;
      }
      z.rz = std::max(z.rz, n * widest);
      if (op.in.size() > 1) z.rcat = std::max(z.rcat, n * op.in_width);
    } else if (op.type == IGN_RO_POOLING) {
      z.ties = std::max(z.ties, (int64_t)b->G * p->ro_t[op.in[0]].width);
    }
  }
  for (const DropSite& d : p->drops) z.drop.push_back(stack_rows(p, b, d.stack) * d.units);
  for (const NormSite& ns : p->norms) {
    const int64_t rows = stack_rows(p, b, ns.stack);
    z.norm.push_back(rows * ns.units);
    z.norm_rows.push_back(rows);
    z.part = std::max(z.part, layernorm_partial_floats(rows, ns.units));
  }
  return z;
}

int alloc_mp_scratch(const ign_plan* p, TrainState* t, const TrainScratch& z) {
  int rc;
  if ((rc = talloc(t, &t->ga, z.ga)) || (rc = talloc(t, &t->gu, z.gu)) || (rc = talloc(t, &t->dx, z.dx)) ||
      (rc = talloc(t, &t->dtab, z.dtab)))
    return rc;
  if (z.gu2 && ((rc = talloc(t, &t->gu2, z.gu2)) || (rc = talloc(t, &t->rh, z.rh)))) return rc;
  if (z.rsrc && (rc = talloc(t, &t->rsrc, z.rsrc))) return rc;
  if (z.amsg && ((rc = talloc(t, &t->adw, z.amsg)) || (rc = talloc(t, &t->adv, z.amsg)) ||
                 (rc = talloc(t, &t->ads_src, z.arows)) || (rc = talloc(t, &t->ads_dst, z.arows)) ||
                 (rc = talloc(t, &t->adw12, 2 * p->attn_F))))
    return rc;
  if (z.dmsg && ((rc = talloc(t, &t->dmsg, z.dmsg)) || (rc = talloc(t, &t->mz[0], z.mz)) ||
                 (rc = talloc(t, &t->mz[1], z.mz)) || (rc = talloc(t, &t->mdin, z.mdin))))
    return rc;
  return IGN_OK;
}

// the readout's saved activations and gradient buffers; per extend op, its two input row -> edge CSRs
int alloc_readout(const ign_plan* p, const ign_batch* b, TrainState* t, const TrainScratch& z) {
  const int64_t P = b->n_pred;
  int rc;
  for (size_t l = 0; l + 1 < p->dense.size(); ++l) {
    float* f = nullptr;
    if ((rc = talloc(t, &f, P * p->dense[l].out))) return rc;
    t->act.push_back(f);
  }
  if ((rc = talloc(t, &t->dz[0], z.dz)) || (rc = talloc(t, &t->dz[1], z.dz))) return rc;
  if (p->ro_in.size() > 1 &&
      ((rc = talloc(t, &t->ro_x, P * p->ro_width)) || (rc = talloc(t, &t->dro, P * p->ro_width))))
    return rc;
  // readout operations (GM:605-655)
  t->dT.assign(p->ro_t.size(), nullptr);
  for (size_t k = 0; k < p->ro_ops.size(); ++k) {
    const RoOp& op = p->ro_ops[k];
    const int nout = op.type == IGN_RO_EXTEND ? 2 : 1;
    for (int j = 0; j < nout; ++j) {
      const RoTensor& to = p->ro_t[op.out + j];
      if ((rc = talloc(t, &t->dT[op.out + j], space_rows(p, b, to) * to.width))) return rc;
    }
    if (op.type != IGN_RO_EXTEND) continue;
    for (int j = 0; j < 2; ++j) {
      const std::vector<int32_t>& ix = b->ro[k].h_idx[j];
      hvec<int32_t> ptr, idx;
      lower_row_edges(space_rows(p, b, p->ro_t[op.in[j]]), ix.data(), (int64_t)ix.size(), &ptr, &idx);
      int32_t *dp = nullptr, *di = nullptr;
      if ((rc = tupload(t, &dp, ptr)) || (rc = tupload(t, &di, idx))) return rc;
      t->rx_ptr.push_back(dp);
      t->rx_idx.push_back(di);
    }
  }
  if ((z.rz && ((rc = talloc(t, &t->rz[0], z.rz)) || (rc = talloc(t, &t->rz[1], z.rz)))) ||
      (z.rcat && (rc = talloc(t, &t->rcat, z.rcat))) || (z.ties && (rc = talloc(t, &t->rties, z.ties))))
    return rc;
  for (int64_t n : z.drop) {   // one [rows][units] buffer per Dropout site
    float* f = nullptr;
    if ((rc = talloc(t, &f, n))) return rc;
    t->dbuf.push_back(f);
  }
  for (size_t s = 0; s < z.norm.size(); ++s) {
    float *f = nullptr, *m = nullptr;
    if ((rc = talloc(t, &f, z.norm[s])) || (rc = talloc(t, &m, 2 * z.norm_rows[s]))) return rc;
    t->nbuf.push_back(f);
    t->nstats.push_back(m);
  }
  return IGN_OK;
}

// IGN_DEFER_WGRAD (default on): the per-instance weight gradients of the plain sum and ordered MPs
// (ign_backward_mp): one slot per (gradient tensor, shape), room for every instance of a backward
int alloc_deferred(const ign_plan* p, const ign_batch* b, TrainState* t) {
  int rc;
  struct Want { int64_t c, cb; int M, N, ones; int64_t chunks; };
  std::vector<Want> want;
  auto add = [&](int64_t c, int64_t cb, int M, int N, int64_t rows, int64_t min_slots = 0) {
    const int ones = cb >= 0;
    const int64_t ch = std::max(tsgemm_chunks(rows, M, N, ones), min_slots) * p->T;
    for (auto& w : want)
      if (w.c == c && w.cb == cb && w.M == M && w.N == N) { w.chunks += ch; return; }
    want.push_back({c, cb, M, N, ones, ch});
  };
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {
    const MPP& mp = p->mps[mi];
    const MPB& mb = b->mp[mi];
    const CellP& cp = p->cells[mp.cell];
    bool nets = false;
    for (auto& nn : mp.nn) nets = nets || !nn.layers.empty();
    if (nets || mp.feature_concat) continue;
    const int H = cp.H, H3 = 3 * cp.H, DIN = mp.din;
    if (mp.sorted) {
      for (size_t s2 = 0; s2 < mp.src.size(); ++s2) add(cp.off_k, -1, DIN, H3, t->mp[mi].trows[s2]);
    } else if (mp.aggr == IGN_AGGR_SUM && cp.is_default()) {   // (a cell with options reduces per instance)
      const int64_t fw = sum_bwd_fused_waves(mb.n_dst, DIN, H);   // the fused sum backward's partials
      add(cp.off_k, cp.off_b, DIN, H3, mb.n_dst, fw);
      add(cp.off_rk, cp.off_b + H3, H, H3, mb.n_dst, fw);
    }
  }
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {   // the fused ordered backward's partials
    const MPP& mp = p->mps[mi];
    const CellP& cp = p->cells[mp.cell];
    if (!mp.sorted || !p->bwd_fuse || !seq_bwd_fused_supported(cp.H) || !cp.is_default()) continue;
    const int64_t tiles = (b->mp[mi].n_dst + 15) / 16;
    const int64_t waves = std::min<int64_t>((tiles + 3) / 4 * 4, kBwdPartialWaves) * p->T;   // upper bound
    bool found = false;
    for (auto& d : t->defer_seq)
      if (d.cell == mp.cell) { d.cap += waves; found = true; }
    if (!found) t->defer_seq.push_back({mp.cell, cp.H, nullptr, waves, 0});
  }
  for (auto& d : t->defer_seq)
    if ((rc = talloc(t, &d.part, (d.cap + kTsReduceSegs) * (int64_t)(d.H + 2) * 3 * d.H))) return rc;
  for (auto& w : want) {
    TrainState::DeferredGrad d{w.c, w.cb, w.M, w.N, w.ones, nullptr, w.chunks, 0};
    if ((rc = talloc(t, &d.part, (w.chunks + kTsReduceSegs) * (int64_t)(w.M + w.ones) * w.N))) return rc;
    t->defer.push_back(d);
  }
  return IGN_OK;
}

}  // namespace

extern "C" {

int ign_batch_enable_training(ign_plan* p, ign_batch* b) {
  if (!p || !b) return fail(IGN_ERR_INVALID, "null argument");
  if (b->plan != p) return fail(IGN_ERR_INVALID, "batch was created for another plan");
  if (b->train) return IGN_OK;
  int rc = ensure_device(p);
  if (rc) return rc;
  UploadScope scope("ign_batch_enable_training");
  const char* fine = getenv("IGN_BUILD_PROF_FINE");
  BuildMarks bm(fine && atoi(fine) != 0);   // IGN_BUILD_PROF_FINE=1: host sections of this build
  if ((rc = check_train_shapes(p))) return rc;
  std::unique_ptr<TrainState, void (*)(TrainState*)> t(new TrainState(), train_state_destroy);
  t->pool = b->pool.get();
  t->stream = p->stream;
  if ((rc = alloc_states(p, b, t.get()))) return rc;
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {
    if ((rc = enable_mp(p, b, t.get(), mi, p->train_csr_gpu))) return rc;
    bm.mark(mi == 0 ? "mp0" : mi == 1 ? "mp1" : "mp2+");
  }
  const TrainScratch z = train_scratch(p, b);
  if ((rc = alloc_mp_scratch(p, t.get(), z)) || (rc = alloc_readout(p, b, t.get(), z))) return rc;
  if ((rc = talloc(t.get(), &t->part, z.part)) || (rc = talloc(t.get(), &t->bsum, (32 + 1) * 3 * 32))) return rc;
  if (p->defer_wgrad && (rc = alloc_deferred(p, b, t.get()))) return rc;
  bm.mark("rest");
  HIP_TRY(hipStreamSynchronize(upload_stream()));   // IGN_POOL_POISON fills have landed
  HIP_TRY(upload_flush());                           // (and every staged copy)
  bm.mark("wait");
  bm.print("ign_batch_enable_training fine");
  b->train = t.release();
  return IGN_OK;
}

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
  const bool fused = p->train_fused_readout && p->fused_readout && p->readout_variant >= 4 && p->dense.size() == 3 &&
                     p->dense[1].pk_h >= 0 && p->dense[0].pk_bf >= 0 && p->dense[1].pk_bf >= 0 &&
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

int ign_backward_mp(ign_plan* p, ign_batch* b) {
  int rc = check_train(p, b);
  if (rc) return rc;
  TrainState* t = b->train;
  if (!t->b_open || t->b_ri < 0) return fail(IGN_ERR_INVALID, "ign_backward_mp outside begin .. end");
  hipStream_t st = p->stream;
  hvec<int>& dcur = t->dcur;
  float* grads = t->grads;
  const int ri = t->b_ri--;
  {
    const MPRec& rec = t->recs[ri];
    const MPP& mp = p->mps[rec.mi];
    const MPB& mb = b->mp[rec.mi];
    const CellP& cp = p->cells[mp.cell];
    const MPTrain& mt = t->mp[rec.mi];
    const int dst = mp.dst, H = cp.H, DIN = mp.din, H3 = 3 * cp.H;
    float* dh_in = t->dS[dcur[dst]][dst];
    float* dh_out = t->dS[1 - dcur[dst]][dst];
    if (b->halo[dst])   // a self-loop MP's source gradient lands in dh_out's halo rows too
      HIP_TRY(hipMemsetAsync(dh_out + b->rows[dst] * H, 0, b->halo[dst] * H * sizeof(float), st));
    const float* srcs[IGN_MAX_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t s = 0; s < mp.src.size(); ++s) srcs[s] = t->ver[mp.src[s].entity][rec.src_v[s]];
    // recompute this instance's message networks (and, below, its table): the forward's routines, untimed
    if ((rc = mp_message_nets(p, mp, mb, srcs, t->ver[dst][rec.v_in], st))) return rc;
    Timer untimed{nullptr};
    auto src_grad = [&](size_t s) -> float* {      // where d(state of source s) accumulates
      const int se = mp.src[s].entity;
      return se == dst ? dh_out : t->dS[dcur[se]][se];
    };
    float* gk = grads + cp.off_k;
    float* grk = grads + cp.off_rk;
    float* gb = grads + cp.off_b;
    // A cell with options (gru_cell.hip): the bias gradients in the [3H] layout or nowhere, and for
    // reset_after = false the second pair of rows whose contraction completes dU
    const bool dflt = cp.is_default();
    float* gb_in = cp.use_bias ? gb : nullptr;
    float* gb_rec = cp.use_bias && cp.reset_after ? gb + H3 : nullptr;
    CellBwdExtra cx{};
    if (!cp.reset_after) {
      cx.gu2 = t->gu2;
      cx.rh = t->rh;
    }
    if (mp.sorted) {
      // the forward's table of this instance: saved by the resident training forward, else recomputed
      const bool saved = t->tab_saved && rec.mi == 0 && rec.it < (int)t->tsave.size();
      if (!saved && (rc = mp_project(p, mp, mb, srcs, 0, untimed))) return rc;
      SeqBwdArgs a{mt.hs[rec.it], saved ? t->tsave[rec.it] : mb.d_table, mb.d_order, mb.d_len, mb.d_step_ptr, mb.d_step_code,
                   p->d_packed + cp.pk_u, p->d_packed + cp.pk_b, p->d_packed + cp.pk_ut, dh_in, dh_out,
                   t->ga, t->gu, mb.n_dst};
      a.h_in = t->ver[dst][rec.v_in];
      a.hdr = mt.hdrb;
      if (!dflt) {
        HIP_TRY(launch_seq_gru_cell_bwd(a, H, cell_opt(cp), cx, st));
        HIP_TRY(launch_tsgemm_add(mt.hs[rec.it], H, t->gu, H3, mt.hs_rows, H, H3, t->part, grk, gb_rec, st));
        if (!cp.reset_after)   // dU_h = (r h)^T dc
          HIP_TRY(launch_tsgemm_add(t->rh, H, t->gu2, H3, mt.hs_rows, H, H3, t->part, grk, nullptr, st));
        if (gb_in) HIP_TRY(launch_colsum_add(t->ga, H3, mb.n_steps, H3, t->part, gb_in, st));
      } else if (p->bwd_fuse && seq_bwd_fused_supported(H)) {
        // dU and both bias gradients (column sums of da and du) inside the kernel
        a.gu = nullptr;
        a.part = t->part;
        a.dU = grk;
        a.db_rec = gb + H3;
        a.db_in = gb;
        a.scratch = t->bsum;
        // gate recompute on the forward's path (bitwise the forward's gates): split-fp16 x3 after
        // seq_gru_h16<SAVE>, split-bf16 x6 after seq_gru_bf x6; IGN_BWD_BF=0 keeps the f32 MFMA recompute
        if (p->bwd_bf && H == 32 && cp.pk_uh >= 0 && cp.pk_uth >= 0 && train_seq_variant(p, H) == 6) {
          a.Uh = p->d_packed + cp.pk_uh;
          a.Uth = p->d_packed + cp.pk_uth;
        }
        else if (p->bwd_bf && H == 32 && cp.pk_ubf >= 0 && train_seq_variant(p, H) == 4) a.Ubf = p->d_packed + cp.pk_ubf;
        // the partials stay for one reduction per backward (ign_backward_end) where the cell has room
        const int64_t waves = seq_bwd_fused_waves(a, H);
        for (auto& d : t->defer_seq)
          if (d.cell == mp.cell && d.used + waves <= d.cap) {
            a.part = d.part + d.used * (int64_t)(H + 2) * H3;
            a.defer_reduce = true;
            d.used += waves;
            break;
          }
        HIP_TRY(launch_seq_gru_bwd(a, H, st));
      } else {
        HIP_TRY(launch_seq_gru_bwd(a, H, st));
        HIP_TRY(launch_tsgemm_add(mt.hs[rec.it], H, t->gu, H3, mt.hs_rows, H, H3, t->part, grk, gb + H3, st));
        HIP_TRY(launch_colsum_add(t->ga, H3, mb.n_steps, H3, t->part, gb, st));
      }
      for (size_t s = 0; s < mp.src.size(); ++s) {
        const int se = mp.src[s].entity;
        HIP_TRY(launch_csr_gather_add(t->dtab, mt.trows[s], mt.tptr[s], mt.tidx[s], t->ga, H3, 0, st));
        const bool net = !mp.nn[s].layers.empty();
        float* target = net ? t->dmsg : se == dst ? dh_out : t->dS[dcur[se]][se];
        // dW = x^T dtab over the source rows.  A row that no step reads has a zero dtab row, but in a plan
        // with a convolution MP it may hold 0 / 0 (a destination without a message, AUX:384-401): NaN * 0.
        // Autograd gathers the read rows only, so there the unread rows enter as zeros
        const float* xs = srcs[s];
        if (t->rsrc && !net) {
          HIP_TRY(launch_read_rows(srcs[s], mt.tptr[s], mt.trows[s], mp.feature_concat ? p->ents[se].hidden_dim : DIN,
                                   t->rsrc, st));
          xs = t->rsrc;
        }
        if (mp.feature_concat) {   // AUX:443-456: the source's slice of the input kernel
          const int sdin = p->ents[se].hidden_dim;
          const int64_t koff = (int64_t)mp.slice_off[s] * H3;
          HIP_TRY(launch_tsgemm_add(xs, sdin, t->dtab, H3, mt.trows[s], sdin, H3, t->part, gk + koff, nullptr, st));
          HIP_TRY(launch_row_gemm_t_generic(t->dtab, mt.trows[s], H3, p->d_params + cp.off_k + koff, sdin, target,
                                            net ? 0 : 1, -1, nullptr, st));
        } else {
          if ((rc = tsgemm_deferred(t, xs, DIN, t->dtab, H3, mt.trows[s], DIN, H3, gk, nullptr, st))) return rc;
          HIP_TRY(launch_row_gemm_t(t->dtab, mt.trows[s], H3, p->d_packed + cp.pk_wt, DIN, target, net ? 0 : 1, -1,
                                    nullptr, st));
        }
        if (net && (rc = msg_net_backward(p, b, t, mp, mb, mt, (int)s, src_grad(s), dh_out, grads, st))) return rc;
      }
    } else {
      const float* hin = t->ver[dst][rec.v_in];
      SumBwdArgs a{mt.xs[rec.it], hin, p->d_packed + cp.pk_w, p->d_packed + cp.pk_u, p->d_packed + cp.pk_b,
                   p->d_packed + cp.pk_wt, p->d_packed + cp.pk_ut, dh_in, dh_out, t->dx, t->ga, t->gu, mb.n_dst};
      // plain sums at DIN = H = 32: dW / dU formed in the backward kernel, its partials into the
      // deferred slots (IGN_SUM_BWD_FUSE=0: da / du written, then the two row contractions; with no
      // deferred slot, IGN_DEFER_WGRAD=0, the unfused path runs whatever IGN_SUM_BWD_FUSE says)
      TrainState::DeferredGrad* dw = nullptr;
      TrainState::DeferredGrad* du = nullptr;
      const int64_t fw = mp.aggr == IGN_AGGR_SUM && p->sum_bwd_fuse ? sum_bwd_fused_waves(mb.n_dst, DIN, H) : 0;
      for (auto& d : t->defer) {
        if (fw && d.off_c == cp.off_k && d.off_cb == cp.off_b && d.M == DIN && d.N == H3 && d.used + fw <= d.cap) dw = &d;
        if (fw && d.off_c == cp.off_rk && d.off_cb == cp.off_b + H3 && d.M == H && d.N == H3 && d.used + fw <= d.cap) du = &d;
      }
      if (!dflt) {
        HIP_TRY(launch_sum_gru_cell_bwd(a, DIN, H, cell_opt(cp), cx, st));
        if ((rc = tsgemm_deferred(t, mt.xs[rec.it], DIN, t->ga, H3, mb.n_dst, DIN, H3, gk, gb_in, st)) ||
            (rc = tsgemm_deferred(t, hin, H, t->gu, H3, mb.n_dst, H, H3, grk, gb_rec, st)) ||
            (!cp.reset_after && (rc = tsgemm_deferred(t, t->rh, H, t->gu2, H3, mb.n_dst, H, H3, grk, nullptr, st))))
          return rc;
      } else if (dw && du) {
        HIP_TRY(launch_sum_gru_bwd_fused(a, DIN, H, dw->part + dw->used * (int64_t)(DIN + 1) * H3,
                                         du->part + du->used * (int64_t)(H + 1) * H3, st));
        dw->used += fw;
        du->used += fw;
      } else {
        HIP_TRY(launch_sum_gru_bwd(a, DIN, H, st));
        if ((rc = tsgemm_deferred(t, mt.xs[rec.it], DIN, t->ga, H3, mb.n_dst, DIN, H3, gk, gb, st)) ||
            (rc = tsgemm_deferred(t, hin, H, t->gu, H3, mb.n_dst, H, H3, grk, gb + H3, st)))
          return rc;
      }
      if (mp.aggr == IGN_AGGR_ATTENTION) {   // AUX:287-343 (see train_kernels.hip)
        if ((rc = attention_weights(p, b, mp, mb, srcs, hin, st))) return rc;   // this instance's weights
        const int F = DIN;
        SrcBases sb{};
        for (size_t s = 0; s < mp.src.size(); ++s) sb.base[s] = srcs[s];
        AttnArgs aa{mb.d_group_ptr, mb.d_group_empty, mb.d_cell_dst, mb.d_cell_ptr, mb.d_cell_msgs, mb.d_msg_src,
                    {mb.d_s_src[0], mb.d_s_src[1], mb.d_s_src[2], mb.d_s_src[3]}, mb.d_s_dst, mb.d_ecell, mb.d_msg_w,
                    mb.n_groups};
        const float* w12 = p->d_packed + p->pk_w12;
        HIP_TRY(hipMemsetAsync(t->adw12, 0, 2 * p->attn_F * sizeof(float), st));
        HIP_TRY(launch_attn_bwd_parts(aa, t->dx, mt.amdst, sb, F, mb.n_msgs, t->adw, t->adv, st));
        for (size_t s = 0; s < mp.src.size(); ++s) {
          // over a message network the source rows are its per-edge messages: their gradient goes
          // through the network's backward to the states it read (GM:440-475)
          const bool net = !mp.nn[s].layers.empty();
          const int64_t rows_s = net ? mb.n_edges[s] : b->rows[mp.src[s].entity];
          if (net) HIP_TRY(hipMemsetAsync(t->dmsg, 0, rows_s * F * sizeof(float), st));
          HIP_TRY(launch_attn_src_bwd(rows_s, mt.asptr[s], mt.asidx[s], mb.d_msg_w, t->adv, mt.amdst, t->dx, w12, F,
                                      net ? t->dmsg : src_grad(s), t->ads_src, st));
          HIP_TRY(launch_tsgemm_add(srcs[s], F, t->ads_src, 1, rows_s, F, 1, t->part, t->adw12, nullptr, st));
          if (net && (rc = msg_net_backward(p, b, t, mp, mb, mt, (int)s, src_grad(s), dh_out, grads, st))) return rc;
        }
        HIP_TRY(launch_attn_dst_bwd(mb.n_dst, mb.d_order, mb.d_msg_ptr, t->adv, w12 + p->attn_F, H, dh_out, t->ads_dst,
                                    st));
        HIP_TRY(launch_tsgemm_add(hin, H, t->ads_dst, 1, mb.n_dst, H, 1, t->part, t->adw12 + p->attn_F, nullptr, st));
        HIP_TRY(launch_attn_param_bwd(t->adw12, p->d_params + p->off_k1, p->d_params + p->off_k2,
                                      p->d_params + p->off_att, p->attn_F, grads + p->off_k1, grads + p->off_k2,
                                      grads + p->off_att, st));
        dcur[dst] = 1 - dcur[dst];
        return IGN_OK;
      }
      const float* dmsgs = t->dx;   // gradient of the aggregated messages, by destination row
      if (mp.aggr == IGN_AGGR_CONVOLUTION) {
        // x = act((s.K + h) / deg): du = dx act'(x) / deg, dh += du, dK += s^T du, ds = du K^T
        float* du = t->dtab;
        float* ds = t->dtab + mb.n_dst * DIN;
        HIP_TRY(launch_conv_bwd(t->dx, mt.xs[rec.it], mt.deg, mb.n_dst, DIN, mp.act, du, dh_out, st));
        HIP_TRY(launch_tsgemm_add(mt.ss[rec.it], DIN, du, DIN, mb.n_dst, DIN, DIN, t->part, grads + p->off_conv, nullptr, st));
        HIP_TRY(launch_row_gemm_t_generic(du, mb.n_dst, DIN, p->d_params + p->off_conv, DIN, ds, 0, -1, nullptr, st));
        dmsgs = ds;
      }
      for (size_t s = 0; s < mp.src.size(); ++s) {
        const bool net = !mp.nn[s].layers.empty();
        float* target = net ? t->dmsg : src_grad(s);
        HIP_TRY(launch_csr_gather_add(target, mt.trows[s], mt.tptr[s], mt.tidx[s], dmsgs, DIN, net ? 0 : 1, st));
        if (net && (rc = msg_net_backward(p, b, t, mp, mb, mt, (int)s, src_grad(s), dh_out, grads, st))) return rc;
      }
    }
    dcur[dst] = 1 - dcur[dst];
  }
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

int ign_batch_enable_edge_param_gradients(ign_plan* p, ign_batch* b) {
  if (!p || !b) return fail(IGN_ERR_INVALID, "null argument");
  if (b->plan != p) return fail(IGN_ERR_INVALID, "batch was created for another plan");
  if (!b->train) return fail(IGN_ERR_INVALID, "training not enabled on this batch (ign_batch_enable_training)");
  TrainState* t = b->train;
  if (t->edge_grads) return IGN_OK;
  int rc = set_device(p->device);
  if (rc) return rc;
  for (size_t mi = 0; mi < p->mps.size(); ++mi)
    for (size_t s = 0; s < p->mps[mi].src.size(); ++s) {
      const MsgNN& nn = p->mps[mi].nn[s];
      if (nn.layers.empty() || std::find(nn.inputs.begin(), nn.inputs.end(), (int)IGN_MSG_EDGE_PARAMS) == nn.inputs.end())
        continue;
      if (!t->mp[mi].dprm[s] && (rc = talloc(t, &t->mp[mi].dprm[s], b->mp[mi].n_edges[s] * nn.param_dim))) return rc;
    }
  t->edge_grads = true;
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
