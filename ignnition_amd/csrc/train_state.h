// train_state.h — the training state of a batch (ign_batch::train) and the helpers its units share:
// train_alloc.cpp builds it (ign_batch_enable_training), train.cpp runs the step on it and
// mp_backward.cpp the backward of one MP instance.  engine.cpp sees the forward declaration only.
#pragma once
#include "engine_internal.h"

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

namespace ign {

// train_alloc.cpp: n floats (plus a pad) of the batch's pool into *out, released with the state
int talloc(TrainState* t, float** out, int64_t n);

// h on the device, in a block released with the state (the one definition: a template)
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

// mp_backward.cpp: C (+ Cb) += A^T B over n_rows rows, its partial tiles parked for
// ign_backward_end's reduction when C has a deferred slot with room (else reduced now, as
// launch_tsgemm_add); the flush reduces every slot in use, the fused ordered backward's first
int tsgemm_deferred(TrainState* t, const float* A, int lda, const float* B, int ldb, int64_t n_rows, int M, int N,
                    float* C, float* Cb, hipStream_t st);
int tsgemm_deferred_flush(const ign_plan* p, TrainState* t, hipStream_t st);

// train.cpp: what every training entry point checks first
int check_train(ign_plan* p, ign_batch* b);

}  // namespace ign
