// plan_lower.h — the plan lowering of ign_plan_create, separate from the device: an ign_plan_desc
// and the plan-level switches become a PlanModel (the validated model, every readout Dense stack's
// layers as one ordered list, the raw parameter layout, the packed-fragment layout and the list of
// pack launches that fills it), plain host data.  No HIP
// header: plan_lower.cpp builds with a plain C++17 compiler (tests/cpp/plan_lower_check.cpp, run
// under the sanitizers).  engine.cpp's ign_plan derives from PlanModel and adds the device side.
#pragma once
#include "host_types.h"
#include "kernel_shapes.h"

namespace ign {

struct Tensor {
  int kind, owner;
  int64_t offset;
  int rows, cols;
};

// readout program (GM:611-655): tensors on row spaces, operations before predict
enum { RS_ENTITY = 0, RS_GRAPH = 1, RS_ADJ = 2 };
struct RoTensor {
  int space = RS_ENTITY, sid = 0;   // sid: entity or adjacency slot
  int width = 0;
  bool same_space(const RoTensor& o) const { return space == o.space && (space == RS_GRAPH || sid == o.sid); }
};
// One layer of a readout Dense stack, in the architecture's order.  idx: the Dense layer of the
// stack, or the site in PlanModel::drops / PlanModel::norms.  A stack's list reads: the layers in
// front of Dense 0, Dense 0, those in front of Dense 1, ..., the last Dense, the layers after it.
// Everything that needs to know which layer follows which walks this list; nothing else orders them.
enum { SL_DENSE = 0, SL_DROPOUT = 1, SL_LAYERNORM = 2 };
struct StackLayer {
  int kind, idx;
};
struct RoOp {
  int type = 0, mode = 0, adj = -1;
  std::vector<int> in;            // tensor ids
  std::vector<DenseP> layers;     // IGN_RO_NEURAL_NETWORK
  std::vector<StackLayer> seq;    // ... and all its layers in order
  int in_width = 0;               // neural_network: concatenated input width
  int out = -1;                   // first output tensor id
};

// A Dropout layer of a readout Dense stack (ign_plan_add_dropout): live in training only.  The
// plan keeps them in site order: readout ops in order, then predict; within a stack by position,
// then by insertion.  A site's ordinal is its index there: its Philox counter word and its slot in
// DropRun::buf.  Where it stands among the LayerNormalization layers is the stack's seq.
struct DropSite {
  int stack = -1;        // readout-op index, or -1 for predict
  int before = 0;        // Dense layer it precedes; the stack's layer count = after the last one
  float rate = 0.f, scale = 1.f;
  uint64_t seed = 0;     // the layer's own seed option, xor-mixed into the batch's stream seed
  int units = 0;         // the width it masks: the input width of `before`, or the stack's output width
};

// A LayerNormalization layer of a readout Dense stack (ign_plan_add_layernorm): live in inference and
// in training.  Kept like the Dropout sites (readout ops in order, then predict; by position, then
// by insertion), numbered on their own: a Dropout site's number, its Philox counter word, counts
// Dropout layers only.  Its index is its slot in NormRun::buf / stats and ign_batch::d_norm, and its
// tensors' owner.
struct NormSite {
  int stack = -1;        // readout-op index, or -1 for predict
  int before = 0;        // Dense layer it precedes; the stack's layer count = after the last one
  float epsilon = 1e-3f;
  int64_t off_gamma = -1, off_beta = -1;   // [units] each; -1: scale / center false, no tensor
  bool center = true, scale = true;
  int units = 0;         // the width it normalises: the input width of `before`, or the stack's output width
};

// The plan-level switches.  engine.cpp's switches_from_env fills them from the IGN_* environment
// once per ign_plan_create; nothing else reads the environment for them.
struct PlanSwitches {
  int readout_variant = 4;        // fused readout: 4 = both layers on split-fp16 (3 products) on 16x16x32 MFMAs
                                  // (readout_h16), 5 = the same on 32x32x16 (readout_h32.hip, slower: DESIGN
                                  // §3b), 1 = f32
                                  // MFMA (readout3), 2 = split-bf16 x6 (readout_bf); IGN_READOUT_VARIANT
  int seq_variant = 6;            // ordered update: 6 = split-fp16 h.U with 3 piece products (H = 32,
                                  // 64), 4 = split-bf16 x6, 2 = f32 MFMA; IGN_SEQ_VARIANT
  int xcd_remap = 0;              // XCD-aware tile order in the GRU kernels (placement only; off:
                                  // measured slower, profiles/r02/seq_experiments)
  bool fuse_proj = true;          // sum_gru_g32 projects for the next ordered MP (IGN_FUSE_PROJ=0: off)
  int sum_variant = 8;            // sum update: 8 = split-fp16 GRU step at DIN = H = 64 and split-bf16
                                  // at 32, 7 = split-bf16 at both, 3 = f32 MFMA; IGN_SUM_VARIANT
  bool train_dense_bf = true;     // training forward's Dense layers on dense_bf (IGN_TRAIN_DENSE_BF=0: f32)
  bool train_dense_h16 = true;    // ... on the split-fp16 form of dense_bf (IGN_TRAIN_DENSE_H16=0: split-bf16;
                                  // lower_plan turns it off for a plan that names `exponential`)
  bool tsgemm_bf = true;          // weight-gradient row contractions on tsgemm_bf (IGN_TSGEMM_BF=0: f32 MFMA)
  bool train_fused_readout = true;   // training forward's readout on readout_h16 with saves (IGN_TRAIN_FUSED_READOUT=0: per layer)
  bool fuse_outer_bwd = true;     // 1-unit output layer's backward formed on the fly (IGN_FUSE_OUTER_BWD=0: row_outer_t)
  bool bwd_bf = true;             // ordered backward's gate recompute on split-bf16 (IGN_BWD_BF=0: f32 MFMA)
  bool train_seq_h16 = true;      // training forward's ordered update on split-fp16 (IGN_TRAIN_SEQ_H16=0: bf16)
  bool bwd_fuse = true;           // ordered backward forms dU in the kernel (IGN_BWD_FUSE=0: tsgemm)
  bool sum_bwd_fuse = true;       // sum backward forms dW / dU in the kernel (IGN_SUM_BWD_FUSE=0: tsgemm)
  bool defer_wgrad = true;        // the sum and ordered MPs' weight-gradient partials reduced once per backward
                                  // (IGN_DEFER_WGRAD=0: per MP instance)
  bool train_csr_gpu = true;      // the training tables' transposed CSRs built on the GPU (train_csr.hip;
                                  // IGN_TRAIN_CSR_GPU=0: on the host, train_lower.cpp)
  bool resident = true;           // graph-resident forward for small RouteNet-shaped graphs (IGN_RESIDENT=0: off)
  bool resident_pg = true;        // ... with the path states in global memory where they do not fit LDS (IGN_RESIDENT_PG)
  bool resident_path_global = false;   // IGN_RESIDENT=2: that form for every eligible batch (tests)
  bool resident_train = true;     // the training forward on the resident form's SAVE variant (IGN_RESIDENT_TRAIN=0: off)
  bool resident_eager = true;     // a batch's resident tables built in ign_batch_create (IGN_RESIDENT_EAGER=0: at
                                  // its first forward)
  bool res_lpt = true;            // resident workgroups take their graphs longest first (IGN_RES_LPT=0: batch order)
  int res_group = 0;              // consecutive graphs per resident workgroup (IGN_RES_GROUP; 0: auto, 1 or 2)
  bool resident_save_table = true;   // ... which also saves the ordered MP's tables (IGN_RESIDENT_SAVE_TABLE=0: recompute)
  int sum_window = -1;            // IGN_SUM_WINDOW: 1 windowed sum aggregation where eligible; -1 (default)
                                  // segmented for destinations of >= 64 messages, 0 of >= 128, 2 for all.
                                  // (The windowed form:)
                                  // Measured 0.120 vs 0.112 ms (RouteNet link update, 37 messages per link);
                                  // Q-size x512 7.33 -> 6.44 ms/step with both sum MPs windowed
  bool use_graph = true;          // replay ign_forward as one captured hipGraph; IGN_HIP_GRAPH=0 disables
  bool dead_last = true;          // the resident ign_forward leaves out the last iteration's MPs that are dead_in_last_iter
                                  // (ign_batch_state runs them on demand); IGN_DEAD_LAST=0: every MP runs
};

// One slot of d_packed and the pack launch that fills it from the raw parameters (ign::repack runs
// the list in order after every parameter update).  src: offsets into the raw parameters (-1: a null
// pointer); dst, floats: the slot; a, b, c: the launch's integer arguments.
enum {
  PK_GRU,           // pack_gru(W, U, bias; din a, H b): dst = W's slot; the PK_GRU_U and PK_GRU_B records
  PK_GRU_U,         //   that follow name its U and bias slots and launch nothing themselves
  PK_GRU_B,
  PK_GRU_W,         // pack_gru with W alone (an axis-2 concat slice; din a, H b)
  PK_U_BF16,        // pack_u_bf16(U; H a)
  PK_U_F16,         // pack_u_f16(U; H a)
  PK_UT_F16,        // pack_ut_f16(U; H a)
  PK_W_F16,         // pack_w_f16(W; K a, H b)
  PK_W_BF16,        // pack_w_bf16(W; K a, H b)
  PK_A,             // pack_a(M; rows a, cols b)
  PK_DENSE_PAD,     // pack_dense_pad(W; IN a, IN_pad b, OUT c)   (pack_dense: IN_pad = IN)
  PK_DENSE_BF16,    // pack_dense_bf16(W; IN a, OUT b, chained c)
  PK_DENSE_BF16_T,  // pack_dense_bf16_t(W; IN a, OUT b)
  PK_DENSE_F16,     // pack_dense_f16(W; IN a, OUT b, trans c)
  PK_READOUT_H16,   // pack_readout_h16(W1, b1, W2; in1 a, n1 b, n2 c)
  PK_READOUT_H32,   // pack_readout_h32(the same)
  PK_ATTN_VECTORS,  // attn_vectors(K1, K2, a; F a)
};
struct PackJob {
  int kind;
  int64_t src[3];
  int64_t dst;
  int a, b, c;
  int64_t floats;
};

struct PlanModel : PlanSwitches {
  int T = 0;
  std::vector<ign_entity_desc> ents;
  int n_adj = 0, n_il = 0;
  std::vector<MPP> mps;
  std::vector<CellP> cells;
  bool any_cell_options = false;  // a cell is not a default cell (layout_packed sets it)
  std::vector<int> ro_in;         // predict inputs: readout tensor ids
  std::vector<DenseP> dense;
  std::vector<StackLayer> seq;    // predict's layers in order (dense: its Dense layers)
  std::vector<RoTensor> ro_t;     // readout tensors: entity states, then the op outputs
  std::vector<RoOp> ro_ops;
  std::vector<int> adj_src_ent, adj_dst_ent;   // per adjacency slot (from the MPs that read it)
  // one convolution / attention weight set per plan (GM:288-300: the last MP's weights serve all)
  int conv_F = 0, attn_F = 0;
  int64_t off_conv = -1, off_k1 = -1, off_k2 = -1, off_att = -1;
  int64_t pk_conv = -1, pk_w12 = -1;
  std::vector<Tensor> tensors;
  int64_t n_params = 0, n_packed = 0;
  std::vector<PackJob> packs;     // every slot of [0, n_packed), in launch order
  bool fused_readout = false;
  int ro_width = 0;
  std::vector<DropSite> drops;    // Dropout sites of the readout stacks, in site order (rate > 0 only)
  std::vector<NormSite> norms;    // LayerNormalization layers of the readout stacks, in the same order
};

// the Dense layers of `stack` (-1 predict, k readout neural_network operation k), or null
inline const std::vector<DenseP>* stack_layers(const PlanModel* p, int stack) {
  if (stack == -1) return &p->dense;
  if (stack < 0 || stack >= (int)p->ro_ops.size() || p->ro_ops[stack].type != IGN_RO_NEURAL_NETWORK) return nullptr;
  return &p->ro_ops[stack].layers;
}
// ... and all of the stack's layers in order, or null
inline const std::vector<StackLayer>* stack_seq(const PlanModel* p, int stack) {
  return !stack_layers(p, stack) ? nullptr : stack == -1 ? &p->seq : &p->ro_ops[stack].seq;
}
// a site's place among the Dropout and LayerNormalization layers in front of the same Dense layer
inline int site_order(const PlanModel* p, int stack, int kind, int idx) {
  int n = 0;
  for (const StackLayer& e : *stack_seq(p, stack)) {
    if (e.kind == kind && e.idx == idx) break;
    n = e.kind == SL_DENSE ? 0 : n + 1;
  }
  return n;
}
// ign_plan_add_dropout / ign_plan_add_layernorm on the model: the site enters drops / norms at its
// place in site order and the stack's seq in front of Dense layer before_layer, behind the layers
// already there.  A rate of 0 adds nothing (tf.nn.dropout returns x).  A LayerNormalization brings
// its gamma / beta tensors (kinds 13 / 14, in front of the Dense layer it precedes) and both layouts
// again, and predict's stack leaves the fused readout: only before the parameters exist on a device
// (the caller checks).
int add_dropout(PlanModel* p, int stack, int before_layer, float rate, uint64_t layer_seed);
int add_layernorm(PlanModel* p, int stack, int before_layer, float epsilon, int center, int scale);
// ign_plan_set_cell_options on the model: the options enter CellP and both layouts run again (the bias
// tensor [2][3H], [3H] or absent; a cell with options packs pack_gru's unscaled form and none of the
// split pieces, which takes it off the resident, split and fused paths).  IGN_ERR_INVALID for a bad
// cell index or activation code.  Only before the parameters exist on a device (the caller checks).
int set_cell_options(PlanModel* p, int cell, const ign_cell_options* o);

// d + sw -> *m (a fresh PlanModel); IGN_OK or the refusal's code, its text in ign_last_error
int lower_plan(const ign_plan_desc* d, const PlanSwitches& sw, PlanModel* m);
// MPP::dead_in_last_iter of every MP (lower_plan calls it): a property of the model alone, whatever
// PlanSwitches::dead_last says.  MP m into entity e is dead when no readout operation and no predict
// input reads e's states, no later MP of the iteration reads them (as a source or as its own
// destination), and no later MP writes an entity m reads: then the update can also run after the
// forward, from the states the forward left, with the same result.  Anything else keeps the MP live.
void mark_dead_last(PlanModel* m);

// The activation codes a position of the model takes.  Predict's Dense layers take all ten.  Three
// position / code pairs, and softplus as a convolution activation, stay refused as they were before
// elu .. hard_sigmoid were lowered: the kernels make no such difference.
enum { ACT_AT_PREDICT, ACT_AT_READOUT_OP, ACT_AT_MESSAGE, ACT_AT_CONVOLUTION };
inline bool act_ok(int a, int at) {
  if (a < IGN_ACT_LINEAR || a > IGN_ACT_HARD_SIGMOID) return false;
  switch (at) {
    case ACT_AT_READOUT_OP: return a != IGN_ACT_ELU;
    case ACT_AT_MESSAGE: return a != IGN_ACT_HARD_SIGMOID;
    case ACT_AT_CONVOLUTION: return a != IGN_ACT_SOFTPLUS && a != IGN_ACT_HARD_SIGMOID;
    default: return true;
  }
}

// the training forward's ordered update: split-fp16 x3 with state saving (seq_gru_h16<SAVE>) where
// the backward can recompute its gates bitwise (fused seq_gru_bwd, H = 32; IGN_TRAIN_SEQ_H16=0: the
// split-bf16 x6 form), else split-bf16 x6 / f32
inline int train_seq_variant(const PlanModel* p, int H) {
  if (p->seq_variant == 6 && H == 32 && p->train_seq_h16 && p->bwd_bf && p->bwd_fuse) return 6;
  return p->seq_variant >= 6 ? 4 : std::max(2, p->seq_variant);
}

}  // namespace ign
