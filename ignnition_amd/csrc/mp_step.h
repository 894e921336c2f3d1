// mp_step.h — one message-passing (MP) instance forward, for ign_forward_mp (engine.cpp), for
// ign_forward_train_mp (train.cpp) and, its message networks and projected table, the recompute of
// the instance's backward (mp_backward.cpp).  What depends on the mode hangs on the save record
// (DESIGN.md §2).
#pragma once
#include "engine_internal.h"
#include "gru_cell.h"

namespace ign {

// the options of a cell as gru_cell.hip's kernels take them
inline CellOpt cell_opt(const CellP& cp) { return CellOpt{cp.act, cp.ract, cp.reset_after ? 1 : 0}; }

// Event pairs around the launches of one kind into the plan's ring (ign_plan_set_timing), resolved
// lazily by flush_timing; a null plan never records (the training forward and the backward).
struct Timer {
  ign_plan* p;
  bool on = false;
  void begin(int kind, double flops, double bytes, double mfma_bf16 = 0, double mfma_f32 = 0);
  void end();
};
int flush_timing(ign_plan* p);   // engine.cpp: the pending pairs into p->stats (one host wait)

// the states one MP instance reads and writes, resolved by the caller (ping-pong buffers or versions)
struct MpStates {
  SrcBases src{};
  const float* hin = nullptr;
  float* hout = nullptr;
};
// what the training forward keeps for its backward; all null: inference
struct MpSave {
  float* hs = nullptr;    // ordered: SeqGruArgs::hs_save
  float* x = nullptr;     // sum: SumGruArgs::x_save
  float* sum = nullptr;   // convolution: SumGruArgs::sum_save
  bool any() const { return hs || x || sum; }
};

// The message-creation networks of MP instance (mp, mb) (GM:440-475), each from src[s] and hin into
// mb.d_msg_layer[s]; src[s] then names the last layer's rows, the messages.
int mp_message_nets(ign_plan* p, const MPP& mp, const MPB& mb, const float** src, const float* hin, hipStream_t st);
// Sorted MP: every source not in the `projected` mask through the input kernel into mb.d_table (an
// axis-2 concat: through its own row slice, AUX:443-456), then the pre-summed rows.
int mp_project(ign_plan* p, const MPP& mp, const MPB& mb, const float* const* src, int projected, Timer& tm);
// attention weights of one MP instance (AUX:287-343) into mb.d_msg_w (scores in mb.d_s_src / d_s_dst)
int attention_weights(ign_plan* p, ign_batch* b, const MPP& mp, const MPB& mb, const float* const* srcs,
                      const float* hin, hipStream_t st);
// MP instance mi forward on destinations `part`: s.hin -> s.hout.  No host synchronisation and no
// allocation: it runs inside ign_forward's stream capture.
int mp_forward(ign_plan* p, ign_batch* b, int mi, int part, MpStates s, const MpSave& save, Timer& tm);

}  // namespace ign
