// dense_stack.h — one walk over a Dense stack (gemm, bias, activation, Dropout and
// LayerNormalization layers) and its
// reverse, for every stack of the training step: predict (p->dense), a readout neural_network
// operation (RoOp::layers), a message-creation network (MsgNN::layers).  Which Dropout and
// LayerNormalization layers stand in front of which Dense layer, and in what order, is the stack's
// seq (plan_lower.h), written at plan time: the walks index into it.  Each layer's kernels
// follow from its pk_* slots (plan_lower.cpp's layout_packed): only predict's layers have more
// than pk_w, so the other two end in launch_dense_fwd and launch_row_gemm_t_generic.
#pragma once
#include "engine_internal.h"

namespace ign {

// One stack for one run: a view, it owns nothing.
struct DenseStackRun {
  const DenseP* layers = nullptr;
  int L = 0;
  int64_t n = 0;                    // rows
  const float* x = nullptr;         // input rows, ldx floats apart (a message network's: layers[0].in
  int ldx = 0;                      // padded with zero columns to a multiple of 16; else layers[0].in)
  float* const* hid = nullptr;      // outputs of layers 0 .. L-2
  float* y = nullptr;               // the last layer's output, behind the sites after it
  const DropRun* drop = nullptr;    // Dropout: the forward's mask stream; null = seq's Dropout layers do not run (inference)
  const std::vector<StackLayer>* seq = nullptr;   // the stack's layers in order; null = Dense layers only (message networks)
  const NormRun* norm = nullptr;    // LayerNormalization: the run's buffers; null = seq's do not run
  // backward
  const float* dy = nullptr;        // d(y)
  float* const* gz = nullptr;       // two layer-gradient buffers (ping-pong) [n][widest]
  float* part = nullptr;            // weight-gradient partial tiles (launch_tsgemm_add)
  float* grads = nullptr;
  const float* l2_scale = nullptr;  // weight of the layers' l2 terms; null = none added here (a message
                                    // network's are added once per step, not per MP instance)
  float* dx = nullptr;              // d(x) [n][layers[0].in]: added to (dx_acc = 1: a tensor's gradient) or
  int dx_acc = 0;                   // overwritten (0: a scratch the caller splits or gathers from)
};

int dense_stack_forward(const ign_plan* p, const DenseStackRun& r, hipStream_t st);
// Weight / bias gradients and l2 terms into grads, d(x) into dx.  May write gradient rows over
// hid[L - 2] (the 1-unit output layer's fusion): one backward per forward.
int dense_stack_backward(const ign_plan* p, const DenseStackRun& r, hipStream_t st);

// the l2 kernel regularizer's gradient (AUX:833-834) of Dense layer d: grads[W] += 2 l2 scale W
int add_l2_grad(const ign_plan* p, const DenseP& d, float* grads, float scale, hipStream_t st);

}  // namespace ign
