// mp_backward.cpp — the backward of one MP instance (GM:404-603 under tf.gradients, GM:790), built
// from stages: the cell backward (ordered or sum, each in three forms: a cell with options, the fused
// kernel, the unfused kernel plus row contractions), then the aggregation's (attention, convolution)
// and the sources' message gradients.  A source with a message network takes its gradient through
// the network's backward (msg_net_backward) to the states it read.  Host dispatch only: the kernels
// are train_kernels.hip's and gru_cell.hip's.

#include <hip/hip_runtime.h>

#include "dense_stack.h"
#include "mp_backward.h"
#include "mp_step.h"
#include "train_kernels.h"

namespace ign {

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

namespace {

// One MP instance of a backward, resolved once, and its stages.  Each stage's comment says what it
// reads and what it leaves, and where.
struct MpBwd {
  ign_plan* p;
  ign_batch* b;
  TrainState* t;
  hipStream_t st;
  const MPRec& rec;
  const MPP& mp;
  const MPB& mb;
  const CellP& cp;
  const MPTrain& mt;
  const int H, DIN, H3;
  // per source: its state rows (after mp_message_nets, over a message network: its messages)
  const float* srcs[IGN_MAX_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
  const float* hin;   // the destination's input version
  float* dh_in;       // dLoss/d(output version), given
  float* dh_out;      // dLoss/d(input version), formed here
  // the cell's gradients.  A cell with options (gru_cell.hip): the bias gradients in the [3H] layout
  // or nowhere, and for reset_after = false the second pair of rows whose contraction completes dU
  float* gk;
  float* grk;
  float* gb_in;
  float* gb_rec;
  CellBwdExtra cx{};

  MpBwd(ign_plan* p_, ign_batch* b_, TrainState* t_, const MPRec& r)
      : p(p_), b(b_), t(t_), st(p_->stream), rec(r), mp(p_->mps[r.mi]), mb(b_->mp[r.mi]), cp(p_->cells[mp.cell]),
        mt(t_->mp[r.mi]), H(cp.H), DIN(mp.din), H3(3 * cp.H) {
    const int dst = mp.dst;
    float* gb = t->grads + cp.off_b;
    for (size_t s = 0; s < mp.src.size(); ++s) srcs[s] = t->ver[mp.src[s].entity][rec.src_v[s]];
    hin = t->ver[dst][rec.v_in];
    dh_in = t->dS[t->dcur[dst]][dst];
    dh_out = t->dS[1 - t->dcur[dst]][dst];
    gk = t->grads + cp.off_k;
    grk = t->grads + cp.off_rk;
    gb_in = cp.use_bias ? gb : nullptr;
    gb_rec = cp.use_bias && cp.reset_after ? gb + H3 : nullptr;
    if (!cp.reset_after) {
      cx.gu2 = t->gu2;
      cx.rh = t->rh;
    }
  }
  float* src_grad(size_t s) const {   // where d(state of source s) accumulates
    const int se = mp.src[s].entity;
    return se == mp.dst ? dh_out : t->dS[t->dcur[se]][se];
  }
  bool has_net(size_t s) const { return !mp.nn[s].layers.empty(); }

  int msg_net_backward(int s) const;
  template <typename Launch>
  int into_source(size_t s, bool zero_first, Launch launch) const;
  int ordered_cell_backward() const;
  int ordered_source_backward(size_t s) const;
  int sum_cell_backward() const;
  int attention_backward() const;
  int convolution_backward(const float** dmsgs) const;
  int sum_sources_backward(const float* dmsgs) const;
};

// Backward of MP source s's message-creation network (GM:440-475), given d(messages) in t->dmsg:
// Dense stack in reverse (weight / bias gradients; the l2 terms are added once per step by
// ign_backward, not per MP instance), then the hs_source / hs_dest column
// slices of d(input) gathered back to the state rows they were read from.  The layer activations
// are the ones mp_message_nets left in mb (recomputed for this MP instance by the caller).
int MpBwd::msg_net_backward(int s) const {
  const MsgNN& nn = mp.nn[s];
  DenseStackRun r{nn.layers.data(), (int)nn.layers.size(), mb.n_edges[s], mb.d_msg_in[s], nn.din_pad,
                  mb.d_msg_layer[s].data(), mb.d_msg_layer[s].back()};
  r.dy = t->dmsg;
  r.gz = t->mz;
  r.part = t->part;
  r.grads = t->grads;
  r.dx = t->mdin;   // overwritten: gathered below
  if (int rc = dense_stack_backward(p, r, st)) return rc;
  int col = 0;
  for (size_t q = 0; q < nn.inputs.size(); ++q) {
    const int w = nn.widths[q];
    if (nn.inputs[q] == IGN_MSG_HS_SOURCE)
      HIP_TRY(launch_csr_gather_cols_add(src_grad(s), b->rows[mp.src[s].entity] + b->halo[mp.src[s].entity],
                                         mt.nsrc_ptr[s], mt.nsrc_idx[s], t->mdin, nn.din, col, w, 1, st));
    else if (nn.inputs[q] == IGN_MSG_HS_DEST)
      HIP_TRY(launch_csr_gather_cols_add(dh_out, b->rows[mp.dst], mt.ndst_ptr[s], mt.ndst_idx[s], t->mdin, nn.din,
                                         col, w, 1, st));
    else if (nn.inputs[q] == IGN_MSG_EDGE_PARAMS && t->edge_grads_live)   // input data: its gradient only on request
      HIP_TRY(launch_slice_cols_add(t->mdin, mb.n_edges[s], nn.din, col, w, mt.dprm[s], st));
    col += w;
  }
  return IGN_OK;
}

// The tail every source loop shares.  launch(target, accumulate) leaves source s's message gradient:
// added to src_grad(s), or, over a message network, written to t->dmsg (zeroed first where the
// launch adds into it), from where the network's backward takes it to the states it read.
template <typename Launch>
int MpBwd::into_source(size_t s, bool zero_first, Launch launch) const {
  const bool net = has_net(s);
  if (net && zero_first) HIP_TRY(hipMemsetAsync(t->dmsg, 0, mb.n_edges[s] * DIN * sizeof(float), st));
  if (int rc = launch(net ? t->dmsg : src_grad(s), net ? 0 : 1)) return rc;
  return net ? msg_net_backward((int)s) : IGN_OK;
}

// Ordered cell backward.  Reads dh_in, the per-step states mt.hs and the instance's projected table
// (the resident training forward's saved one, else recomputed into mb.d_table); leaves dh_out, da
// per step in t->ga, and dU and the bias gradients in grads or the cell's deferred slot.
int MpBwd::ordered_cell_backward() const {
  // the forward's table of this instance: saved by the resident training forward, else recomputed
  const bool saved = t->tab_saved && rec.mi == 0 && rec.it < (int)t->tsave.size();
  Timer untimed{nullptr};
  if (!saved)
    if (int rc = mp_project(p, mp, mb, srcs, 0, untimed)) return rc;
  SeqBwdArgs a{mt.hs[rec.it], saved ? t->tsave[rec.it] : mb.d_table, mb.d_order, mb.d_len, mb.d_step_ptr, mb.d_step_code,
               p->d_packed + cp.pk_u, p->d_packed + cp.pk_b, p->d_packed + cp.pk_ut, dh_in, dh_out,
               t->ga, t->gu, mb.n_dst};
  a.h_in = hin;
  a.hdr = mt.hdrb;
  if (!cp.is_default()) {
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
    a.db_rec = gb_rec;
    a.db_in = gb_in;
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
    HIP_TRY(launch_tsgemm_add(mt.hs[rec.it], H, t->gu, H3, mt.hs_rows, H, H3, t->part, grk, gb_rec, st));
    HIP_TRY(launch_colsum_add(t->ga, H3, mb.n_steps, H3, t->part, gb_in, st));
  }
  return IGN_OK;
}

// Ordered source s.  Reads da in t->ga; leaves d(table rows of s) in t->dtab, the input-kernel
// gradient in grads (its slice under feature_concat) or a deferred slot, and d(source rows) where
// into_source puts it.
int MpBwd::ordered_source_backward(size_t s) const {
  const int se = mp.src[s].entity;
  HIP_TRY(launch_csr_gather_add(t->dtab, mt.trows[s], mt.tptr[s], mt.tidx[s], t->ga, H3, 0, st));
  // dW = x^T dtab over the source rows.  A row that no step reads has a zero dtab row, but in a plan
  // with a convolution MP it may hold 0 / 0 (a destination without a message, AUX:384-401): NaN * 0.
  // Autograd gathers the read rows only, so there the unread rows enter as zeros
  const float* xs = srcs[s];
  if (t->rsrc && !has_net(s)) {
    HIP_TRY(launch_read_rows(srcs[s], mt.tptr[s], mt.trows[s], mp.feature_concat ? p->ents[se].hidden_dim : DIN,
                             t->rsrc, st));
    xs = t->rsrc;
  }
  if (mp.feature_concat) {   // AUX:443-456: the source's slice of the input kernel
    const int sdin = p->ents[se].hidden_dim;
    const int64_t koff = (int64_t)mp.slice_off[s] * H3;
    HIP_TRY(launch_tsgemm_add(xs, sdin, t->dtab, H3, mt.trows[s], sdin, H3, t->part, gk + koff, nullptr, st));
    return into_source(s, false, [&](float* target, int accumulate) -> int {
      HIP_TRY(launch_row_gemm_t_generic(t->dtab, mt.trows[s], H3, p->d_params + cp.off_k + koff, sdin, target,
                                        accumulate, -1, nullptr, st));
      return IGN_OK;
    });
  }
  if (int rc = tsgemm_deferred(t, xs, DIN, t->dtab, H3, mt.trows[s], DIN, H3, gk, nullptr, st)) return rc;
  return into_source(s, false, [&](float* target, int accumulate) -> int {
    HIP_TRY(launch_row_gemm_t(t->dtab, mt.trows[s], H3, p->d_packed + cp.pk_wt, DIN, target, accumulate, -1, nullptr, st));
    return IGN_OK;
  });
}

// Sum cell backward.  Reads dh_in, the aggregated messages mt.xs and hin; leaves dh_out, the
// gradient of the aggregated messages by destination row in t->dx, and dW, dU and the bias
// gradients in grads or the deferred slots.
int MpBwd::sum_cell_backward() const {
  int rc;
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
  if (!cp.is_default()) {
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
    if ((rc = tsgemm_deferred(t, mt.xs[rec.it], DIN, t->ga, H3, mb.n_dst, DIN, H3, gk, gb_in, st)) ||
        (rc = tsgemm_deferred(t, hin, H, t->gu, H3, mb.n_dst, H, H3, grk, gb_rec, st)))
      return rc;
  }
  return IGN_OK;
}

// Attention backward (AUX:287-343, see train_kernels.hip).  Reads t->dx and the instance's
// recomputed weights (mb.d_msg_w); leaves the message gradients with every source (into_source),
// the destination's score gradient added to dh_out, and d(w1 | w2 | attention kernel) in grads.
int MpBwd::attention_backward() const {
  if (int rc = attention_weights(p, b, mp, mb, srcs, hin, st)) return rc;   // this instance's weights
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
    const int64_t rows_s = has_net(s) ? mb.n_edges[s] : b->rows[mp.src[s].entity];
    const int rc = into_source(s, true, [&](float* target, int) -> int {
      HIP_TRY(launch_attn_src_bwd(rows_s, mt.asptr[s], mt.asidx[s], mb.d_msg_w, t->adv, mt.amdst, t->dx, w12, F, target,
                                  t->ads_src, st));
      HIP_TRY(launch_tsgemm_add(srcs[s], F, t->ads_src, 1, rows_s, F, 1, t->part, t->adw12, nullptr, st));
      return IGN_OK;
    });
    if (rc) return rc;
  }
  HIP_TRY(launch_attn_dst_bwd(mb.n_dst, mb.d_order, mb.d_msg_ptr, t->adv, w12 + p->attn_F, H, dh_out, t->ads_dst, st));
  HIP_TRY(launch_tsgemm_add(hin, H, t->ads_dst, 1, mb.n_dst, H, 1, t->part, t->adw12 + p->attn_F, nullptr, st));
  HIP_TRY(launch_attn_param_bwd(t->adw12, p->d_params + p->off_k1, p->d_params + p->off_k2,
                                p->d_params + p->off_att, p->attn_F, t->grads + p->off_k1, t->grads + p->off_k2,
                                t->grads + p->off_att, st));
  return IGN_OK;
}

// Convolution backward.  x = act((s.K + h) / deg): du = dx act'(x) / deg, dh += du, dK += s^T du,
// ds = du K^T.  Reads t->dx, mt.xs, mt.ss and mt.deg; leaves du and ds in t->dtab, du added to
// dh_out, dK in grads, and in *dmsgs the ds the scatter reads.
int MpBwd::convolution_backward(const float** dmsgs) const {
  float* du = t->dtab;
  float* ds = t->dtab + mb.n_dst * DIN;
  HIP_TRY(launch_conv_bwd(t->dx, mt.xs[rec.it], mt.deg, mb.n_dst, DIN, mp.act, du, dh_out, st));
  HIP_TRY(launch_tsgemm_add(mt.ss[rec.it], DIN, du, DIN, mb.n_dst, DIN, DIN, t->part, t->grads + p->off_conv, nullptr, st));
  HIP_TRY(launch_row_gemm_t_generic(du, mb.n_dst, DIN, p->d_params + p->off_conv, DIN, ds, 0, -1, nullptr, st));
  *dmsgs = ds;
  return IGN_OK;
}

// Sum sources.  Reads dmsgs, the gradient of the aggregated messages by destination row; scatters
// it over each source's transposed CSR to where into_source puts it.
int MpBwd::sum_sources_backward(const float* dmsgs) const {
  for (size_t s = 0; s < mp.src.size(); ++s) {
    const int rc = into_source(s, false, [&](float* target, int accumulate) -> int {
      HIP_TRY(launch_csr_gather_add(target, mt.trows[s], mt.tptr[s], mt.tidx[s], dmsgs, DIN, accumulate, st));
      return IGN_OK;
    });
    if (rc) return rc;
  }
  return IGN_OK;
}

}  // namespace

int mp_backward(ign_plan* p, ign_batch* b, TrainState* t, const MPRec& rec) {
  MpBwd c(p, b, t, rec);
  const int dst = c.mp.dst;
  int rc;
  if (b->halo[dst])   // a self-loop MP's source gradient lands in dh_out's halo rows too
    HIP_TRY(hipMemsetAsync(c.dh_out + b->rows[dst] * c.H, 0, b->halo[dst] * c.H * sizeof(float), c.st));
  // recompute this instance's message networks (and, in the ordered cell backward, its table): the
  // forward's routines, untimed
  if ((rc = mp_message_nets(p, c.mp, c.mb, c.srcs, c.hin, c.st))) return rc;
  if (c.mp.sorted) {
    if ((rc = c.ordered_cell_backward())) return rc;
    for (size_t s = 0; s < c.mp.src.size(); ++s)
      if ((rc = c.ordered_source_backward(s))) return rc;
    return IGN_OK;
  }
  if ((rc = c.sum_cell_backward())) return rc;
  if (c.mp.aggr == IGN_AGGR_ATTENTION) return c.attention_backward();
  const float* dmsgs = t->dx;   // gradient of the aggregated messages, by destination row
  if (c.mp.aggr == IGN_AGGR_CONVOLUTION && (rc = c.convolution_backward(&dmsgs))) return rc;
  return c.sum_sources_backward(dmsgs);
}

}  // namespace ign
