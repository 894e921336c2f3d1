// mp_step.cpp — one MP instance forward (mp_step.h): message networks, the ordered update's projected
// table, the kernels' argument blocks and variants, launched in one order for inference and training.

#include "mp_step.h"

#include "dense_stack.h"
#include "train_kernels.h"

namespace ign {

// timed launches record event pairs into a ring on the plan; they are resolved lazily
constexpr int kMaxPendingEvents = 1 << 14;

void Timer::begin(int kind, double flops, double bytes, double mfma_bf16, double mfma_f32) {
  on = p && p->timing && ((p->timing_kinds >> kind) & 1u);
  if (!on) return;
  if (p->ev_slot >= kMaxPendingEvents) flush_timing(p);
  const int slot = p->ev_slot;
  size_t need = 2 * (slot + 1);
  while (p->ev.size() < need) {
    hipEvent_t e;
    hipEventCreate(&e);
    p->ev.push_back(e);
  }
  if ((int)p->ev_kind.size() <= slot) {
    p->ev_kind.resize(slot + 1);
    p->ev_cost.resize(slot + 1);
  }
  p->ev_kind[slot] = kind;
  p->ev_cost[slot] = EvCost{flops, bytes, mfma_bf16, mfma_f32};
  hipEventRecord(p->ev[2 * slot], p->stream);
}

void Timer::end() {
  if (!on) return;
  hipEventRecord(p->ev[2 * p->ev_slot + 1], p->stream);
  ++p->ev_slot;
}

int mp_message_nets(ign_plan* p, const MPP& mp, const MPB& mb, const float** src, const float* hin, hipStream_t st) {
  for (int s = 0; s < (int)mp.src.size(); ++s) {
    const MsgNN& nn = mp.nn[s];
    if (nn.layers.empty()) continue;
    MsgGatherArgs g{};   // per-edge [inputs...], then the Dense stack into d_msg_layer[s]
    g.out = mb.d_msg_in[s];
    g.n = mb.n_edges[s];
    g.ld = nn.din_pad;
    g.nparts = (int)nn.inputs.size();
    int col = 0;
    for (int q = 0; q < g.nparts; ++q) {
      const int kind = nn.inputs[q];
      g.col[q] = col;
      g.width[q] = nn.widths[q];
      if (kind == IGN_MSG_HS_SOURCE) { g.base[q] = src[s]; g.rows[q] = mb.d_edge_src[s]; }
      else if (kind == IGN_MSG_HS_DEST) { g.base[q] = hin; g.rows[q] = mb.d_edge_dst[s]; }
      else { g.base[q] = mb.d_edge_params[s]; g.rows[q] = nullptr; }
      col += g.width[q];
    }
    HIP_TRY(launch_msg_gather(g, st));
    if (int rc = dense_stack_forward(p, {nn.layers.data(), (int)nn.layers.size(), mb.n_edges[s], mb.d_msg_in[s], nn.din_pad,
                                         mb.d_msg_layer[s].data(), mb.d_msg_layer[s].back()}, st))
      return rc;
    src[s] = mb.d_msg_layer[s].back();
  }
  return IGN_OK;
}

int mp_project(ign_plan* p, const MPP& mp, const MPB& mb, const float* const* src, int projected, Timer& tm) {
  const CellP& cp = p->cells[mp.cell];
  const int W3 = 3 * cp.H;
  for (size_t s = 0; s < mp.src.size(); ++s) {
    if (projected >> s & 1) continue;
    const int64_t rs = mb.src_rows[s];
    const int sdin = mp.feature_concat ? p->ents[mp.src[s].entity].hidden_dim : mp.din;
    const float* wp = p->d_packed + (mp.feature_concat ? mp.pk_slice[s] : cp.pk_w);
    tm.begin(K_PROJECT, 2.0 * rs * mp.din * W3, (double)rs * (4.0 * mp.din + 4.0 * W3), 0,
             (double)((rs + 15) / 16) * 3 * (cp.H / 16) * (sdin / 4) * kMfmaF32Flops);
    HIP_TRY(launch_project(src[s], rs, wp, p->d_packed + cp.pk_b, mb.d_table + mb.src_off[s] * W3,
                           s == 0 ? mb.d_table + mb.zero_row * W3 : nullptr, sdin, cp.H, p->stream));
    tm.end();
  }
  if (mb.n_multi) {
    tm.begin(K_OTHER, 0, 0);
    HIP_TRY(launch_multi_sum(mb.d_table, mb.zero_row + 1, mb.n_multi, mb.d_multi_ptr, mb.d_multi_rows, W3,
                             mb.d_table + mb.zero_row * W3, p->stream));
    tm.end();
  }
  return IGN_OK;
}

// Attention weights of one MP instance (AUX:287-343): per-row scores s_src = h_src (K1 a1),
// s_dst = h_dst (K2 a2), then the axis-0 softmax over (graph, position) cells into mb.d_msg_w.
int attention_weights(ign_plan* p, ign_batch* b, const MPP& mp, const MPB& mb, const float* const* srcs,
                      const float* hin, hipStream_t st) {
  const CellP& cp = p->cells[mp.cell];
  const float* w12 = p->d_packed + p->pk_w12;
  for (size_t s = 0; s < mp.src.size(); ++s) {
    const int se = mp.src[s].entity;
    const int64_t rows_s = mp.nn[s].layers.empty() ? b->rows[se] + b->halo[se] : mb.n_edges[s];
    HIP_TRY(launch_dense_fwd(srcs[s], rows_s, mp.din, mp.din, nullptr, w12, nullptr, 1, IGN_ACT_LINEAR, mb.d_s_src[s],
                             st));
  }
  HIP_TRY(launch_dense_fwd(hin, mb.n_dst, cp.H, cp.H, nullptr, w12 + p->attn_F, nullptr, 1, IGN_ACT_LINEAR, mb.d_s_dst,
                           st));
  AttnArgs aa{mb.d_group_ptr, mb.d_group_empty, mb.d_cell_dst, mb.d_cell_ptr, mb.d_cell_msgs, mb.d_msg_src,
              {mb.d_s_src[0], mb.d_s_src[1], mb.d_s_src[2], mb.d_s_src[3]}, mb.d_s_dst, mb.d_ecell, mb.d_msg_w,
              mb.n_groups};
  HIP_TRY(launch_attn_softmax(aa, st));
  return IGN_OK;
}

// The ordered MP whose input projection sum MP mi can produce in its epilogue (sum_gru_g32), or -1,
// and in *slot the source of that MP whose table rows it fills: the next MP (cyclically, within this
// forward) that touches mi's destination entity reads it as exactly one of its sources, with the
// projection sum_gru_g32 forms (32 -> 3 x 32, no message network, no feature concat), and every row
// of the entity is one of mi's destinations (no halo rows).  A multi-source reader (Q-size's
// {link, node} -> path interleave) gets each source's rows from the sum update of that source.
static int fused_proj_target(const ign_plan* p, const ign_batch* b, int mi, int* slot) {
  const MPP& mp = p->mps[mi];
  const int e = mp.dst, n = (int)p->mps.size();
  if (mp.sorted || mp.aggr != IGN_AGGR_SUM || mp.feature_concat || mp.din != 32 || p->cells[mp.cell].H != 32 ||
      b->halo[e] > 0)
    return -1;
  for (const MsgNN& nn : mp.nn)
    if (!nn.layers.empty()) return -1;
  for (int k = 1; k <= n; ++k) {
    const int m2 = (mi + k) % n;
    if (m2 <= mi && b->fuse_last_iter) return -1;   // the next reader runs in no later iteration
    const MPP& q = p->mps[m2];
    int reads = 0, s_e = -1;
    for (size_t s = 0; s < q.src.size(); ++s)
      if (q.src[s].entity == e) {
        ++reads;
        s_e = (int)s;
      }
    if (!reads && q.dst != e) continue;
    const CellP& qc = p->cells[q.cell];
    if (m2 == mi || reads != 1 || !q.sorted || q.src.size() > 8 || q.feature_concat || !q.nn[s_e].layers.empty() ||
        q.din != 32 || qc.H != 32 || qc.pk_wbf < 0)
      return -1;
    *slot = s_e;
    return m2;
  }
  return -1;
}

int mp_forward(ign_plan* p, ign_batch* b, int mi, int part, MpStates s, const MpSave& save, Timer& tm) {
  hipStream_t st = p->stream;
  const MPP& mp = p->mps[mi];
  const MPB& mb = b->mp[mi];
  const CellP& cp = p->cells[mp.cell];
  const bool saving = save.any();
  // (b->fuse_ok: forward_body's fused projection; it and the parts are inference's alone)
  const bool fusing = b->fuse_ok && !saving;
  int rc;
  for (const MsgNN& nn : mp.nn)   // the per-edge network reads halo rows: it must run after the exchange, not beside it
    if (!nn.layers.empty() && part != IGN_PART_ALL)
      return fail(IGN_ERR_UNSUPPORTED, "interior/boundary split with a message network");
  if ((rc = mp_message_nets(p, mp, mb, s.src.base, s.hin, st))) return rc;
  if (mp.sorted) {
    if (part != IGN_PART_ALL) return fail(IGN_ERR_UNSUPPORTED, "interior/boundary split is for sum MPs only");
    // sources whose table rows the previous sum updates' epilogues already formed (bit s)
    int projected = 0;
    if (fusing) {
      projected = b->proj_ready[mi];
      b->proj_ready[mi] = 0;
    }
    if ((rc = mp_project(p, mp, mb, s.src.base, projected, tm))) return rc;
    SeqGruArgs a{s.hin, s.hout, mb.d_table, mb.d_order, mb.d_len, mb.d_step_ptr, mb.d_step_code,
                 p->d_packed + cp.pk_u, p->d_packed + cp.pk_b, mb.n_dst, p->xcd_remap};
    a.hs_save = save.hs;
    if (cp.pk_ubf >= 0) a.Ubf = p->d_packed + cp.pk_ubf;
    if (cp.pk_uh >= 0) a.Uh = p->d_packed + cp.pk_uh;
    a.hdr = mb.d_seq_hdr;
    if (!cp.is_default()) {   // a cell with options: seq_gru_cell (f32 MFMA; reset_after false: a second K = H sweep)
      tm.begin(K_SEQ, mb.flops, mb.bytes, 0,
               (double)mb.wave_steps * 3 * (cp.H / 16) * (cp.H / 4) * kMfmaF32Flops);
      HIP_TRY(launch_seq_gru_cell(a, cp.H, cell_opt(cp), st));
      tm.end();
      return IGN_OK;
    }
    const int v = saving ? train_seq_variant(p, cp.H) : p->seq_variant;
    {   // MFMAs per wave step: split-fp16 / split-bf16 (variants 6, 7 / 4, 5; H = 32 / 64) passes x
        // 3 gates x H/16 x H/32 on the 16x16x32 pipe; f32 (seq_gru2) 3 gates x H/16 x H/4
      const int passes = v == 6 ? 3 : 6;
      const bool bf = v >= 4 && (cp.H == 32 || cp.H == 64) && a.Ubf;
      const double ws = (double)mb.wave_steps;
      tm.begin(K_SEQ, mb.flops, mb.bytes,
               bf ? ws * passes * 3 * (cp.H / 16) * (cp.H / 32) * kMfmaBf16Flops : 0,
               bf ? 0 : ws * 3 * (cp.H / 16) * (cp.H / 4) * kMfmaF32Flops);
    }
    HIP_TRY(launch_seq_gru(a, cp.H, v, st));
    tm.end();
    return IGN_OK;
  }
  // destinations [first, first + count) of the order array
  const int64_t first = part == IGN_PART_BOUNDARY ? mb.n_interior : 0;
  const int64_t count = part == IGN_PART_INTERIOR ? mb.n_interior
                      : part == IGN_PART_BOUNDARY ? mb.n_dst - mb.n_interior : mb.n_dst;
  if (mp.aggr == IGN_AGGR_ATTENTION) {   // AUX:287-343: scores, then the axis-0 softmax weights
    // a softmax group spans interior and boundary destinations: no split
    if (part != IGN_PART_ALL) return fail(IGN_ERR_UNSUPPORTED, "interior/boundary split with attention");
    tm.begin(K_OTHER, 0, 0);
    if ((rc = attention_weights(p, b, mp, mb, s.src.base, s.hin, st))) return rc;
    tm.end();
  }
  if (count <= 0) return IGN_OK;
  // windowed or segmented aggregation (sum MPs over all destinations): the sum kernel writes x,
  // then the GRU step reads it through an identity CSR (one message per destination: x itself)
  // (the training forward of a plan of default cells sums in the lane walk; a plan with a cell with
  // options, for all its sum MPs, default cells' included, keeps one summation order for both forwards,
  // so its training forward gives the inference forward's bits: DESIGN.md 3g)
  const bool pre = (mb.n_win_wg > 0 || mb.sum_seg) && part == IGN_PART_ALL && mp.aggr == IGN_AGGR_SUM &&
                   (!saving || p->any_cell_options);
  SrcBases xb = mb.sum_seg ? s.src : SrcBases{};   // windowed: every x from the xsum table (slot 0);
  xb.base[mb.sum_seg ? 1 : 0] = mb.d_xsum;          // segmented: the mixed CSR's slot 1
  SumGruArgs a{s.hin, s.hout, pre ? xb : s.src, pre ? mb.d_order : mb.d_order + first,
               pre ? mb.d_id_ptr : mb.d_msg_ptr + first, pre ? mb.d_id_src : mb.d_msg_src,
               p->d_packed + cp.pk_w, p->d_packed + cp.pk_u, p->d_packed + cp.pk_b, count, p->xcd_remap};
  a.x_save = save.x;
  a.sum_save = save.sum;
  if (mp.aggr == IGN_AGGR_ATTENTION) a.msg_w = mb.d_msg_w;
  if (mp.aggr == IGN_AGGR_CONVOLUTION) {   // AUX:384-401
    a.conv_kp = p->d_packed + p->pk_conv;
    a.conv_act = mp.act;
  }
  // The sum variant (launch_sum_gru): IGN_SUM_VARIANT up to 7, the split-bf16 step where a plain sum's
  // fragments exist (DIN = H = 32 or 64), else the f32 kernels, which read no fragment; 8, split-fp16
  // (DIN = H = 64), only when nothing is saved: sum_gru_h16 has no x_save.
  int sv = std::min(p->sum_variant, 7);
  if (mp.aggr == IGN_AGGR_SUM && cp.pk_wbf >= 0 && cp.pk_ubf >= 0 && mp.din == cp.din && !mp.feature_concat) {
    a.Wbf = p->d_packed + cp.pk_wbf;
    a.Ubf = p->d_packed + cp.pk_ubf;
    if (p->sum_variant == 8 && cp.pk_wh >= 0 && cp.pk_uh >= 0 && !saving) {
      a.Wbf = p->d_packed + cp.pk_wh;
      a.Ubf = p->d_packed + cp.pk_uh;
      sv = 8;
    }
  }
  // the next ordered MP's input projection in the epilogue (sum_gru_g32 only)
  int target = -1, tslot = 0;
  if (fusing && part == IGN_PART_ALL && sv == 7 && a.Wbf && a.Ubf && mp.aggr == IGN_AGGR_SUM && count == mb.n_dst &&
      mb.n_dst == b->rows[mp.dst])
    target = fused_proj_target(p, b, mi, &tslot);
  if (target >= 0) {
    const CellP& tc = p->cells[p->mps[target].cell];
    a.proj_out = b->mp[target].d_table + b->mp[target].src_off[tslot] * 3 * tc.H;
    a.proj_W = p->d_packed + tc.pk_wbf;
    a.proj_b = p->d_packed + tc.pk_b;
    a.proj_bias_row = b->mp[target].d_table + b->mp[target].zero_row * 3 * tc.H;
  }
  const double frac = mb.n_dst ? (double)count / mb.n_dst : 0.0;
  // split GRU step (sum_gru_g32 / sum_gru_bf: x6 of x.W and h.U per 16-row tile, sum_gru_h16: x3) or f32
  // MFMA (sum_gru_kernel / sum_gru_lds: 3 gates x H/16 unit tiles x (DIN + H)/4 k-steps per tile)
  const bool bf = sv >= 7 && a.Wbf && a.Ubf && mp.din == cp.H && (cp.H == 32 || cp.H == 64);
  const double tiles = (double)((count + 15) / 16);
  tm.begin(K_SUM, mb.flops * frac, mb.bytes * frac,
           bf ? tiles * (sv == 8 ? 3 : 6) * 3 * (cp.H / 16) * (mp.din / 32 + cp.H / 32) * kMfmaBf16Flops : 0,
           bf ? 0 : tiles * 3 * (cp.H / 16) * ((mp.din + cp.H) / 4) * kMfmaF32Flops);
  if (pre && mb.sum_seg) {
    SumSegArgs sa{s.src.base[0], mb.d_order, mb.d_msg_ptr, mb.d_msg_src, mb.d_xsum, mb.n_seg};
    HIP_TRY(launch_sum_seg(sa, mp.din, st));
  } else if (pre) {
    SumWinArgs wa{s.src.base[0], mb.d_win_wg, mb.d_win_dst, mb.d_win_ptr, mb.d_win_src, mb.d_xsum, mb.n_win_wg};
    HIP_TRY(launch_sum_win(wa, mp.din, st));
  }
  // a cell with options has no split pieces (Wbf / Ubf unset above, no projection target): sum_gru_cell
  if (cp.is_default()) HIP_TRY(launch_sum_gru(a, mp.din, cp.H, sv, st));
  else HIP_TRY(launch_sum_gru_cell(a, mp.din, cp.H, cell_opt(cp), st));
  tm.end();
  if (target >= 0) b->proj_ready[target] |= (char)(1 << tslot);
  return IGN_OK;
}

}  // namespace ign
