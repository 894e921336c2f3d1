// plan_lower.cpp — ign_plan_create's lowering (plan_lower.h): validation of the description into
// entities / cells / MPs / message networks (lower_mps) and the readout program (lower_readout), the
// raw parameter layout (layout_params), and the packed-fragment layout with its pack list
// (layout_packed).  No HIP, no environment: the switches arrive as a PlanSwitches.
#include "plan_lower.h"

#include <climits>

#include "dropout_rng.h"

namespace ign {

namespace {

int64_t align64(int64_t x) { return (x + 63) & ~int64_t(63); }   // tensors and slots start 256-B aligned

int lower_mps(const ign_plan_desc* d, PlanModel* p) {
  if (d->num_iterations <= 0) return fail(IGN_ERR_INVALID, "num_iterations must be > 0");
  if (d->num_entities <= 0 || d->num_entities > 8) return fail(IGN_ERR_INVALID, "1..8 entities supported");
  p->T = d->num_iterations;
  p->ents.assign(d->entities, d->entities + d->num_entities);
  for (size_t e = 0; e < p->ents.size(); ++e) {
    const auto& en = p->ents[e];
    if (en.hidden_dim <= 0) return fail(IGN_ERR_INVALID, "entity %zu: hidden_state_dimension must be > 0", e);
    if (en.feature_total > en.hidden_dim)   // AUX:155-159: zeros(H - total) needs total <= H
      return fail(IGN_ERR_INVALID, "entity %zu: total feature size %d exceeds hidden_state_dimension %d", e,
                  en.feature_total, en.hidden_dim);
  }
  p->n_adj = d->num_adjacencies;
  p->n_il = d->num_interleave;
  for (int c = 0; c < d->num_cells; ++c) {
    CellP cp;
    cp.din = d->cells[c].input_dim;
    cp.H = d->cells[c].units;
    p->cells.push_back(cp);
  }
  for (int m = 0; m < d->num_mps; ++m) {
    const ign_mp_desc& md = d->mps[m];
    MPP mp;
    mp.dst = md.dst_entity;
    mp.aggr = md.aggregation;
    mp.concat_axis = md.concat_axis;
    mp.cell = md.cell;
    if (mp.dst < 0 || mp.dst >= d->num_entities) return fail(IGN_ERR_INVALID, "mp %d: bad destination", m);
    if (md.num_sources <= 0) return fail(IGN_ERR_INVALID, "mp %d: no source entities", m);
    if (md.num_sources > IGN_MAX_SLOTS)
      return fail(IGN_ERR_UNSUPPORTED, "mp %d: more than %d source entities", m, IGN_MAX_SLOTS);
    mp.src.assign(md.sources, md.sources + md.num_sources);
    switch (mp.aggr) {
      case IGN_AGGR_SUM: mp.sorted = false; break;
      case IGN_AGGR_ORDERED: mp.sorted = true; break;
      case IGN_AGGR_INTERLEAVE:
        mp.sorted = true;
        if (md.num_sources != 2)  // tf.stack of the index lists (GM:518) needs exactly two sources
          return fail(IGN_ERR_UNSUPPORTED, "mp %d: interleave aggregation supports exactly 2 sources (GM:518)", m);
        break;
      case IGN_AGGR_CONCAT:
        if (mp.concat_axis != 1 && mp.concat_axis != 2)
          return fail(IGN_ERR_INVALID, "mp %d: concat_axis must be 1 or 2", m);
        mp.sorted = true;
        mp.feature_concat = mp.concat_axis == 2;
        break;
      case IGN_AGGR_ATTENTION:
      case IGN_AGGR_CONVOLUTION:
        mp.sorted = false;
        mp.act = md.activation;
        if (mp.aggr == IGN_AGGR_CONVOLUTION && !act_ok(mp.act, ACT_AT_CONVOLUTION))
          return fail(IGN_ERR_UNSUPPORTED, "mp %d: convolution activation %d", m, mp.act);
        break;
      default:
        return fail(IGN_ERR_UNSUPPORTED, "mp %d: aggregation %d is not lowered", m, mp.aggr);
    }
    int din = -1;
    for (auto& s : mp.src) {
      if (s.entity < 0 || s.entity >= d->num_entities) return fail(IGN_ERR_INVALID, "mp %d: bad source entity", m);
      if (s.adjacency < 0 || s.adjacency >= p->n_adj) return fail(IGN_ERR_INVALID, "mp %d: bad adjacency slot", m);
      if (mp.aggr == IGN_AGGR_INTERLEAVE && (s.interleave < 0 || s.interleave >= p->n_il))
        return fail(IGN_ERR_INVALID, "mp %d: interleave slot missing", m);
      int dm = p->ents[s.entity].hidden_dim;   // direct_assignation: message = source state
      MsgNN nn;
      if (s.msg_num_layers > 0) {               // message-creation network (GM:440-475)
        nn.param_dim = s.msg_param_dim;
        for (int q = 0; q < s.msg_num_inputs; ++q) {
          const int kind = s.msg_inputs[q];
          nn.inputs.push_back(kind);
          int w = 0;
          if (kind == IGN_MSG_HS_SOURCE) w = p->ents[s.entity].hidden_dim;
          else if (kind == IGN_MSG_HS_DEST) w = p->ents[mp.dst].hidden_dim;
          else if (kind == IGN_MSG_EDGE_PARAMS) w = s.msg_param_dim;
          else return fail(IGN_ERR_UNSUPPORTED, "mp %d: message input %d is not lowered", m, kind);
          if (w <= 0) return fail(IGN_ERR_INVALID, "mp %d: message input %d has no width", m, kind);
          if (q >= 4) return fail(IGN_ERR_UNSUPPORTED, "mp %d: more than 4 message inputs", m);
          nn.widths.push_back(w);
          nn.din += w;
        }
        if (nn.din <= 0) return fail(IGN_ERR_INVALID, "mp %d: empty message-network input", m);
        nn.din_pad = (nn.din + 15) / 16 * 16;
        int in = nn.din;
        for (int l = 0; l < s.msg_num_layers; ++l) {
          DenseP dp;
          dp.in = in;
          dp.out = s.msg_layers[l].units;
          dp.act = s.msg_layers[l].activation;
          dp.use_bias = s.msg_layers[l].use_bias;
          dp.l2 = s.msg_layers[l].l2;   // kernel_regularizer: part of model.losses (AUX:833-834)
          if (dp.out <= 0) return fail(IGN_ERR_INVALID, "mp %d: message layer %d units", m, l);
          if (!act_ok(dp.act, ACT_AT_MESSAGE)) return fail(IGN_ERR_UNSUPPORTED, "mp %d: message layer activation %d", m, dp.act);
          nn.layers.push_back(dp);
          in = dp.out;
        }
        dm = nn.dout();
      }
      mp.nn.push_back(nn);
      if (mp.feature_concat) {                 // axis 2: the step input is the sources' concatenation
        mp.slice_off.push_back(din < 0 ? 0 : din);
        din = (din < 0 ? 0 : din) + dm;
        continue;
      }
      if (din >= 0 && dm != din)
        return fail(IGN_ERR_INVALID, "mp %d: sources have different message dimensions (%d vs %d)", m, din, dm);
      din = dm;
    }
    mp.din = din;
    if (mp.cell < 0 || mp.cell >= (int)p->cells.size()) return fail(IGN_ERR_INVALID, "mp %d: bad cell index", m);
    CellP& cp = p->cells[mp.cell];
    if (cp.H != p->ents[mp.dst].hidden_dim)
      return fail(IGN_ERR_INVALID, "mp %d: cell units %d != destination hidden dim %d", m, cp.H, p->ents[mp.dst].hidden_dim);
    if (cp.din != din)
      return fail(IGN_ERR_INVALID, "mp %d: cell input_dim %d != message dim %d", m, cp.din, din);
    if (mp.feature_concat) {   // x.W is hoisted per source slice: the shapes that matter are (slice, H)
      for (auto& s : mp.src)
        if (!gru_shape_supported(p->ents[s.entity].hidden_dim, cp.H))
          return fail(IGN_ERR_UNSUPPORTED, "mp %d: concat slice (input %d, units %d) not instantiated", m,
                      p->ents[s.entity].hidden_dim, cp.H);
    } else if (!gru_shape_supported(din, cp.H)) {
      return fail(IGN_ERR_UNSUPPORTED, "mp %d: GRU shape (input %d, units %d) not instantiated (16/32, 64/64)", m,
                  din, cp.H);
    }
    if (mp.aggr == IGN_AGGR_ATTENTION || mp.aggr == IGN_AGGR_CONVOLUTION) {
      const int F = p->ents[mp.dst].hidden_dim;
      // AUX:311-319 / GM:293-298: the messages and the destination states must have one width
      if (din != F)
        return fail(IGN_ERR_INVALID, "mp %d: %s needs message dim %d == destination dim %d", m,
                    mp.aggr == IGN_AGGR_ATTENTION ? "attention" : "convolution", din, F);
      if (F != 16 && F != 32)
        return fail(IGN_ERR_UNSUPPORTED, "mp %d: attention / convolution lowered for 16 or 32 units", m);
      int& pf = mp.aggr == IGN_AGGR_ATTENTION ? p->attn_F : p->conv_F;
      if (pf && pf != F)
        return fail(IGN_ERR_INVALID, "mp %d: the shared %s weights have width %d, this MP needs %d (GM:288-300)", m,
                    mp.aggr == IGN_AGGR_ATTENTION ? "attention" : "convolution", pf, F);
      pf = F;
    }
    cp.used = true;
    p->mps.push_back(mp);
  }
  return IGN_OK;
}

int parse_dense(const ign_dense_desc* d, int n, int in, std::vector<DenseP>& out, const char* what, int idx, int at) {
  for (int l = 0; l < n; ++l) {
    DenseP dp;
    dp.in = in;
    dp.out = d[l].units;
    dp.act = d[l].activation;
    dp.use_bias = d[l].use_bias;
    dp.l2 = d[l].l2;
    if (dp.out <= 0) return fail(IGN_ERR_INVALID, "%s %d, dense layer %d: units must be > 0", what, idx, l);
    if (!act_ok(dp.act, at)) return fail(IGN_ERR_UNSUPPORTED, "%s %d, dense layer %d: activation %d", what, idx, l, dp.act);
    out.push_back(dp);
    in = dp.out;
  }
  return IGN_OK;
}

const char* space_name(int s) { return s == RS_ENTITY ? "entity" : s == RS_GRAPH ? "graph" : "adjacency"; }

// the readout program and predict (GM:605-629): parse, row spaces, widths
int lower_readout(const ign_plan_desc* d, PlanModel* p) {
  const int NE = (int)p->ents.size();
  p->adj_src_ent.assign(p->n_adj, -1);
  p->adj_dst_ent.assign(p->n_adj, -1);
  for (const MPP& mp : p->mps)
    for (const auto& s : mp.src) {
      p->adj_src_ent[s.adjacency] = s.entity;
      p->adj_dst_ent[s.adjacency] = mp.dst;
    }
  for (int e = 0; e < NE; ++e) p->ro_t.push_back({RS_ENTITY, e, p->ents[e].hidden_dim});
  if (d->num_readout_ops < 0 || (d->num_readout_ops > 0 && !d->readout_ops))
    return fail(IGN_ERR_INVALID, "bad readout operation list");
  for (int k = 0; k < d->num_readout_ops; ++k) {
    const ign_readout_op_desc& od = d->readout_ops[k];
    RoOp op;
    op.type = od.type;
    op.mode = od.mode;
    op.adj = od.adjacency;
    if (od.num_inputs <= 0 || !od.inputs) return fail(IGN_ERR_INVALID, "readout op %d: no input", k);
    for (int i = 0; i < od.num_inputs; ++i) {
      const int id = od.inputs[i];
      if (id < 0 || id >= (int)p->ro_t.size()) return fail(IGN_ERR_INVALID, "readout op %d: input tensor %d", k, id);
      op.in.push_back(id);
    }
    const RoTensor t0 = p->ro_t[op.in[0]];   // copies: ro_t grows below
    op.out = (int)p->ro_t.size();
    int rc;
    switch (op.type) {
      case IGN_RO_NEURAL_NETWORK: {
        for (int id : op.in) {
          if (!p->ro_t[id].same_space(t0))
            return fail(IGN_ERR_UNSUPPORTED, "readout op %d: inputs on different row spaces (concat axis 1)", k);
          op.in_width += p->ro_t[id].width;
        }
        if (od.num_dense <= 0 || !od.dense) return fail(IGN_ERR_INVALID, "readout op %d: no Dense layer", k);
        if ((rc = parse_dense(od.dense, od.num_dense, op.in_width, op.layers, "readout op", k, ACT_AT_READOUT_OP))) return rc;
        for (int l = 0; l < od.num_dense; ++l) op.seq.push_back({SL_DENSE, l});
        p->ro_t.push_back({t0.space, t0.sid, op.layers.back().out});
        break;
      }
      case IGN_RO_POOLING:   // Pooling_operation reads input[0] only (GM:634)
        if (op.mode < IGN_POOL_SUM || op.mode > IGN_POOL_MAX)
          return fail(IGN_ERR_INVALID, "readout op %d: pooling type %d", k, op.mode);
        p->ro_t.push_back({RS_GRAPH, 0, t0.width});
        break;
      case IGN_RO_PRODUCT: {  // input[0] * input[1] (GM:641-642)
        if (op.mode != 0)
          return fail(IGN_ERR_UNSUPPORTED, "readout op %d: dot_product (tf.tensordot axes=0) is a rank-4 outer "
                      "product the reference records as width 1 (GM:374-375); only element_wise is lowered", k);
        if (op.in.size() < 2) return fail(IGN_ERR_INVALID, "readout op %d: product needs two inputs", k);
        const RoTensor t1 = p->ro_t[op.in[1]];
        if (t1.width != t0.width && t1.width != 1)
          return fail(t0.width == 1 ? IGN_ERR_UNSUPPORTED : IGN_ERR_INVALID,
                      "readout op %d: product of widths %d and %d (the result keeps input 0's width, GM:372-373)",
                      k, t0.width, t1.width);
        RoTensor o = t0;
        if (!t0.same_space(t1)) {
          if (t0.space == RS_GRAPH) o = {t1.space, t1.sid, t0.width};
          else if (t1.space != RS_GRAPH)
            return fail(IGN_ERR_UNSUPPORTED, "readout op %d: product of tensors on different row spaces (%s %d, %s %d)",
                        k, space_name(t0.space), t0.sid, space_name(t1.space), t1.sid);
        }
        p->ro_t.push_back(o);
        break;
      }
      case IGN_RO_EXTEND: {
        if (op.in.size() < 2) return fail(IGN_ERR_INVALID, "readout op %d: extend_adjacencies needs two inputs", k);
        if (op.adj < 0 || op.adj >= p->n_adj || p->adj_src_ent[op.adj] < 0)
          return fail(IGN_ERR_INVALID, "readout op %d: adjacency slot %d is not read by any message passing", k, op.adj);
        const RoTensor t1 = p->ro_t[op.in[1]];
        if (t0.space != RS_ENTITY || t0.sid != p->adj_src_ent[op.adj] || t1.space != RS_ENTITY ||
            t1.sid != p->adj_dst_ent[op.adj])
          return fail(IGN_ERR_INVALID, "readout op %d: extend_adjacencies inputs must live on the adjacency's source "
                      "and destination entities", k);
        p->ro_t.push_back({RS_ADJ, op.adj, t0.width});
        p->ro_t.push_back({RS_ADJ, op.adj, t1.width});
        break;
      }
      default:
        return fail(IGN_ERR_UNSUPPORTED, "readout op %d: type %d", k, op.type);
    }
    p->ro_ops.push_back(std::move(op));
  }

  // predict (GM:612-629)
  p->ro_in.assign(d->readout_inputs, d->readout_inputs + d->num_readout_inputs);
  if (p->ro_in.empty()) return fail(IGN_ERR_INVALID, "readout has no input");
  int width = 0;
  for (int id : p->ro_in) {
    if (id < 0 || id >= (int)p->ro_t.size()) return fail(IGN_ERR_INVALID, "readout input tensor %d", id);
    if (!p->ro_t[id].same_space(p->ro_t[p->ro_in[0]]))
      return fail(IGN_ERR_UNSUPPORTED, "predict inputs on different row spaces (concat axis 1)");
    width += p->ro_t[id].width;
  }
  p->ro_width = width;
  int rc = parse_dense(d->dense, d->num_dense, width, p->dense, "predict", 0, ACT_AT_PREDICT);
  if (rc) return rc;
  if (p->dense.empty()) return fail(IGN_ERR_INVALID, "readout has no Dense layer");
  for (int l = 0; l < d->num_dense; ++l) p->seq.push_back({SL_DENSE, l});
  p->fused_readout = p->dense.size() == 3 &&
                     readout3_supported(width, p->dense[0].out, p->dense[1].out, p->dense[0].act, p->dense[1].act,
                                        p->dense[2].act) &&
                     p->dense[2].out == 1 && p->dense[0].use_bias && p->dense[1].use_bias;
  return IGN_OK;
}

// The raw parameter tensors, in the order of the ABI's tensor list: cells, message networks,
// convolution, attention, readout ops, predict.
void layout_params(PlanModel* p) {
  int64_t off = 0;
  p->tensors.clear();
  auto put = [&](int kind, int owner, int rows, int cols) {
    const int64_t at = off;
    p->tensors.push_back({kind, owner, at, rows, cols});
    off = align64(off + (int64_t)rows * cols);
    return at;
  };
  // use_bias false: Keras' Dense owns no bias variable, so the layout has none either
  auto put_dense = [&](DenseP& dp, int kind_w, int kind_b, int owner) {
    dp.off_w = put(kind_w, owner, dp.in, dp.out);
    dp.off_b = dp.use_bias ? put(kind_b, owner, 1, dp.out) : -1;
  };
  for (size_t c = 0; c < p->cells.size(); ++c) {
    CellP& cp = p->cells[c];
    cp.off_k = put(0, (int)c, cp.din, 3 * cp.H);
    cp.off_rk = put(1, (int)c, cp.H, 3 * cp.H);
    // Keras' GRUCell: bias [2][3H]; reset_after false, [3H]; use_bias false, no variable
    cp.off_b = cp.bias_rows() ? put(2, (int)c, cp.bias_rows(), 3 * cp.H) : -1;
  }
  for (size_t mi = 0; mi < p->mps.size(); ++mi)
    for (size_t s = 0; s < p->mps[mi].nn.size(); ++s)
      for (auto& dp : p->mps[mi].nn[s].layers) put_dense(dp, 9, 10, (int)(mi * IGN_MAX_SLOTS + s));
  if (p->conv_F) p->off_conv = put(5, -1, p->conv_F, p->conv_F);
  if (p->attn_F) {
    const int F = p->attn_F;
    p->off_k1 = put(6, -1, F, F);
    p->off_k2 = put(7, -1, F, F);
    p->off_att = put(8, -1, 2 * F, 1);
  }
  // a stack's LayerNormalization tensors stand where Keras creates them: in front of the Dense
  // layer they precede (after the last one: at the stack's end), gamma then beta; owner = the site
  auto put_stack = [&](std::vector<DenseP>& layers, const std::vector<StackLayer>& seq, int kind_w, int kind_b, int owner) {
    for (const StackLayer& e : seq) {
      if (e.kind == SL_DENSE) put_dense(layers[e.idx], kind_w, kind_b, owner + e.idx);
      if (e.kind != SL_LAYERNORM) continue;
      NormSite& ns = p->norms[e.idx];
      ns.off_gamma = ns.scale ? put(13, e.idx, 1, ns.units) : -1;
      ns.off_beta = ns.center ? put(14, e.idx, 1, ns.units) : -1;
    }
  };
  for (size_t k = 0; k < p->ro_ops.size(); ++k) put_stack(p->ro_ops[k].layers, p->ro_ops[k].seq, 11, 12, (int)(k * 64));
  put_stack(p->dense, p->seq, 3, 4, 0);
  p->n_params = off;
}

// The slots of d_packed, assigned in the order below, and PlanModel::packs: one record per slot,
// stated where the slot is assigned, in the order ign::repack launches them (`at`: cells with all
// their fragments, concat slices, message networks, convolution, attention, the fused readout's
// fp16 blocks, predict's layers, predict's W^T, readout ops).
void layout_packed(PlanModel* p) {
  enum { AT_CELL, AT_SLICE, AT_MSG, AT_CONV, AT_ATTN, AT_RO_H16, AT_DENSE, AT_DENSE_WT, AT_RO_OPS };
  std::vector<std::pair<int64_t, PackJob>> jobs;
  int64_t pk = 0;
  // from clean slots: every pk_* offset below is assigned here or stays unset (the layouts run again
  // when ign_plan_add_layernorm changes the stacks)
  p->packs.clear();
  p->any_cell_options = false;
  for (const CellP& c : p->cells) p->any_cell_options = p->any_cell_options || !c.is_default();
  for (CellP& c : p->cells) {   // (a fresh struct carries every slot's default)
    CellP z{c.din, c.H, c.off_k, c.off_rk, c.off_b, -1, -1, -1};
    z.used = c.used;
    z.act = c.act;
    z.ract = c.ract;
    z.use_bias = c.use_bias;
    z.reset_after = c.reset_after;
    c = z;
  }
  auto unpacked = [](DenseP& d) {
    DenseP z{d.in, d.out, d.act, d.use_bias, d.l2};
    z.off_w = d.off_w;
    z.off_b = d.off_b;
    d = z;
  };
  for (auto& d : p->dense) unpacked(d);
  for (auto& op : p->ro_ops)
    for (auto& d : op.layers) unpacked(d);
  for (auto& mp : p->mps) {
    mp.pk_slice.clear();
    for (auto& nn : mp.nn)
      for (auto& d : nn.layers) unpacked(d);
  }
  // reserves `floats` and records the launch that fills them; (at, idx, sub) orders the launches
  auto slot = [&](int at, size_t idx, int sub, int kind, int64_t floats, int64_t s0, int64_t s1, int64_t s2, int a,
                  int b = 0, int c = 0) {
    const int64_t dst = pk;
    jobs.push_back({((int64_t)at << 40) | ((int64_t)idx << 8) | sub, PackJob{kind, {s0, s1, s2}, dst, a, b, c, floats}});
    pk = align64(pk + floats);
    return dst;
  };
  for (size_t c = 0; c < p->cells.size(); ++c) {
    CellP& cp = p->cells[c];
    if (!cp.used) continue;
    const int din = cp.din, H = cp.H;
    // A cell with options (ign_plan_set_cell_options) runs on gru_cell.hip's kernels: pack_gru's unscaled
    // fragments and its bias form, and none of the split pieces below.  Their absence is what takes
    // the cell off the fast paths: the resident forward (resident_plan_shape needs pk_uh / pk_wbf /
    // pk_ubf), the split-bf16 / split-fp16 sequence and sum variants, and sum_gru_g32's fused projection
    // (its own pieces, and the target cell's pk_wbf).  mp_step.cpp and mp_backward.cpp dispatch on is_default().
    const bool dflt = cp.is_default();
    const int mode = dflt ? 0 : kPackGruRaw | cp.bias_rows();
    cp.pk_w = slot(AT_CELL, c, 0, PK_GRU, pack_gru_w_floats(din, H), cp.off_k, cp.off_rk, cp.off_b, din, H, mode);
    cp.pk_u = slot(AT_CELL, c, 1, PK_GRU_U, pack_gru_u_floats(H), -1, cp.off_rk, -1, din, H);
    cp.pk_b = slot(AT_CELL, c, 2, PK_GRU_B, pack_gru_b_floats(H), -1, -1, cp.off_b, din, H);
    if (!dflt) continue;
    if (pack_u_bf16_floats(H)) cp.pk_ubf = slot(AT_CELL, c, 3, PK_U_BF16, pack_u_bf16_floats(H), cp.off_rk, -1, -1, H);
    if (pack_u_f16_floats(H)) cp.pk_uh = slot(AT_CELL, c, 4, PK_U_F16, pack_u_f16_floats(H), cp.off_rk, -1, -1, H);
    if (din == 64 && H == 64)
      cp.pk_wh = slot(AT_CELL, c, 5, PK_W_F16, pack_w_f16_floats(din, H), cp.off_k, -1, -1, din, H);
    if ((din == 64 && H == 64) || (din == 32 && H == 32))
      cp.pk_wbf = slot(AT_CELL, c, 6, PK_W_BF16, pack_w_bf16_floats(din, H), cp.off_k, -1, -1, din, H);
  }
  for (size_t l = 0; l < p->dense.size(); ++l) {
    DenseP& dp = p->dense[l];
    const int in = dp.in, out = dp.out;
    if ((p->fused_readout && l < 2) || dense_fwd_supported(in, out))
      dp.pk_w = slot(AT_DENSE, l, 0, PK_DENSE_PAD, pack_dense_floats(in, out), dp.off_w, -1, -1, in, in, out);
    if (p->fused_readout && l < 2 && in % 32 == 0 && out % 16 == 0 &&
        readout_bf_supported(p->dense[0].in, p->dense[0].out, p->dense[1].out, p->dense[0].act, p->dense[1].act,
                             p->dense[2].act)) {
      // layer 1 reads its input from memory (natural k), layer 2 chains from registers
      dp.pk_bf = slot(AT_DENSE, l, 1, PK_DENSE_BF16, pack_dense_bf16_floats(in, out), dp.off_w, -1, -1, in, out, l != 0);
      if (l == 1) {
        const DenseP& l1 = p->dense[0];
        const int64_t n = pack_readout_h16_floats(l1.in, l1.out, out);
        dp.pk_h = slot(AT_RO_H16, 0, 0, PK_READOUT_H16, n, l1.off_w, l1.off_b, dp.off_w, l1.in, l1.out, out);
        if (p->readout_variant == 5)   // (otherwise neither packed after each optimizer step nor allocated)
          dp.pk_h32 = slot(AT_RO_H16, 0, 1, PK_READOUT_H32, n, l1.off_w, l1.off_b, dp.off_w, l1.in, l1.out, out);
      }
    }
    if (dense_bf_supported(in, out)) {
      dp.pk_bfn = slot(AT_DENSE, l, 2, PK_DENSE_BF16, pack_dense_bf16_floats(in, out), dp.off_w, -1, -1, in, out, 0);
      dp.pk_hn = slot(AT_DENSE, l, 4, PK_DENSE_F16, pack_dense_f16_floats(in, out), dp.off_w, -1, -1, in, out, 0);
    }
    if (dense_bf_supported(out, in)) {
      dp.pk_bft = slot(AT_DENSE, l, 3, PK_DENSE_BF16_T, pack_dense_bf16_floats(in, out), dp.off_w, -1, -1, in, out);
      dp.pk_ht = slot(AT_DENSE, l, 5, PK_DENSE_F16, pack_dense_f16_floats(out, in), dp.off_w, -1, -1, out, in, 1);
    }
  }
  // backward fragments (training): W^T / U^T per cell, W^T per Dense layer where the MFMA
  // row GEMM is instantiated
  for (size_t c = 0; c < p->cells.size(); ++c) {
    CellP& cp = p->cells[c];
    if (!cp.used || !bwd_shape_supported(cp.H, cp.H)) continue;   // U^T: the recurrent backward
    cp.pk_ut = slot(AT_CELL, c, 8, PK_A, pack_gru_u_floats(cp.H), cp.off_rk, -1, -1, cp.H, 3 * cp.H);
    if (pack_ut_f16_floats(cp.H) && cp.is_default())
      cp.pk_uth = slot(AT_CELL, c, 9, PK_UT_F16, pack_ut_f16_floats(cp.H), cp.off_rk, -1, -1, cp.H);
    if (!bwd_shape_supported(cp.din, cp.H)) continue;            // W^T (an axis-2 concat cell goes generic)
    cp.pk_wt = slot(AT_CELL, c, 7, PK_A, pack_gru_w_floats(cp.din, cp.H), cp.off_k, -1, -1, cp.din, 3 * cp.H);
  }
  for (size_t l = 0; l < p->dense.size(); ++l) {
    DenseP& dp = p->dense[l];
    if (!row_gemm_supported(dp.out, dp.in)) continue;
    dp.pk_wt = slot(AT_DENSE_WT, l, 0, PK_A, pack_dense_floats(dp.in, dp.out), dp.off_w, -1, -1, dp.in, dp.out);
  }
  size_t n_msg = 0;
  for (auto& mp : p->mps)
    for (auto& nn : mp.nn)
      for (size_t l = 0; l < nn.layers.size(); ++l) {
        DenseP& dp = nn.layers[l];
        const int kin = l == 0 ? nn.din_pad : dp.in;
        if (dense_fwd_supported(kin, dp.out))
          dp.pk_w = slot(AT_MSG, n_msg++, 0, PK_DENSE_PAD, pack_dense_floats(kin, dp.out), dp.off_w, -1, -1, dp.in, kin, dp.out);
      }
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {
    MPP& mp = p->mps[mi];
    if (!mp.feature_concat) continue;
    const CellP& cp = p->cells[mp.cell];
    for (size_t s = 0; s < mp.src.size(); ++s) {
      const int w = p->ents[mp.src[s].entity].hidden_dim;
      mp.pk_slice.push_back(slot(AT_SLICE, mi, (int)s, PK_GRU_W, pack_gru_w_floats(w, cp.H),
                                 cp.off_k + (int64_t)mp.slice_off[s] * 3 * cp.H, -1, -1, w, cp.H,
                                 cp.is_default() ? 0 : kPackGruRaw));
    }
  }
  if (p->conv_F)
    p->pk_conv = slot(AT_CONV, 0, 0, PK_DENSE_PAD, pack_dense_floats(p->conv_F, p->conv_F), p->off_conv, -1, -1, p->conv_F,
                      p->conv_F, p->conv_F);
  if (p->attn_F)
    p->pk_w12 = slot(AT_ATTN, 0, 0, PK_ATTN_VECTORS, attn_vectors_floats(p->attn_F), p->off_k1, p->off_k2, p->off_att, p->attn_F);
  size_t n_ro = 0;
  for (auto& op : p->ro_ops)
    for (auto& dp : op.layers)
      if (dense_fwd_supported(dp.in, dp.out))
        dp.pk_w = slot(AT_RO_OPS, n_ro++, 0, PK_DENSE_PAD, pack_dense_floats(dp.in, dp.out), dp.off_w, -1, -1, dp.in, dp.in, dp.out);
  p->n_packed = pk;
  std::stable_sort(jobs.begin(), jobs.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
  p->packs.reserve(jobs.size());
  for (auto& j : jobs) p->packs.push_back(j.second);
}

// s into its array in site order (readout ops in order, then predict; by position; then by
// insertion); the index it got
template <class Site>
int insert_site(std::vector<Site>& sites, const Site& s) {
  auto key = [](const Site& x) { return std::make_pair(x.stack < 0 ? INT_MAX : x.stack, x.before); };
  size_t at = 0;
  while (at < sites.size() && key(sites[at]) <= key(s)) ++at;
  sites.insert(sites.begin() + at, s);
  return (int)at;
}

// The one place a Dropout (d) or LayerNormalization (n) layer enters a stack: the checks of stack and
// before_layer, the kind's own check, the site array and every seq the insertion touches.
int add_site(PlanModel* p, int kind, int stack, int before_layer, DropSite d, NormSite n) {
  const char* api = kind == SL_DROPOUT ? "ign_plan_add_dropout" : "ign_plan_add_layernorm";
  const std::vector<DenseP>* layers = stack_layers(p, stack);
  if (!layers)
    return fail(IGN_ERR_INVALID, "%s: stack %d is neither -1 (predict) nor a readout neural_network operation", api, stack);
  const int L = (int)layers->size();
  if (before_layer < 0 || before_layer > L)
    return fail(IGN_ERR_INVALID, "%s: before_layer %d outside 0..%d", api, before_layer, L);
  if (kind == SL_DROPOUT) {
    if (!(d.rate >= 0.f && d.rate < 1.f))   // tf.nn.dropout raises ValueError
      return fail(IGN_ERR_INVALID, "Dropout rate must be in [0, 1), got %g", (double)d.rate);
    if (d.rate == 0.f) return IGN_OK;   // tf.nn.dropout returns x: no layer, no site
  } else if (!(n.epsilon >= 0.f)) {   // Keras raises ValueError
    return fail(IGN_ERR_INVALID, "LayerNormalization epsilon must be >= 0, got %g", (double)n.epsilon);
  }
  d.stack = n.stack = stack;
  d.before = n.before = before_layer;
  d.units = n.units = before_layer < L ? (*layers)[before_layer].in : layers->back().out;
  const int at = kind == SL_DROPOUT ? insert_site(p->drops, d) : insert_site(p->norms, n);
  auto shift = [&](std::vector<StackLayer>& seq) {   // the sites behind it moved up by one
    for (StackLayer& e : seq) e.idx += e.kind == kind && e.idx >= at;
  };
  for (RoOp& op : p->ro_ops) shift(op.seq);
  shift(p->seq);
  std::vector<StackLayer>& seq = stack == -1 ? p->seq : p->ro_ops[stack].seq;
  auto pos = seq.begin();   // in front of Dense before_layer, behind what stands there; or at the end
  while (pos != seq.end() && !(pos->kind == SL_DENSE && pos->idx == before_layer)) ++pos;
  seq.insert(pos, {kind, at});
  return IGN_OK;
}

}  // namespace

void mark_dead_last(PlanModel* p) {
  const int NE = (int)p->ents.size(), n = (int)p->mps.size();
  // the entities whose final states the readout reads: every input of every operation (whatever
  // the operation does with it) and predict's inputs; tensor ids below NE are entity states
  std::vector<char> read(NE, 0);
  for (const RoOp& op : p->ro_ops)
    for (int id : op.in)
      if (id >= 0 && id < NE) read[id] = 1;
  for (int id : p->ro_in)
    if (id >= 0 && id < NE) read[id] = 1;
  for (int mi = 0; mi < n; ++mi) {
    MPP& mp = p->mps[mi];
    bool dead = !read[mp.dst];
    for (int m2 = mi + 1; m2 < n && dead; ++m2) {
      const MPP& q = p->mps[m2];
      if (q.dst == mp.dst) dead = false;          // its previous state (and, with a message network, hs_dest)
      for (const auto& s : q.src) dead = dead && s.entity != mp.dst;
      for (const auto& s : mp.src) dead = dead && s.entity != q.dst;   // mi's input would change under it
    }
    mp.dead_in_last_iter = dead;
  }
}

int add_dropout(PlanModel* p, int stack, int before_layer, float rate, uint64_t layer_seed) {
  DropSite d;
  d.rate = rate;
  d.scale = dropout_scale(rate);
  d.seed = layer_seed;
  return add_site(p, SL_DROPOUT, stack, before_layer, d, NormSite());
}

int add_layernorm(PlanModel* p, int stack, int before_layer, float epsilon, int center, int scale) {
  NormSite n;
  n.epsilon = epsilon;
  n.center = center != 0;
  n.scale = scale != 0;
  if (int rc = add_site(p, SL_LAYERNORM, stack, before_layer, DropSite(), n)) return rc;
  if (stack == -1) p->fused_readout = false;   // the fused 256-256-1 kernel has no place for the layer
  layout_params(p);   // both layouts again
  layout_packed(p);
  return IGN_OK;
}

int set_cell_options(PlanModel* p, int cell, const ign_cell_options* o) {
  if (!o) return fail(IGN_ERR_INVALID, "ign_plan_set_cell_options: null options");
  if (cell < 0 || cell >= (int)p->cells.size())
    return fail(IGN_ERR_INVALID, "ign_plan_set_cell_options: cell %d outside 0..%d", cell, (int)p->cells.size() - 1);
  for (int a : {o->activation, o->recurrent_activation})
    if (!act_ok(a, ACT_AT_PREDICT))
      return fail(IGN_ERR_INVALID, "ign_plan_set_cell_options: activation code %d", a);
  CellP& cp = p->cells[cell];
  cp.act = o->activation;
  cp.ract = o->recurrent_activation;
  cp.use_bias = o->use_bias != 0;
  cp.reset_after = o->reset_after != 0;
  layout_params(p);   // the bias tensor's form, and both layouts after it
  layout_packed(p);
  return IGN_OK;
}

int lower_plan(const ign_plan_desc* d, const PlanSwitches& sw, PlanModel* m) {
  static_cast<PlanSwitches&>(*m) = sw;
  int rc;
  if ((rc = lower_mps(d, m)) || (rc = lower_readout(d, m))) return rc;
  // exp(z) and whatever a relu / selu / linear layer makes of it reach 2^127, beyond the 2^75 a tile of
  // dense_h16 (forward and transposed) scales into fp16 range (its exponent clamp): a plan that names
  // `exponential` anywhere runs its Dense stacks on split-bf16 (exact pieces, no scale) and f32 operands
  auto has_exp = [](const std::vector<DenseP>& layers) {
    for (const DenseP& l : layers)
      if (l.act == IGN_ACT_EXPONENTIAL) return true;
    return false;
  };
  bool any_exp = has_exp(m->dense);
  for (const RoOp& op : m->ro_ops) any_exp = any_exp || has_exp(op.layers);
  for (const MPP& mp : m->mps) {
    any_exp = any_exp || (mp.aggr == IGN_AGGR_CONVOLUTION && mp.act == IGN_ACT_EXPONENTIAL);
    for (const MsgNN& nn : mp.nn) any_exp = any_exp || has_exp(nn.layers);
  }
  if (any_exp) m->train_dense_h16 = false;
  mark_dead_last(m);
  layout_params(m);
  layout_packed(m);
  return IGN_OK;
}

}  // namespace ign
