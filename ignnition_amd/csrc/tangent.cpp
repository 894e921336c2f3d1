// tangent.cpp — ign_forward_tangent: the forward on dual numbers.  Every entity keeps
// a primal and a tangent state pair in scratch blocks of the batch's pool; the MP instances run in the
// forward's order on tangent.hip's kernels, and what is linear runs the existing launches on the
// tangent rows: init_state on the direction, project on the raw W fragments with a zero bias block,
// multi_sum, sum_seg / sum_win, and per Dense layer of predict xd.W (no bias, linear) followed by
// act_bwd's act'(y).  Nothing of the batch is written: its states, tables, predictions and captured
// graph stay as the last forward left them.

#include "mp_step.h"
#include "tangent.h"
#include "train_kernels.h"

namespace {

using namespace ign;

// scratch of one call: blocks of the batch's pool, handed back behind the plan's stream
struct Scratch {
  ign_batch* b;
  hipStream_t st;
  std::vector<void*> blocks;
  ~Scratch() {
    if (!blocks.empty()) pool_release(b->pool.get(), blocks, st);
  }
  // n floats (+ the slack dev_alloc gives: a masked-off row 0 of an empty table may be read)
  int get(float** out, int64_t n, bool zero = false) {
    void* q = nullptr;
    const size_t bytes = (size_t)(std::max<int64_t>(n, 0) + 256) * sizeof(float);
    const hipError_t e = pool_alloc(b->pool.get(), &q, bytes, false);
    if (e != hipSuccess) return fail(IGN_ERR_OOM, "forward tangent: device alloc (%zu bytes): %s", bytes, hipGetErrorString(e));
    blocks.push_back(q);
    if (zero) HIP_TRY(hipMemsetAsync(q, 0, bytes, st));
    *out = static_cast<float*>(q);
    return IGN_OK;
  }
};

int refuse(const char* what) { return fail(IGN_ERR_UNSUPPORTED, "forward tangent: %s", what); }

// what the dual kernels do not cover, by name
int check_scope(const ign_plan* p, const ign_batch* b) {
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
    if (mp.din != cp.din || !gru_cell_sum_supported(mp.din, cp.H, 0) || (mp.sorted && !gru_cell_seq_supported(cp.H)))
      return fail(IGN_ERR_UNSUPPORTED, "forward tangent: GRU shape %d / %d", mp.din, cp.H);
  }
  if (!p->ro_ops.empty()) return refuse("a readout operation before predict");
  if (!p->norms.empty()) return refuse("LayerNormalization");
  return IGN_OK;
}

struct RawCell {   // pack_gru's unscaled form of one cell, packed per call from the live parameters
  float *W = nullptr, *U = nullptr, *b = nullptr;
};

// per entity: primal and tangent ping-pong states
struct DualStates {
  std::vector<float*> h[2], hd[2];
  std::vector<int> cur;
};

int ordered_step(ign_plan* p, const MPP& mp, const MPB& mb, const RawCell& rc, const float* zero_bias, const DualStates& s,
                 float* tab, float* tabd) {
  hipStream_t st = p->stream;
  const CellP& cp = p->cells[mp.cell];
  const int W3 = 3 * cp.H;
  for (size_t k = 0; k < mp.src.size(); ++k) {
    const int se = mp.src[k].entity;
    const int64_t ofs = mb.src_off[k] * W3;
    HIP_TRY(launch_project(s.h[s.cur[se]][se], mb.src_rows[k], rc.W, rc.b, tab + ofs, k == 0 ? tab + mb.zero_row * W3 : nullptr,
                           mp.din, cp.H, st));
    HIP_TRY(launch_project(s.hd[s.cur[se]][se], mb.src_rows[k], rc.W, zero_bias, tabd + ofs,
                           k == 0 ? tabd + mb.zero_row * W3 : nullptr, mp.din, cp.H, st));
  }
  if (mb.n_multi) {
    HIP_TRY(launch_multi_sum(tab, mb.zero_row + 1, mb.n_multi, mb.d_multi_ptr, mb.d_multi_rows, W3, tab + mb.zero_row * W3, st));
    HIP_TRY(launch_multi_sum(tabd, mb.zero_row + 1, mb.n_multi, mb.d_multi_ptr, mb.d_multi_rows, W3, tabd + mb.zero_row * W3,
                             st));
  }
  const int c = s.cur[mp.dst];
  SeqTangentArgs a{};
  a.p = SeqGruArgs{s.h[c][mp.dst], s.h[1 - c][mp.dst], tab, mb.d_order, mb.d_len, mb.d_step_ptr, mb.d_step_code,
                   rc.U, rc.b, mb.n_dst, 0};
  a.hd_in = s.hd[c][mp.dst];
  a.hd_out = s.hd[1 - c][mp.dst];
  a.table_d = tabd;
  HIP_TRY(launch_seq_gru_tangent(a, cp.H, cell_opt(cp), st));
  return IGN_OK;
}

int sum_step(ign_plan* p, const MPP& mp, const MPB& mb, const RawCell& rc, const DualStates& s, float* xs, float* xsd) {
  hipStream_t st = p->stream;
  const CellP& cp = p->cells[mp.cell];
  SrcBases sp{}, sd{};
  for (size_t k = 0; k < mp.src.size(); ++k) {
    const int se = mp.src[k].entity;
    sp.base[k] = s.h[s.cur[se]][se];
    sd.base[k] = s.hd[s.cur[se]][se];
  }
  // the forward's per-destination rule: destinations of the segmented (or windowed) sum read their x
  // from the summed table through the batch's identity CSR.  Both sums are plain row sums, so the
  // tangent rows go through the same launches
  const bool pre = mb.n_win_wg > 0 || mb.sum_seg;
  if (pre && mb.sum_seg) {
    HIP_TRY(launch_sum_seg(SumSegArgs{sp.base[0], mb.d_order, mb.d_msg_ptr, mb.d_msg_src, xs, mb.n_seg}, mp.din, st));
    HIP_TRY(launch_sum_seg(SumSegArgs{sd.base[0], mb.d_order, mb.d_msg_ptr, mb.d_msg_src, xsd, mb.n_seg}, mp.din, st));
    sp.base[1] = xs;   // the mixed CSR's slot 1
    sd.base[1] = xsd;
  } else if (pre) {
    HIP_TRY(launch_sum_win(SumWinArgs{sp.base[0], mb.d_win_wg, mb.d_win_dst, mb.d_win_ptr, mb.d_win_src, xs, mb.n_win_wg},
                           mp.din, st));
    HIP_TRY(launch_sum_win(SumWinArgs{sd.base[0], mb.d_win_wg, mb.d_win_dst, mb.d_win_ptr, mb.d_win_src, xsd, mb.n_win_wg},
                           mp.din, st));
    sp = SrcBases{};
    sd = SrcBases{};
    sp.base[0] = xs;   // every x from the summed table
    sd.base[0] = xsd;
  }
  const int c = s.cur[mp.dst];
  SumTangentArgs a{};
  a.p = SumGruArgs{s.h[c][mp.dst], s.h[1 - c][mp.dst], sp, mb.d_order, pre ? mb.d_id_ptr : mb.d_msg_ptr,
                   pre ? mb.d_id_src : mb.d_msg_src, rc.W, rc.U, rc.b, mb.n_dst, 0};
  a.src_d = sd;
  a.hd_in = s.hd[c][mp.dst];
  a.hd_out = s.hd[1 - c][mp.dst];
  HIP_TRY(launch_sum_gru_tangent(a, mp.din, cp.H, cell_opt(cp), st));
  return IGN_OK;
}

// predict's Dense stack on (x, xd): y = act(x.W + b), yd = act'(y) (xd.W); a Dropout layer is the identity
int predict_dual(ign_plan* p, ign_batch* b, Scratch& sc, const float* x, const float* xd, const float** y_out,
                 const float** yd_out) {
  hipStream_t st = p->stream;
  const int64_t P = b->n_pred;
  int stride = p->ro_width, rc;
  int widest = 1;
  for (const DenseP& d : p->dense) widest = std::max(widest, d.out);
  float* lin = nullptr;
  if ((rc = sc.get(&lin, P * widest))) return rc;
  for (const DenseP& d : p->dense) {
    float *y = nullptr, *yd = nullptr;
    if ((rc = sc.get(&y, P * d.out)) || (rc = sc.get(&yd, P * d.out))) return rc;
    const int K = d.pk_w >= 0 ? stride : d.in;
    const float* Wp = d.pk_w >= 0 ? p->d_packed + d.pk_w : nullptr;
    const float* W = p->d_params + d.off_w;
    HIP_TRY(launch_dense_fwd(x, P, K, stride, Wp, W, d.use_bias ? p->d_params + d.off_b : nullptr, d.out, d.act, y, st));
    HIP_TRY(launch_dense_fwd(xd, P, K, stride, Wp, W, nullptr, d.out, IGN_ACT_LINEAR, lin, st));
    HIP_TRY(launch_act_bwd(lin, y, P * d.out, d.act, yd, st));
    x = y;
    xd = yd;
    stride = d.out;
  }
  *y_out = x;
  *yd_out = xd;
  return IGN_OK;
}

int forward_tangent(ign_plan* p, ign_batch* b, const float* const* dfeat, float* pred, float* dpred) {
  hipStream_t st = p->stream;
  const int E = (int)p->ents.size();
  Scratch sc{b, st, {}};
  int rc;
  // raw fragments of every cell an MP runs, from the parameters as they are now
  std::vector<RawCell> raw(p->cells.size());
  for (const MPP& mp : p->mps) {
    const CellP& cp = p->cells[mp.cell];
    RawCell& r = raw[mp.cell];
    if (r.W) continue;
    if ((rc = sc.get(&r.W, pack_gru_w_floats(cp.din, cp.H))) || (rc = sc.get(&r.U, pack_gru_u_floats(cp.H))) ||
        (rc = sc.get(&r.b, pack_gru_b_floats(cp.H))))
      return rc;
    HIP_TRY(launch_pack_gru(p->d_params + cp.off_k, p->d_params + cp.off_rk, cp.bias_rows() ? p->d_params + cp.off_b : nullptr,
                            r.W, r.U, r.b, cp.din, cp.H, kPackGruRaw | cp.bias_rows(), st));
  }
  float* zero_bias = nullptr;
  if ((rc = sc.get(&zero_bias, 4 * 64, true))) return rc;
  // h0 = [features | 0], h0d = [direction | 0]
  DualStates s;
  s.cur.assign(E, 0);
  for (int k = 0; k < 2; ++k) {
    s.h[k].assign(E, nullptr);
    s.hd[k].assign(E, nullptr);
  }
  for (int e = 0; e < E; ++e) {
    const int H = p->ents[e].hidden_dim, F = p->ents[e].feature_total;
    for (int k = 0; k < 2; ++k)
      if ((rc = sc.get(&s.h[k][e], b->rows[e] * H)) || (rc = sc.get(&s.hd[k][e], b->rows[e] * H))) return rc;
    const float* dir = nullptr;
    if (dfeat[e] && F > 0 && b->rows[e] > 0) {
      float* d = nullptr;
      if ((rc = sc.get(&d, b->rows[e] * F))) return rc;
      HIP_TRY(hipMemcpyAsync(d, dfeat[e], (size_t)b->rows[e] * F * sizeof(float), hipMemcpyDefault, st));
      dir = d;
    }
    HIP_TRY(launch_init_state(s.h[0][e], b->d_feat[e], b->rows[e], H, F, st));
    HIP_TRY(launch_init_state(s.hd[0][e], dir, b->rows[e], H, F, st));
  }
  // per MP: the ordered update's two projected tables, or the summed rows of a segmented / windowed sum
  std::vector<float*> t0(p->mps.size(), nullptr), t1(p->mps.size(), nullptr);
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {
    const MPP& mp = p->mps[mi];
    const MPB& mb = b->mp[mi];
    const int64_t n = mp.sorted ? (mb.zero_row + 1 + mb.n_multi) * 3LL * p->cells[mp.cell].H
                    : mb.n_win_wg > 0 || mb.sum_seg ? std::max<int64_t>(mb.n_dst, 1) * mp.din : 0;
    if (n && ((rc = sc.get(&t0[mi], n)) || (rc = sc.get(&t1[mi], n)))) return rc;
  }
  for (int it = 0; it < p->T; ++it)
    for (size_t mi = 0; mi < p->mps.size(); ++mi) {
      const MPP& mp = p->mps[mi];
      if (it + 1 == p->T && mp.dead_in_last_iter) continue;   // nothing reads this update (§3e)
      if ((rc = mp.sorted ? ordered_step(p, mp, b->mp[mi], raw[mp.cell], zero_bias, s, t0[mi], t1[mi])
                          : sum_step(p, mp, b->mp[mi], raw[mp.cell], s, t0[mi], t1[mi])))
        return rc;
      s.cur[mp.dst] ^= 1;
    }
  // predict on the final states and their tangents
  std::vector<const float*> ep(E), ed(E);
  for (int e = 0; e < E; ++e) {
    ep[e] = s.h[s.cur[e]][e];
    ed[e] = s.hd[s.cur[e]][e];
  }
  float *catp = nullptr, *catd = nullptr;
  if (p->ro_in.size() > 1 && ((rc = sc.get(&catp, b->n_pred * p->ro_width)) || (rc = sc.get(&catd, b->n_pred * p->ro_width))))
    return rc;
  const float *x = nullptr, *xd = nullptr, *y = nullptr, *yd = nullptr;
  if ((rc = predict_input(p, b, ep.data(), catp, &x, st)) || (rc = predict_input(p, b, ed.data(), catd, &xd, st)) ||
      (rc = predict_dual(p, b, sc, x, xd, &y, &yd)))
    return rc;
  const size_t bytes = (size_t)b->n_pred * b->out_units * sizeof(float);
  if (pred) HIP_TRY(hipMemcpyAsync(pred, y, bytes, hipMemcpyDefault, st));
  if (dpred) HIP_TRY(hipMemcpyAsync(dpred, yd, bytes, hipMemcpyDefault, st));
  HIP_TRY(hipStreamSynchronize(st));   // the caller's host arrays (directions in, results out) are done with
  return IGN_OK;
}

}  // namespace

extern "C" int ign_forward_tangent(ign_batch* b, const float* const* dfeat, int n_ents, float* pred, float* dpred) {
  if (!b || !dfeat) return fail(IGN_ERR_INVALID, "null argument");
  ign_plan* p = b->plan;
  int rc = check_pb(p, b);
  if (rc) return rc;
  if (n_ents != (int)p->ents.size())
    return fail(IGN_ERR_INVALID, "forward tangent: %d directions for a plan of %d entities", n_ents, (int)p->ents.size());
  if ((rc = check_scope(p, b))) return rc;
  return forward_tangent(p, b, dfeat, pred, dpred);
}
