// jacobian.cpp — ign_forward_jacobian: K feature directions through one linearised forward (DESIGN.md
// §3n).  The primal runs ONCE on ordinary rows, on jacobian.hip's linearising kernels (the tangent
// kernels' primal, so its bits), and leaves per MP the coefficient rows of that update; right behind
// each primal update the K tangents take the same update as a linear recurrence on [row][Kp][H] states
// (Kp = K rounded up to 16).  What is linear on flat rows runs the existing launches on rows * Kp rows:
// project on the raw W fragments with a zero bias block for the tangent tables, and per Dense layer of
// predict xd.W (linear, no bias).  All memory is scratch blocks of the batch's pool, handed back behind
// the plan's stream.  Nothing of the batch is written: its states, tables, feature buffer, predictions
// and captured graph stay as the last forward left them.

#include "jacobian_common.h"
#include "train_kernels.h"

namespace {

using namespace ign;

using Scratch = JacScratch;
using RawCell = JacRawCell;

struct MpScratch {
  float* tab = nullptr;    // ordered: the primal's projected table
  float* tabd = nullptr;   // ordered: the tangent table [table row][Kp][3H]
  float* coef = nullptr;   // [n_steps or n_dst][kJacCoef][H]
  float* xs = nullptr;     // sum with a segmented / windowed class: the primal's summed rows
};

struct States {   // per entity: primal [rows][H] and tangent [rows][Kp][H] ping-pong states
  std::vector<float*> h[2], hd[2];
  std::vector<int> cur;
  int64_t kp = 0;
};

int ordered_step(ign_plan* p, const MPP& mp, const MPB& mb, const RawCell& rc, const float* zero_bias, const States& s,
                 const MpScratch& m) {
  hipStream_t st = p->stream;
  const CellP& cp = p->cells[mp.cell];
  const int W3 = 3 * cp.H;
  for (size_t k = 0; k < mp.src.size(); ++k) {
    const int se = mp.src[k].entity;
    HIP_TRY(launch_project(s.h[s.cur[se]][se], mb.src_rows[k], rc.W, rc.b, m.tab + mb.src_off[k] * W3,
                           k == 0 ? m.tab + mb.zero_row * W3 : nullptr, mp.din, cp.H, st));
    HIP_TRY(launch_project(s.hd[s.cur[se]][se], mb.src_rows[k] * s.kp, rc.W, zero_bias,
                           m.tabd + scen_offset(mb.src_off[k], 0, s.kp, W3), nullptr, mp.din, cp.H, st));
  }
  if (mb.n_multi)
    HIP_TRY(launch_multi_sum(m.tab, mb.zero_row + 1, mb.n_multi, mb.d_multi_ptr, mb.d_multi_rows, W3, m.tab + mb.zero_row * W3, st));
  HIP_TRY(launch_table_rows_jac(m.tabd, mb.zero_row, mb.n_multi, mb.d_multi_ptr, mb.d_multi_rows, W3, s.kp, st));
  const int c = s.cur[mp.dst];
  const SeqGruArgs pa{s.h[c][mp.dst], s.h[1 - c][mp.dst], m.tab, mb.d_order, mb.d_len, mb.d_step_ptr, mb.d_step_code,
                      rc.U, rc.b, mb.n_dst, 0};
  HIP_TRY(launch_seq_gru_lin(pa, m.coef, cp.H, cell_opt(cp), st));
  const SeqJacArgs ja{s.hd[c][mp.dst], s.hd[1 - c][mp.dst], m.tabd, m.coef, mb.d_order, mb.d_len, mb.d_step_ptr,
                      mb.d_step_code, rc.U, mb.n_dst, (int32_t)(s.kp / 16)};
  HIP_TRY(launch_seq_gru_jac(ja, cp.H, st));
  return IGN_OK;
}

int sum_step(ign_plan* p, const MPP& mp, const MPB& mb, const RawCell& rc, const States& s, const MpScratch& m) {
  hipStream_t st = p->stream;
  const CellP& cp = p->cells[mp.cell];
  SrcBases sp{}, sd{};
  for (size_t k = 0; k < mp.src.size(); ++k) {
    const int se = mp.src[k].entity;
    sp.base[k] = s.h[s.cur[se]][se];
    sd.base[k] = s.hd[s.cur[se]][se];
  }
  // the primal follows the forward's per-destination rule, as the tangent pass's primal does (its
  // bits): destinations of the segmented or windowed sum read x through the batch's identity CSR
  const bool pre = mb.n_win_wg > 0 || mb.sum_seg;
  if (pre && mb.sum_seg) {
    HIP_TRY(launch_sum_seg(SumSegArgs{sp.base[0], mb.d_order, mb.d_msg_ptr, mb.d_msg_src, m.xs, mb.n_seg}, mp.din, st));
    sp.base[1] = m.xs;   // the mixed CSR's slot 1
  } else if (pre) {
    HIP_TRY(launch_sum_win(SumWinArgs{sp.base[0], mb.d_win_wg, mb.d_win_dst, mb.d_win_ptr, mb.d_win_src, m.xs, mb.n_win_wg},
                           mp.din, st));
    sp = SrcBases{};
    sp.base[0] = m.xs;   // every x from the summed table
  }
  const int c = s.cur[mp.dst];
  const SumGruArgs pa{s.h[c][mp.dst], s.h[1 - c][mp.dst], sp, mb.d_order, pre ? mb.d_id_ptr : mb.d_msg_ptr,
                      pre ? mb.d_id_src : mb.d_msg_src, rc.W, rc.U, rc.b, mb.n_dst, 0};
  HIP_TRY(launch_sum_gru_lin(pa, m.coef, mp.din, cp.H, cell_opt(cp), st));
  // the tangents: the MP's own CSR for every destination, whatever its in-degree
  const SumJacArgs ja{s.hd[c][mp.dst], s.hd[1 - c][mp.dst], sd, m.coef, mb.d_order, mb.d_msg_ptr, mb.d_msg_src,
                      rc.W, rc.U, mb.n_dst, (int32_t)(s.kp / 16)};
  HIP_TRY(launch_sum_gru_jac(ja, mp.din, cp.H, st));
  return IGN_OK;
}

int forward_jacobian(ign_plan* p, ign_batch* b, int64_t n_dir, const float* const* dfeat, float* pred, float* dpred) {
  hipStream_t st = p->stream;
  const int E = (int)p->ents.size();
  const int64_t kp = scen_padded(n_dir), P = b->n_pred, rows_d = P * kp;
  Scratch sc{b, st, "forward jacobian", {}};
  int rc;
  // ---- every block of the call first: a poisoned pool fills them on the upload stream ----
  std::vector<RawCell> raw(p->cells.size());
  for (const MPP& mp : p->mps) {
    const CellP& cp = p->cells[mp.cell];
    RawCell& r = raw[mp.cell];
    if (!r.W && ((rc = sc.get(&r.W, pack_gru_w_floats(cp.din, cp.H))) || (rc = sc.get(&r.U, pack_gru_u_floats(cp.H))) ||
                 (rc = sc.get(&r.b, pack_gru_b_floats(cp.H)))))
      return rc;
  }
  float* zero_bias = nullptr;
  if ((rc = sc.get(&zero_bias, 4 * 64))) return rc;
  States s;
  s.kp = kp;
  s.cur.assign(E, 0);
  std::vector<float*> dcopy(E, nullptr);
  for (int k = 0; k < 2; ++k) {
    s.h[k].assign(E, nullptr);
    s.hd[k].assign(E, nullptr);
  }
  for (int e = 0; e < E; ++e) {
    const int H = p->ents[e].hidden_dim, F = p->ents[e].feature_total;
    for (int k = 0; k < 2; ++k)
      if ((rc = sc.get(&s.h[k][e], b->rows[e] * H)) || (rc = sc.get(&s.hd[k][e], scen_floats(b->rows[e], kp, H)))) return rc;
    if (dfeat[e] && b->rows[e] > 0 && (rc = sc.get(&dcopy[e], n_dir * b->rows[e] * F))) return rc;
  }
  std::vector<MpScratch> ms(p->mps.size());
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {
    const MPP& mp = p->mps[mi];
    const MPB& mb = b->mp[mi];
    const int H = p->cells[mp.cell].H;
    if (mp.sorted) {
      const int64_t trows = mb.zero_row + 1 + mb.n_multi;
      if ((rc = sc.get(&ms[mi].tab, trows * 3 * H)) || (rc = sc.get(&ms[mi].tabd, scen_floats(trows, kp, 3 * H))) ||
          (rc = sc.get(&ms[mi].coef, mb.n_steps * kJacCoef * H)))
        return rc;
    } else {
      if ((rc = sc.get(&ms[mi].coef, mb.n_dst * kJacCoef * H))) return rc;
      if ((mb.n_win_wg > 0 || mb.sum_seg) && (rc = sc.get(&ms[mi].xs, std::max<int64_t>(mb.n_dst, 1) * mp.din))) return rc;
    }
  }
  float *catp = nullptr, *catd = nullptr, *lin = nullptr, *out = nullptr;
  if (p->ro_in.size() > 1 && ((rc = sc.get(&catp, P * p->ro_width)) || (rc = sc.get(&catd, rows_d * p->ro_width)))) return rc;
  int widest = 1;
  std::vector<float*> ys(p->dense.size(), nullptr), yds(p->dense.size(), nullptr);
  for (size_t l = 0; l < p->dense.size(); ++l) {
    widest = std::max(widest, p->dense[l].out);
    if ((rc = sc.get(&ys[l], P * p->dense[l].out)) || (rc = sc.get(&yds[l], rows_d * p->dense[l].out))) return rc;
  }
  if ((rc = sc.get(&lin, rows_d * widest)) || (rc = sc.get(&out, n_dir * P * b->out_units))) return rc;
  HIP_TRY(hipStreamSynchronize(upload_stream()));

  // ---- raw fragments of every cell an MP runs, from the parameters as they are now; a block of zeros ----
  for (size_t ci = 0; ci < raw.size(); ++ci) {
    const CellP& cp = p->cells[ci];
    if (raw[ci].W)
      HIP_TRY(launch_pack_gru(p->d_params + cp.off_k, p->d_params + cp.off_rk, cp.bias_rows() ? p->d_params + cp.off_b : nullptr,
                              raw[ci].W, raw[ci].U, raw[ci].b, cp.din, cp.H, kPackGruRaw | cp.bias_rows(), st));
  }
  HIP_TRY(launch_init_state(zero_bias, nullptr, 4, 64, 0, st));
  // ---- h0 = [features | 0], h0d = [direction | 0] per direction ----
  for (int e = 0; e < E; ++e) {
    const int H = p->ents[e].hidden_dim, F = p->ents[e].feature_total;
    if (dcopy[e])
      HIP_TRY(hipMemcpyAsync(dcopy[e], dfeat[e], (size_t)(n_dir * b->rows[e] * F) * sizeof(float), hipMemcpyDefault, st));
    HIP_TRY(launch_init_state(s.h[0][e], b->d_feat[e], b->rows[e], H, F, st));
    HIP_TRY(launch_init_dir(s.hd[0][e], dcopy[e], b->rows[e], n_dir, H, F, st));
  }
  // ---- the MP loop: each primal update, and behind it the K tangents of that update ----
  for (int it = 0; it < p->T; ++it)
    for (size_t mi = 0; mi < p->mps.size(); ++mi) {
      const MPP& mp = p->mps[mi];
      if (it + 1 == p->T && mp.dead_in_last_iter) continue;   // nothing reads this update (§3e)
      if ((rc = mp.sorted ? ordered_step(p, mp, b->mp[mi], raw[mp.cell], zero_bias, s, ms[mi])
                          : sum_step(p, mp, b->mp[mi], raw[mp.cell], s, ms[mi])))
        return rc;
      s.cur[mp.dst] ^= 1;
    }
  // ---- predict: the primal layer by layer keeping every y; the tangents on the flat rows ----
  std::vector<const float*> ep(E);
  for (int e = 0; e < E; ++e) ep[e] = s.h[s.cur[e]][e];
  const float* x = nullptr;
  if ((rc = predict_input(p, b, ep.data(), catp, &x, st))) return rc;
  const float* xd = s.hd[s.cur[p->ro_in[0]]][p->ro_in[0]];
  if (catd) {
    int col = 0;
    for (int id : p->ro_in) {
      const int w = p->ro_t[id].width;
      HIP_TRY(launch_concat_cols(catd, rows_d, p->ro_width, col, s.hd[s.cur[id]][id], w, st));
      col += w;
    }
    xd = catd;
  }
  int stride = p->ro_width;
  for (size_t l = 0; l < p->dense.size(); ++l) {
    const DenseP& d = p->dense[l];
    const int K = d.pk_w >= 0 ? stride : d.in;
    const float* Wp = d.pk_w >= 0 ? p->d_packed + d.pk_w : nullptr;
    const float* W = p->d_params + d.off_w;
    HIP_TRY(launch_dense_fwd(x, P, K, stride, Wp, W, d.use_bias ? p->d_params + d.off_b : nullptr, d.out, d.act, ys[l], st));
    HIP_TRY(launch_dense_fwd(xd, rows_d, K, stride, Wp, W, nullptr, d.out, IGN_ACT_LINEAR, lin, st));
    HIP_TRY(launch_act_bwd_bcast(lin, ys[l], P, kp, d.out, d.act, yds[l], st));
    x = ys[l];
    xd = yds[l];
    stride = d.out;
  }
  if (pred) HIP_TRY(hipMemcpyAsync(pred, x, (size_t)(P * b->out_units) * sizeof(float), hipMemcpyDefault, st));
  if (dpred) {
    HIP_TRY(launch_gather_dpred(xd, P, n_dir, (int)b->out_units, out, st));
    HIP_TRY(hipMemcpyAsync(dpred, out, (size_t)(n_dir * P * b->out_units) * sizeof(float), hipMemcpyDefault, st));
  }
  HIP_TRY(hipStreamSynchronize(st));   // the caller's arrays (directions in, results out) are done with
  return IGN_OK;
}

}  // namespace

extern "C" int ign_forward_jacobian(ign_batch* b, int32_t n_dir, const float* const* dfeat, int n_ents, float* pred,
                                    float* dpred) {
  if (!b || !dfeat || (!pred && !dpred)) return fail(IGN_ERR_INVALID, "forward jacobian: null argument");
  ign_plan* p = b->plan;
  int rc = check_pb(p, b);
  if (rc) return rc;
  if (n_dir < 1) return fail(IGN_ERR_INVALID, "forward jacobian: %d directions", n_dir);
  if (n_ents != (int)p->ents.size())
    return fail(IGN_ERR_INVALID, "forward jacobian: %d direction arrays for a plan of %d entities", n_ents, (int)p->ents.size());
  for (int e = 0; e < n_ents; ++e)
    if (dfeat[e] && (p->ents[e].feature_total <= 0 || !b->d_feat[e]))
      return fail(IGN_ERR_INVALID, "forward jacobian: entity %d has no features", e);
  if ((rc = jac_check_scope(p, b, "forward jacobian"))) return rc;
  return forward_jacobian(p, b, n_dir, dfeat, pred, dpred);
}
