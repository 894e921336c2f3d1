// adjoint.cpp — ign_backward_jacobian: K prediction cotangents through one adjoint sweep of the linearised
// forward.  Phase 1 is ign_forward_jacobian's primal loop without the tangents (the same
// launches, so pred is its pred bit for bit), keeping one coefficient block per MP instance PER ITERATION
// and every predict layer's activations.  Phase 2 walks back: predict's adjoint on the flat
// predictions * Kp rows (the existing row launches), then the MP instances in reverse order on
// adjoint.hip's kernels, a cotangent state [rows][Kp][H] per entity accumulating over everything that
// read the state.  The per-step cotangent blocks are sized for a chunk of cotangent blocks (kChunkBytes)
// with a host loop over the chunks.  The transposed CSRs (source row -> the steps / destinations that read
// it, ascending) come from the batch's host tables through train_lower's routines, multi rows included,
// once per call.  All device memory is scratch of the batch's pool; nothing of the batch is written; no
// training table is needed and no parameter gradient is formed.

#include "adjoint.h"
#include "jacobian_common.h"
#include "train_kernels.h"
#include "train_lower.h"

namespace {

using namespace ign;

constexpr const char* kWhat = "backward jacobian";
constexpr int64_t kChunkBytes = 256LL << 20;   // the per-step cotangent buffer's budget

struct MpAdj {
  float* tab = nullptr;                 // ordered: the primal's projected table (rewritten every iteration)
  float* xs = nullptr;                  // sum with a segmented / windowed class: the primal's summed rows
  std::vector<float*> coef;             // per iteration: [n_steps or n_dst][kJacCoef][H]
  std::vector<int32_t*> tptr, tidx;     // per source: row -> steps (ordered) / destination rows (sum)
};

struct TCell {   // launch_pack_a's fragments of the raw W [DIN][3H] / U [H][3H]
  float *Wt = nullptr, *Ut = nullptr;
};

int backward_jacobian(ign_plan* p, ign_batch* b, int64_t n_cot, const float* cot, float* pred, float* const* dfeat_out) {
  hipStream_t st = p->stream;
  const int E = (int)p->ents.size();
  const int units = (int)b->out_units;
  const int64_t kp = scen_padded(n_cot), P = b->n_pred, rows_d = P * kp;
  const int32_t n_blk = (int32_t)(kp / 16);
  JacScratch sc{b, st, kWhat, {}};
  int rc;
  // ---- every block of the call first: a poisoned pool fills them on the upload stream ----
  std::vector<JacRawCell> raw(p->cells.size());
  std::vector<TCell> tc(p->cells.size());
  for (const MPP& mp : p->mps) {
    const CellP& cp = p->cells[mp.cell];
    JacRawCell& r = raw[mp.cell];
    if (!r.W && ((rc = sc.get(&r.W, pack_gru_w_floats(cp.din, cp.H))) || (rc = sc.get(&r.U, pack_gru_u_floats(cp.H))) ||
                 (rc = sc.get(&r.b, pack_gru_b_floats(cp.H))) || (rc = sc.get(&tc[mp.cell].Wt, pack_gru_w_floats(cp.din, cp.H))) ||
                 (rc = sc.get(&tc[mp.cell].Ut, pack_gru_u_floats(cp.H)))))
      return rc;
  }
  std::vector<float*> h[2], lam[2], fout(E, nullptr);
  std::vector<int> cur(E, 0), lcur(E, 0);
  for (int k = 0; k < 2; ++k) {
    h[k].assign(E, nullptr);
    lam[k].assign(E, nullptr);
  }
  for (int e = 0; e < E; ++e) {
    const int H = p->ents[e].hidden_dim, F = p->ents[e].feature_total;
    for (int k = 0; k < 2; ++k)
      if ((rc = sc.get(&h[k][e], b->rows[e] * H)) || (rc = sc.get(&lam[k][e], scen_floats(b->rows[e], kp, H)))) return rc;
    if (dfeat_out[e] && b->rows[e] > 0 && (rc = sc.get(&fout[e], n_cot * b->rows[e] * F))) return rc;
  }
  // the step / destination blocks of one chunk: the largest MP's need per cotangent block decides the chunk
  int64_t per_blk = 1;
  std::vector<MpAdj> ms(p->mps.size());
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {
    const MPP& mp = p->mps[mi];
    const MPB& mb = b->mp[mi];
    MpAdj& m = ms[mi];
    const int H = p->cells[mp.cell].H, S = (int)mp.src.size();
    if (mp.sorted) {
      if ((rc = sc.get(&m.tab, (mb.zero_row + 1 + mb.n_multi) * 3 * H))) return rc;
      per_blk = std::max(per_blk, mb.n_steps * 16 * 3 * H);
    } else {
      if ((mb.n_win_wg > 0 || mb.sum_seg) && (rc = sc.get(&m.xs, std::max<int64_t>(mb.n_dst, 1) * mp.din))) return rc;
      per_blk = std::max(per_blk, mb.n_dst * 16 * mp.din);
    }
    m.coef.assign(p->T, nullptr);
    for (int it = 0; it < p->T; ++it)
      if (!(it + 1 == p->T && mp.dead_in_last_iter) &&
          (rc = sc.get(&m.coef[it], (mp.sorted ? mb.n_steps : mb.n_dst) * kJacCoef * H)))
        return rc;
    // source row -> its readers, in ascending step / message order (train_lower.h), from the host tables
    std::vector<int64_t> keys(S);
    for (int s = 0; s < S; ++s) keys[s] = b->rows[mp.src[s].entity];
    const TrainMpIn in{mb.h_order, mb.h_len, mb.h_step_ptr, mb.h_msg_ptr, mb.h_multi_ptr, mb.h_step_code,
                       mb.h_msg_src, mb.h_multi_rows, mb.src_off, mb.zero_row, mb.n_dst, mb.n_msgs};
    std::vector<hvec<int32_t>> hp, hi;
    if (mp.sorted) lower_train_ordered(S, keys.data(), in, hp, hi);
    else lower_train_sum(S, keys.data(), in, hp, hi);
    m.tptr.assign(S, nullptr);
    m.tidx.assign(S, nullptr);
    for (int s = 0; s < S; ++s)
      if ((rc = jac_upload_i32(sc, hp[s], &m.tptr[s])) || (rc = jac_upload_i32(sc, hi[s], &m.tidx[s]))) return rc;
  }
  const int32_t chunk = (int32_t)std::max<int64_t>(1, std::min<int64_t>(n_blk, kChunkBytes / (per_blk * (int64_t)sizeof(float))));
  float* blocks = nullptr;
  if ((rc = sc.get(&blocks, per_blk * chunk))) return rc;
  float *catp = nullptr, *ga = nullptr, *gb = nullptr, *dcot = nullptr;
  if (p->ro_in.size() > 1 && (rc = sc.get(&catp, P * p->ro_width))) return rc;
  int widest = std::max(units, p->ro_width);
  std::vector<float*> ys(p->dense.size(), nullptr);
  for (size_t l = 0; l < p->dense.size(); ++l) {
    widest = std::max(widest, std::max(p->dense[l].out, p->dense[l].in));
    if ((rc = sc.get(&ys[l], P * p->dense[l].out))) return rc;
  }
  if ((rc = sc.get(&ga, rows_d * widest)) || (rc = sc.get(&gb, rows_d * widest)) || (rc = sc.get(&dcot, n_cot * P * units)))
    return rc;
  HIP_TRY(hipStreamSynchronize(upload_stream()));

  // ---- raw fragments of every cell an MP runs, forward and transposed, from the parameters as they are now ----
  for (size_t ci = 0; ci < raw.size(); ++ci) {
    const CellP& cp = p->cells[ci];
    if (!raw[ci].W) continue;
    HIP_TRY(launch_pack_gru(p->d_params + cp.off_k, p->d_params + cp.off_rk, cp.bias_rows() ? p->d_params + cp.off_b : nullptr,
                            raw[ci].W, raw[ci].U, raw[ci].b, cp.din, cp.H, kPackGruRaw | cp.bias_rows(), st));
    HIP_TRY(launch_pack_a(p->d_params + cp.off_k, cp.din, 3 * cp.H, tc[ci].Wt, st));
    HIP_TRY(launch_pack_a(p->d_params + cp.off_rk, cp.H, 3 * cp.H, tc[ci].Ut, st));
  }
  HIP_TRY(hipMemcpyAsync(dcot, cot, (size_t)(n_cot * P * units) * sizeof(float), hipMemcpyDefault, st));
  for (int e = 0; e < E; ++e)
    HIP_TRY(launch_init_state(h[0][e], b->d_feat[e], b->rows[e], p->ents[e].hidden_dim, p->ents[e].feature_total, st));

  // ---- phase 1: the primal, every instance's coefficient rows kept ----
  for (int it = 0; it < p->T; ++it)
    for (size_t mi = 0; mi < p->mps.size(); ++mi) {
      const MPP& mp = p->mps[mi];
      if (it + 1 == p->T && mp.dead_in_last_iter) continue;   // nothing reads this update (§3e)
      const MPB& mb = b->mp[mi];
      const MpAdj& m = ms[mi];
      const CellP& cp = p->cells[mp.cell];
      const JacRawCell& r = raw[mp.cell];
      const int c = cur[mp.dst], W3 = 3 * cp.H;
      if (mp.sorted) {
        for (size_t k = 0; k < mp.src.size(); ++k) {
          const int se = mp.src[k].entity;
          HIP_TRY(launch_project(h[cur[se]][se], mb.src_rows[k], r.W, r.b, m.tab + mb.src_off[k] * W3,
                                 k == 0 ? m.tab + mb.zero_row * W3 : nullptr, mp.din, cp.H, st));
        }
        if (mb.n_multi)
          HIP_TRY(launch_multi_sum(m.tab, mb.zero_row + 1, mb.n_multi, mb.d_multi_ptr, mb.d_multi_rows, W3, m.tab + mb.zero_row * W3, st));
        const SeqGruArgs pa{h[c][mp.dst], h[1 - c][mp.dst], m.tab, mb.d_order, mb.d_len, mb.d_step_ptr, mb.d_step_code,
                            r.U, r.b, mb.n_dst, 0};
        HIP_TRY(launch_seq_gru_lin(pa, m.coef[it], cp.H, cell_opt(cp), st));
      } else {
        SrcBases sp{};
        for (size_t k = 0; k < mp.src.size(); ++k) sp.base[k] = h[cur[mp.src[k].entity]][mp.src[k].entity];
        const bool pre = mb.n_win_wg > 0 || mb.sum_seg;   // the forward's per-destination rule, as §3n's primal
        if (pre && mb.sum_seg) {
          HIP_TRY(launch_sum_seg(SumSegArgs{sp.base[0], mb.d_order, mb.d_msg_ptr, mb.d_msg_src, m.xs, mb.n_seg}, mp.din, st));
          sp.base[1] = m.xs;
        } else if (pre) {
          HIP_TRY(launch_sum_win(SumWinArgs{sp.base[0], mb.d_win_wg, mb.d_win_dst, mb.d_win_ptr, mb.d_win_src, m.xs, mb.n_win_wg},
                                 mp.din, st));
          sp = SrcBases{};
          sp.base[0] = m.xs;
        }
        const SumGruArgs pa{h[c][mp.dst], h[1 - c][mp.dst], sp, mb.d_order, pre ? mb.d_id_ptr : mb.d_msg_ptr,
                            pre ? mb.d_id_src : mb.d_msg_src, r.W, r.U, r.b, mb.n_dst, 0};
        HIP_TRY(launch_sum_gru_lin(pa, m.coef[it], mp.din, cp.H, cell_opt(cp), st));
      }
      cur[mp.dst] ^= 1;
    }
  std::vector<const float*> ep(E);
  for (int e = 0; e < E; ++e) ep[e] = h[cur[e]][e];
  const float* x = nullptr;
  if ((rc = predict_input(p, b, ep.data(), catp, &x, st))) return rc;
  int stride = p->ro_width;
  for (size_t l = 0; l < p->dense.size(); ++l) {
    const DenseP& d = p->dense[l];
    const int K = d.pk_w >= 0 ? stride : d.in;
    HIP_TRY(launch_dense_fwd(x, P, K, stride, d.pk_w >= 0 ? p->d_packed + d.pk_w : nullptr, p->d_params + d.off_w,
                             d.use_bias ? p->d_params + d.off_b : nullptr, d.out, d.act, ys[l], st));
    x = ys[l];
    stride = d.out;
  }
  if (pred) HIP_TRY(hipMemcpyAsync(pred, x, (size_t)(P * units) * sizeof(float), hipMemcpyDefault, st));

  // ---- phase 2: predict's adjoint on the flat rows; its input's cotangent starts the entities' ----
  HIP_TRY(launch_cot_transpose(dcot, P, n_cot, units, ga, st));
  for (int l = (int)p->dense.size() - 1; l >= 0; --l) {
    const DenseP& d = p->dense[l];
    HIP_TRY(launch_act_bwd_bcast(ga, ys[l], P, kp, d.out, d.act, gb, st));
    if (d.pk_wt >= 0)
      HIP_TRY(launch_row_gemm_t(gb, rows_d, d.out, p->d_packed + d.pk_wt, d.in, ga, 0, -1, nullptr, st));
    else
      HIP_TRY(launch_row_gemm_t_generic(gb, rows_d, d.out, p->d_params + d.off_w, d.in, ga, 0, -1, nullptr, st));
  }
  const int gw = p->dense.empty() ? units : p->dense[0].in;   // the row width of predict's input cotangent
  for (int e = 0; e < E; ++e)
    HIP_TRY(launch_init_state(lam[0][e], nullptr, b->rows[e] * kp, p->ents[e].hidden_dim, 0, st));
  int col = 0;
  for (int id : p->ro_in) {
    const int w = p->ro_t[id].width;
    HIP_TRY(launch_split_cols_add(lam[0][id], rows_d, w, ga, gw, col, st));
    col += w;
  }
  // ---- the MP instances in reverse order ----
  for (int it = p->T - 1; it >= 0; --it)
    for (int mi = (int)p->mps.size() - 1; mi >= 0; --mi) {
      const MPP& mp = p->mps[mi];
      if (it + 1 == p->T && mp.dead_in_last_iter) continue;
      const MPB& mb = b->mp[mi];
      const MpAdj& m = ms[mi];
      const CellP& cp = p->cells[mp.cell];
      const int d = mp.dst, c = lcur[d];
      for (int32_t b0 = 0; b0 < n_blk; b0 += chunk) {
        const int32_t nb = std::min(chunk, n_blk - b0);
        if (mp.sorted) {
          const SeqAdjArgs a{lam[c][d], lam[1 - c][d], m.coef[it], blocks, mb.d_order, mb.d_len, mb.d_step_ptr,
                             tc[mp.cell].Ut, mb.n_dst, (int32_t)kp, b0, nb};
          HIP_TRY(launch_seq_gru_adj(a, cp.H, st));
        } else {
          const SumAdjArgs a{lam[c][d], lam[1 - c][d], m.coef[it], blocks, mb.d_order, tc[mp.cell].Wt, tc[mp.cell].Ut,
                             mb.n_dst, (int32_t)kp, b0, nb};
          HIP_TRY(launch_sum_gru_adj(a, mp.din, cp.H, st));
        }
        // a source read the state its entity had then: the destination's own before this update
        for (size_t s = 0; s < mp.src.size(); ++s) {
          const int se = mp.src[s].entity;
          const SrcAdjArgs g{se == d ? lam[1 - c][d] : lam[lcur[se]][se], blocks, m.tptr[s], m.tidx[s],
                             mp.sorted ? tc[mp.cell].Wt : nullptr, b->rows[se], (int32_t)kp, b0, nb};
          HIP_TRY(launch_src_adj(g, mp.din, cp.H, st));
        }
      }
      lcur[d] ^= 1;
    }
  // ---- h0 = [features | 0]: the feature columns of its cotangent ----
  for (int e = 0; e < E; ++e) {
    if (!fout[e]) continue;
    const int F = p->ents[e].feature_total;
    HIP_TRY(launch_feature_rows_adj(lam[lcur[e]][e], b->rows[e], n_cot, p->ents[e].hidden_dim, F, fout[e], st));
    HIP_TRY(hipMemcpyAsync(dfeat_out[e], fout[e], (size_t)(n_cot * b->rows[e] * F) * sizeof(float), hipMemcpyDefault, st));
  }
  HIP_TRY(hipStreamSynchronize(st));   // the caller's arrays (cotangents in, results out) are done with
  return IGN_OK;
}

}  // namespace

extern "C" int ign_backward_jacobian(ign_batch* b, int32_t n_cot, const float* cot, int n_ents, float* pred,
                                     float* const* dfeat_out) {
  if (!b || !cot || !dfeat_out) return fail(IGN_ERR_INVALID, "backward jacobian: null argument");
  ign_plan* p = b->plan;
  int rc = check_pb(p, b);
  if (rc) return rc;
  if (n_cot < 1) return fail(IGN_ERR_INVALID, "backward jacobian: %d cotangents", n_cot);
  if (n_ents != (int)p->ents.size())
    return fail(IGN_ERR_INVALID, "backward jacobian: %d output arrays for a plan of %d entities", n_ents, (int)p->ents.size());
  for (int e = 0; e < n_ents; ++e)
    if (dfeat_out[e] && (p->ents[e].feature_total <= 0 || !b->d_feat[e]))
      return fail(IGN_ERR_INVALID, "backward jacobian: entity %d has no features", e);
  if ((rc = jac_check_scope(p, b, kWhat))) return rc;
  if ((rc = adj_check_layout(p, b, kWhat))) return rc;
  return backward_jacobian(p, b, n_cot, cot, pred, dfeat_out);
}
