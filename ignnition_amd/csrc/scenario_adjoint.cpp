// scenario_adjoint.cpp — ign_backward_scenarios: d(sum cot_s . pred_s) / d(features of scenario s) for S
// feature sets on the batch's topology, in one pass.  Scenarios are independent, so the
// WHOLE pass runs per chunk of scenario blocks, as a call of its own on Sp = 16 * (the chunk's blocks):
//   1. ign_forward_scenarios' primal on scenario.hip's kernels with their linearising epilogue, keeping one
//      coefficient block per MP instance PER ITERATION and every predict layer's activations;
//   2. predict's adjoint on the flat predictions * Sp rows (the existing row launches, the activations per
//      row), then the MP instances in reverse order on scenario_adjoint.hip's kernels and §3o's source
//      gather, a cotangent state [rows][Sp][H] per entity accumulating over everything that read the state.
// The chunk is the most blocks whose buffers fit kChunkMiB (IGN_SCEN_GRAD_CHUNK_MIB per call), one at
// least; a scenario's bits do not depend on it.  The transposed CSRs come from the batch's host tables
// through train_lower's routines once per call.  All device memory is scratch of the batch's pool; nothing
// of the batch is written; no training table is needed and no parameter gradient is formed.
//
// ign_backward_scenarios_params is the same chunk loop with a WGrad: d(sum_s cot_s . pred_s) /
// d(parameters), summed over the scenarios, instead of the feature gradients.  The primal then keeps what
// the contractions need -- every version of every entity's states instead of two, the ordered updates'
// h_prev tiles, the sum updates' summed messages --, the ordered adjoint runs with its recurrent weight
// gradient (scenario_wgrad.hip), and everything row-count-sized goes through launch_tsgemm_add on flat
// rows x Sp: the gradients accumulate in the reverse sweep's order, and over chunks in chunk order.

#include <cstdlib>

#include "jacobian_common.h"
#include "scenario_adjoint.h"
#include "scenario_wgrad.h"
#include "train_kernels.h"
#include "train_lower.h"

namespace {

using namespace ign;

constexpr const char* kWhat = "backward scenarios";
constexpr const char* kWhatParams = "scenario parameter gradients";
// The chunk's byte budget.  A block's buffers grow with the graph (its steps), and so does the work of one
// block: a graph whose single block exceeds the budget already fills the device with that block's waves,
// and a graph too small to do so gets as many blocks per launch as fit.
constexpr int64_t kChunkMiB = 2048;

struct MpSAdj {
  std::vector<float*> coef;             // per iteration: [n_steps or n_dst][blocks][kScenCoef][16][H]
  std::vector<int32_t*> tptr, tidx;     // per source: row -> steps (ordered) / destination rows (sum)
};

struct TCell {   // launch_pack_a's fragments of the raw W [DIN][3H] / U [H][3H]
  float *Wt = nullptr, *Ut = nullptr;
};

struct WGrad {   // what the parameter gradients add to a chunk's buffers
  bool fused = true;                       // the ordered adjoint's fused form where it exists (IGN_SCEN_WGRAD_FUSED=0: nowhere)
  float* grads = nullptr;                  // [n_params], accumulated over the chunks
  std::vector<std::vector<float*>> keep;   // per MP, per iteration: the primal's h_prev tiles (ordered) / x (sum)
  float *part = nullptr, *bsum = nullptr;  // partial tiles of a contraction, launch_seq_bwd_reduce's target
  float *ubar = nullptr, *asum = nullptr, *hpos = nullptr, *dtab = nullptr;
};

struct Pass {   // the buffers of one chunk, sized for `chunk` blocks
  std::vector<JacRawCell> raw;
  std::vector<TCell> tc;
  std::vector<MpSAdj> ms;
  // an entity's states after its k-th update: hv[e][k % size], two buffers in turn or (WGrad) every version
  std::vector<std::vector<float*>> hv;
  std::vector<float*> lam[2], fin, fout, ys;
  WGrad* g = nullptr;
  float *tab = nullptr, *blocks = nullptr, *cat = nullptr, *ga = nullptr, *gb = nullptr, *dcot = nullptr, *out = nullptr;
};

// the partial tiles of launch_tsgemm_add over n_rows, with or without a bias row, and their reduction's segments
int64_t part_floats(int64_t n_rows, int M, int N) {
  const int64_t plain = M ? tsgemm_chunks(n_rows, M, N, 0) : 0;   // (M = 0: launch_colsum_add, the bias row alone)
  return (std::max(plain, tsgemm_chunks(n_rows, M, N, 1)) + kTsReduceSegs) * (int64_t)(M + 1) * N;
}

int64_t chunk_budget() {
  const char* v = std::getenv("IGN_SCEN_GRAD_CHUNK_MIB");
  char* end = nullptr;
  const long long mib = v ? std::strtoll(v, &end, 10) : -1;
  return (v && end != v && mib >= 0 ? (int64_t)mib : kChunkMiB) << 20;
}

// scenarios [s0, s0 + ns) of the call: the whole pass on sp = ns rounded up to 16
int run_chunk(ign_plan* p, ign_batch* b, const Pass& w, int64_t s0, int64_t ns, const float* const* feat, const float* cot,
              float* pred, float* const* dfeat_out) {
  hipStream_t st = p->stream;
  const int E = (int)p->ents.size(), units = (int)b->out_units;
  const int64_t sp = scen_padded(ns), P = b->n_pred, rows_p = P * sp;
  const int32_t n_blk = (int32_t)(sp / 16);
  WGrad* g = w.g;
  std::vector<int> cur(E, 0), lcur(E, 0);
  auto hver = [&](int e, int k) { return w.hv[e][k % w.hv[e].size()]; };
  // the versions an MP instance read: [iteration][MP] {the destination's, every source's}
  struct Read { int dst, src[IGN_MAX_SLOTS]; };
  std::vector<std::vector<Read>> read(p->T, std::vector<Read>(p->mps.size()));
  HIP_TRY(hipMemcpyAsync(w.dcot, cot + s0 * P * units, (size_t)(ns * P * units) * sizeof(float), hipMemcpyDefault, st));
  // ---- h0 = [features | 0] per scenario: the caller's values, or the batch's for every scenario ----
  for (int e = 0; e < E; ++e) {
    const int H = p->ents[e].hidden_dim, F = p->ents[e].feature_total;
    if (w.fin[e])
      HIP_TRY(hipMemcpyAsync(w.fin[e], feat[e] + s0 * b->rows[e] * F, (size_t)(ns * b->rows[e] * F) * sizeof(float),
                             hipMemcpyDefault, st));
    HIP_TRY(launch_init_state_scen(hver(e, 0), w.fin[e], w.fin[e] ? nullptr : b->d_feat[e], b->rows[e], ns, H, F, st));
  }
  // ---- the primal (scenario.cpp's launches), every instance's coefficient tiles kept ----
  for (int it = 0; it < p->T; ++it)
    for (size_t mi = 0; mi < p->mps.size(); ++mi) {
      const MPP& mp = p->mps[mi];
      if (it + 1 == p->T && mp.dead_in_last_iter) continue;   // nothing reads this update (§3e)
      const MPB& mb = b->mp[mi];
      const CellP& cp = p->cells[mp.cell];
      const JacRawCell& r = w.raw[mp.cell];
      const int c = cur[mp.dst], W3 = 3 * cp.H;
      float* keep = g ? g->keep[mi][it] : nullptr;
      read[it][mi].dst = c;
      for (size_t k = 0; k < mp.src.size(); ++k) read[it][mi].src[k] = cur[mp.src[k].entity];
      if (mp.sorted) {
        for (size_t k = 0; k < mp.src.size(); ++k) {
          const int se = mp.src[k].entity;
          HIP_TRY(launch_project(hver(se, cur[se]), mb.src_rows[k] * sp, r.W, r.b, w.tab + scen_offset(mb.src_off[k], 0, sp, W3),
                                 nullptr, mp.din, cp.H, st));
        }
        HIP_TRY(launch_table_rows_scen(w.tab, mb.zero_row, mb.n_multi, mb.d_multi_ptr, mb.d_multi_rows, r.b, W3, sp, st));
        const SeqScenArgs a{hver(mp.dst, c), hver(mp.dst, c + 1), w.tab, mb.d_order, mb.d_len, mb.d_step_ptr, mb.d_step_code,
                            r.U, r.b, mb.n_dst, n_blk};
        HIP_TRY(launch_seq_gru_scen(a, cp.H, st, w.ms[mi].coef[it], keep, g && g->fused && scen_wgrad_fused_supported(cp.H)));
      } else {
        SrcBases sb{};
        for (size_t k = 0; k < mp.src.size(); ++k) sb.base[k] = hver(mp.src[k].entity, cur[mp.src[k].entity]);
        const SumScenArgs a{hver(mp.dst, c), hver(mp.dst, c + 1), sb, mb.d_order, mb.d_msg_ptr, mb.d_msg_src,
                            r.W, r.U, r.b, mb.n_dst, n_blk};
        HIP_TRY(launch_sum_gru_scen(a, mp.din, cp.H, st, w.ms[mi].coef[it], keep));
      }
      ++cur[mp.dst];
    }
  // ---- predict on the flat rows, every layer's activations kept ----
  const float* x = hver(p->ro_in[0], cur[p->ro_in[0]]);
  if (w.cat) {
    int col = 0;
    for (int id : p->ro_in) {
      const int wd = p->ro_t[id].width;
      HIP_TRY(launch_concat_cols(w.cat, rows_p, p->ro_width, col, hver(id, cur[id]), wd, st));
      col += wd;
    }
    x = w.cat;
  }
  const float* x0 = x;   // predict's input rows
  int stride = p->ro_width;
  for (size_t l = 0; l < p->dense.size(); ++l) {
    const DenseP& d = p->dense[l];
    HIP_TRY(launch_dense_fwd(x, rows_p, d.pk_w >= 0 ? stride : d.in, stride, d.pk_w >= 0 ? p->d_packed + d.pk_w : nullptr,
                             p->d_params + d.off_w, d.use_bias ? p->d_params + d.off_b : nullptr, d.out, d.act, w.ys[l], st));
    x = w.ys[l];
    stride = d.out;
  }
  if (pred) {
    HIP_TRY(launch_gather_pred_scen(x, P, ns, units, w.out, st));
    HIP_TRY(hipMemcpyAsync(pred + s0 * P * units, w.out, (size_t)(ns * P * units) * sizeof(float), hipMemcpyDefault, st));
  }
  // ---- predict's adjoint on the flat rows (a padding scenario's cotangent is zero); its input's
  // cotangent starts the entities' ----
  HIP_TRY(launch_cot_transpose(w.dcot, P, ns, units, w.ga, st));
  for (int l = (int)p->dense.size() - 1; l >= 0; --l) {
    const DenseP& d = p->dense[l];
    HIP_TRY(launch_act_bwd(w.ga, w.ys[l], rows_p * d.out, d.act, w.gb, st));
    if (g)   // dW = (the layer's input rows)^T dz, db = dz's column sums: a padding scenario's dz rows are zeros
      HIP_TRY(launch_tsgemm_add(l ? w.ys[l - 1] : x0, d.in, w.gb, d.out, rows_p, d.in, d.out, g->part, g->grads + d.off_w,
                                d.use_bias ? g->grads + d.off_b : nullptr, st));
    if (d.pk_wt >= 0)
      HIP_TRY(launch_row_gemm_t(w.gb, rows_p, d.out, p->d_packed + d.pk_wt, d.in, w.ga, 0, -1, nullptr, st));
    else
      HIP_TRY(launch_row_gemm_t_generic(w.gb, rows_p, d.out, p->d_params + d.off_w, d.in, w.ga, 0, -1, nullptr, st));
  }
  const int gw = p->dense.empty() ? units : p->dense[0].in;   // the row width of predict's input cotangent
  for (int e = 0; e < E; ++e)
    HIP_TRY(launch_init_state(w.lam[0][e], nullptr, b->rows[e] * sp, p->ents[e].hidden_dim, 0, st));
  int col = 0;
  for (int id : p->ro_in) {
    const int wd = p->ro_t[id].width;
    HIP_TRY(launch_split_cols_add(w.lam[0][id], rows_p, wd, w.ga, gw, col, st));
    col += wd;
  }
  // ---- the MP instances in reverse order ----
  for (int it = p->T - 1; it >= 0; --it)
    for (int mi = (int)p->mps.size() - 1; mi >= 0; --mi) {
      const MPP& mp = p->mps[mi];
      if (it + 1 == p->T && mp.dead_in_last_iter) continue;
      const MPB& mb = b->mp[mi];
      const MpSAdj& m = w.ms[mi];
      const CellP& cp = p->cells[mp.cell];
      const TCell& t = w.tc[mp.cell];
      const int d = mp.dst, c = lcur[d], H = cp.H, W3 = 3 * cp.H;
      float* gb = g ? g->grads + cp.off_b : nullptr;   // the raw bias tensor [2][3H]: input rows, recurrent rows
      if (mp.sorted) {
        const SeqSAdjArgs a{w.lam[c][d], w.lam[1 - c][d], m.coef[it], w.blocks, mb.d_order, mb.d_len, mb.d_step_ptr,
                            t.Ut, mb.n_dst, n_blk};
        if (!g) {
          HIP_TRY(launch_seq_gru_sadj(a, H, st));
        } else if (g->fused && scen_wgrad_fused_supported(H)) {   // dU and both bias gradients inside the sweep
          HIP_TRY(launch_seq_gru_swg(SeqSWgArgs{a, g->keep[mi][it], nullptr, g->part}, H, true, st));
          SeqBwdArgs r{};
          r.part = g->part;
          r.scratch = g->bsum;
          r.dU = g->grads + cp.off_rk;
          r.db_in = gb;
          r.db_rec = gb + W3;
          HIP_TRY(launch_seq_bwd_reduce(r, seq_swg_slots(mb.n_dst, n_blk, H), H, st));
        } else {   // ubar stored beside abar, the flat rows step * Sp + s contracted afterwards
          HIP_TRY(launch_seq_gru_swg(SeqSWgArgs{a, g->keep[mi][it], g->ubar, nullptr}, H, false, st));
          HIP_TRY(launch_tsgemm_add(g->keep[mi][it], H, g->ubar, W3, mb.n_steps * sp, H, W3, g->part, g->grads + cp.off_rk,
                                    gb + W3, st));
          HIP_TRY(launch_colsum_add(w.blocks, W3, mb.n_steps * sp, W3, g->part, gb, st));
        }
      } else {
        const SumSAdjArgs a{w.lam[c][d], w.lam[1 - c][d], m.coef[it], w.blocks, mb.d_order, t.Wt, t.Ut, mb.n_dst, n_blk};
        HIP_TRY(launch_sum_gru_sadj(a, mp.din, H, st));
        if (g) {   // dW = x^T abar, dU = h^T ubar and the bias rows, over the flat rows position * Sp + s
          const SumProductsArgs q{m.coef[it], w.lam[c][d], hver(d, read[it][mi].dst), mb.d_order, g->asum, g->ubar, g->hpos,
                                  mb.n_dst, n_blk};
          HIP_TRY(launch_sum_products_scen(q, H, st));
          HIP_TRY(launch_tsgemm_add(g->keep[mi][it], mp.din, g->asum, W3, mb.n_dst * sp, mp.din, W3, g->part,
                                    g->grads + cp.off_k, gb, st));
          HIP_TRY(launch_tsgemm_add(g->hpos, H, g->ubar, W3, mb.n_dst * sp, H, W3, g->part, g->grads + cp.off_rk, gb + W3, st));
        }
      }
      // a source read the state its entity had then: the destination's own before this update
      for (size_t s = 0; s < mp.src.size(); ++s) {
        const int se = mp.src[s].entity;
        const SrcAdjArgs sa{se == d ? w.lam[1 - c][d] : w.lam[lcur[se]][se], w.blocks, m.tptr[s], m.tidx[s],
                           mp.sorted ? t.Wt : nullptr, b->rows[se], (int32_t)sp, 0, n_blk};
        HIP_TRY(launch_src_adj(sa, mp.din, cp.H, st));
        if (g && mp.sorted) {   // dW = (the source's states then)^T (the cotangent of its projected rows)
          HIP_TRY(launch_gather_blocks_scen(g->dtab, w.blocks, m.tptr[s], m.tidx[s], b->rows[se], sp, W3, st));
          HIP_TRY(launch_tsgemm_add(hver(se, read[it][mi].src[s]), mp.din, g->dtab, W3, b->rows[se] * sp, mp.din, W3, g->part,
                                    g->grads + cp.off_k, nullptr, st));
        }
      }
      lcur[d] ^= 1;
    }
  // ---- h0 = [features | 0]: the feature columns of its cotangent ----
  for (int e = 0; e < E; ++e) {
    if (!w.fout[e]) continue;
    const int F = p->ents[e].feature_total;
    HIP_TRY(launch_feature_rows_adj(w.lam[lcur[e]][e], b->rows[e], ns, p->ents[e].hidden_dim, F, w.fout[e], st));
    HIP_TRY(hipMemcpyAsync(dfeat_out[e] + s0 * b->rows[e] * F, w.fout[e], (size_t)(ns * b->rows[e] * F) * sizeof(float),
                           hipMemcpyDefault, st));
  }
  return IGN_OK;
}

// grads_out (host or device, [n_params]): the parameter gradients instead of the feature gradients
int backward_scenarios(ign_plan* p, ign_batch* b, int64_t n_scen, const float* const* feat, const float* cot, float* pred,
                       float* const* dfeat_out, float* grads_out = nullptr) {
  hipStream_t st = p->stream;
  const int E = (int)p->ents.size(), units = (int)b->out_units;
  const int64_t P = b->n_pred, n_blk = scen_padded(n_scen) / 16;
  JacScratch sc{b, st, grads_out ? kWhatParams : kWhat, {}};
  Pass w;
  WGrad wg;
  int rc;
  std::vector<int> updates(E, 0);   // of an entity's states in one forward
  for (int it = 0; it < p->T; ++it)
    for (const MPP& mp : p->mps) updates[mp.dst] += !(it + 1 == p->T && mp.dead_in_last_iter);
  if (grads_out) {
    const char* v = std::getenv("IGN_SCEN_WGRAD_FUSED");
    wg.fused = !(v && v[0] == '0');
    w.g = &wg;
  }
  // ---- floats per scenario block of everything that grows with the chunk: that decides the chunk ----
  int64_t per_blk = 2 * 16 * P * units, tab_rows_w = 0, blocks_w = 1, ubar_w = 0, hpos_w = 0, dtab_w = 0;
  for (int e = 0; e < E; ++e)
    per_blk += b->rows[e] * 16 * (4 * (int64_t)p->ents[e].hidden_dim + 2 * p->ents[e].feature_total);
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {
    const MPP& mp = p->mps[mi];
    const MPB& mb = b->mp[mi];
    const int H = p->cells[mp.cell].H;
    const int live = p->T - (mp.dead_in_last_iter ? 1 : 0);
    per_blk += live * scen_coef_floats(mp.sorted ? mb.n_steps : mb.n_dst, 1, H);
    if (mp.sorted) {
      tab_rows_w = std::max(tab_rows_w, (mb.zero_row + 1 + mb.n_multi) * 3 * H);
      blocks_w = std::max(blocks_w, mb.n_steps * 3 * H);
    } else {
      blocks_w = std::max(blocks_w, b->rows[mp.dst] * mp.din);
    }
    if (!w.g) continue;
    // the parameter gradients' share: per iteration one more [16][H] tile per step (ordered) or
    // the summed messages per destination (sum); once, the widest of ubar (the unfused ordered form, the sum
    // update), of the sum update's abar and h rows, and of the ordered sources' gathered cotangents
    per_blk += live * 16 * (mp.sorted ? mb.n_steps * H : mb.n_dst * mp.din);
    if (mp.sorted) {
      if (!(wg.fused && scen_wgrad_fused_supported(H))) ubar_w = std::max(ubar_w, mb.n_steps * 3 * H);
      for (const auto& src : mp.src) dtab_w = std::max(dtab_w, b->rows[src.entity] * 3 * H);
    } else {
      ubar_w = std::max(ubar_w, mb.n_dst * 3 * H);
      hpos_w = std::max(hpos_w, mb.n_dst * H);
    }
  }
  if (w.g) {   // every version of an entity's states instead of two; asum is as wide as the sum updates' ubar
    for (int e = 0; e < E; ++e) per_blk += b->rows[e] * 16 * (int64_t)p->ents[e].hidden_dim * (updates[e] - 1);
    per_blk += 16 * (ubar_w + (hpos_w ? ubar_w : 0) + hpos_w + dtab_w);
  }
  int widest = std::max(units, p->ro_width);
  int64_t ys_w = 0;
  for (const DenseP& d : p->dense) {
    widest = std::max(widest, std::max(d.out, d.in));
    ys_w += d.out;
  }
  per_blk += 16 * (tab_rows_w + blocks_w + P * (ys_w + 2 * widest + (p->ro_in.size() > 1 ? p->ro_width : 0)));
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_blk, chunk_budget() / (per_blk * (int64_t)sizeof(float))));
  const int64_t spc = chunk * 16, nsc = std::min(n_scen, spc);
  // ---- every block of the call first: a poisoned pool fills them on the upload stream ----
  w.raw.resize(p->cells.size());
  w.tc.resize(p->cells.size());
  for (const MPP& mp : p->mps) {
    const CellP& cp = p->cells[mp.cell];
    JacRawCell& r = w.raw[mp.cell];
    if (!r.W && ((rc = sc.get(&r.W, pack_gru_w_floats(cp.din, cp.H))) || (rc = sc.get(&r.U, pack_gru_u_floats(cp.H))) ||
                 (rc = sc.get(&r.b, pack_gru_b_floats(cp.H))) || (rc = sc.get(&w.tc[mp.cell].Wt, pack_gru_w_floats(cp.din, cp.H))) ||
                 (rc = sc.get(&w.tc[mp.cell].Ut, pack_gru_u_floats(cp.H)))))
      return rc;
  }
  w.fin.assign(E, nullptr);
  w.fout.assign(E, nullptr);
  for (int k = 0; k < 2; ++k) w.lam[k].assign(E, nullptr);
  w.hv.resize(E);
  for (int e = 0; e < E; ++e) {
    const int H = p->ents[e].hidden_dim, F = p->ents[e].feature_total;
    w.hv[e].assign(w.g ? std::max(2, updates[e] + 1) : 2, nullptr);
    for (int k = 0; k < 2; ++k)
      if ((rc = sc.get(&w.hv[e][k], scen_floats(b->rows[e], spc, H))) || (rc = sc.get(&w.lam[k][e], scen_floats(b->rows[e], spc, H))))
        return rc;
    for (size_t k = 2; k < w.hv[e].size(); ++k)
      if ((rc = sc.get(&w.hv[e][k], scen_floats(b->rows[e], spc, H)))) return rc;
    if (feat && feat[e] && b->rows[e] > 0 && (rc = sc.get(&w.fin[e], nsc * b->rows[e] * F))) return rc;
    if (dfeat_out[e] && b->rows[e] > 0 && (rc = sc.get(&w.fout[e], nsc * b->rows[e] * F))) return rc;
  }
  w.ms.resize(p->mps.size());
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {
    const MPP& mp = p->mps[mi];
    const MPB& mb = b->mp[mi];
    MpSAdj& m = w.ms[mi];
    const int H = p->cells[mp.cell].H, S = (int)mp.src.size();
    m.coef.assign(p->T, nullptr);
    for (int it = 0; it < p->T; ++it)
      if (!(it + 1 == p->T && mp.dead_in_last_iter) &&
          (rc = sc.get(&m.coef[it], scen_coef_floats(mp.sorted ? mb.n_steps : mb.n_dst, chunk, H))))
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
  if (tab_rows_w && (rc = sc.get(&w.tab, tab_rows_w * spc))) return rc;
  if ((rc = sc.get(&w.blocks, blocks_w * spc))) return rc;
  if (p->ro_in.size() > 1 && (rc = sc.get(&w.cat, P * spc * p->ro_width))) return rc;
  w.ys.assign(p->dense.size(), nullptr);
  for (size_t l = 0; l < p->dense.size(); ++l)
    if ((rc = sc.get(&w.ys[l], P * spc * p->dense[l].out))) return rc;
  if ((rc = sc.get(&w.ga, P * spc * widest)) || (rc = sc.get(&w.gb, P * spc * widest)) ||
      (rc = sc.get(&w.dcot, nsc * P * units)) || (rc = sc.get(&w.out, nsc * P * units)))
    return rc;
  if (w.g) {
    // a contraction's partial tiles (launch_tsgemm_add), the fused ordered adjoint's (launch_seq_bwd_reduce)
    int64_t part_w = 1, bsum_w = 1;
    wg.keep.resize(p->mps.size());
    for (size_t mi = 0; mi < p->mps.size(); ++mi) {
      const MPP& mp = p->mps[mi];
      const MPB& mb = b->mp[mi];
      const int H = p->cells[mp.cell].H, W3 = 3 * H;
      wg.keep[mi].assign(p->T, nullptr);
      for (int it = 0; it < p->T; ++it)
        if (w.ms[mi].coef[it] && (rc = sc.get(&wg.keep[mi][it], 16 * chunk * (mp.sorted ? mb.n_steps * H : mb.n_dst * mp.din))))
          return rc;
      if (mp.sorted) {
        if (wg.fused && scen_wgrad_fused_supported(H)) {
          part_w = std::max(part_w, (seq_swg_slots(mb.n_dst, (int32_t)chunk, H) + kTsReduceSegs) * (int64_t)(H + 2) * W3);
          bsum_w = std::max<int64_t>(bsum_w, (H + 1) * W3);
        } else {
          part_w = std::max({part_w, part_floats(mb.n_steps * spc, H, W3), part_floats(mb.n_steps * spc, 0, W3)});
        }
        for (const auto& src : mp.src) part_w = std::max(part_w, part_floats(b->rows[src.entity] * spc, mp.din, W3));
      } else {
        part_w = std::max({part_w, part_floats(mb.n_dst * spc, mp.din, W3), part_floats(mb.n_dst * spc, H, W3)});
      }
    }
    for (const DenseP& d : p->dense) part_w = std::max(part_w, part_floats(P * spc, d.in, d.out));
    if ((rc = sc.get(&wg.grads, p->n_params)) || (rc = sc.get(&wg.part, part_w)) || (rc = sc.get(&wg.bsum, bsum_w)) ||
        (rc = sc.get(&wg.ubar, ubar_w * spc)) || (rc = sc.get(&wg.dtab, dtab_w * spc)) ||
        (hpos_w && ((rc = sc.get(&wg.asum, ubar_w * spc)) || (rc = sc.get(&wg.hpos, hpos_w * spc)))))
      return rc;
  }
  HIP_TRY(hipStreamSynchronize(upload_stream()));
  if (w.g) {
    set_tsgemm_bf(p->tsgemm_bf);
    HIP_TRY(hipMemsetAsync(wg.grads, 0, std::max<int64_t>(p->n_params, 1) * sizeof(float), st));
  }

  // ---- raw fragments of every cell an MP runs, forward and transposed, from the parameters as they are now ----
  for (size_t ci = 0; ci < w.raw.size(); ++ci) {
    const CellP& cp = p->cells[ci];
    if (!w.raw[ci].W) continue;
    HIP_TRY(launch_pack_gru(p->d_params + cp.off_k, p->d_params + cp.off_rk, p->d_params + cp.off_b, w.raw[ci].W, w.raw[ci].U,
                            w.raw[ci].b, cp.din, cp.H, kPackGruRaw | cp.bias_rows(), st));
    HIP_TRY(launch_pack_a(p->d_params + cp.off_k, cp.din, 3 * cp.H, w.tc[ci].Wt, st));
    HIP_TRY(launch_pack_a(p->d_params + cp.off_rk, cp.H, 3 * cp.H, w.tc[ci].Ut, st));
  }
  for (int64_t s0 = 0; s0 < n_scen; s0 += spc)
    if ((rc = run_chunk(p, b, w, s0, std::min(spc, n_scen - s0), feat, cot, pred, dfeat_out))) return rc;
  if (w.g) HIP_TRY(hipMemcpyAsync(grads_out, wg.grads, (size_t)p->n_params * sizeof(float), hipMemcpyDefault, st));
  HIP_TRY(hipStreamSynchronize(st));   // the caller's arrays (features and cotangents in, results out) are done with
  return IGN_OK;
}

}  // namespace

extern "C" int ign_backward_scenarios(ign_batch* b, int32_t n_scen, const float* const* feat, int n_ents, const float* cot,
                                      float* pred, float* const* dfeat_out) {
  if (!b || !cot || !dfeat_out) return fail(IGN_ERR_INVALID, "backward scenarios: null argument");
  ign_plan* p = b->plan;
  int rc = check_pb(p, b);
  if (rc) return rc;
  if (n_scen < 1) return fail(IGN_ERR_INVALID, "backward scenarios: %d scenarios", n_scen);
  if (n_ents != (int)p->ents.size())
    return fail(IGN_ERR_INVALID, "backward scenarios: %d arrays for a plan of %d entities", n_ents, (int)p->ents.size());
  for (int e = 0; e < n_ents; ++e)
    if (((feat && feat[e]) || dfeat_out[e]) && (p->ents[e].feature_total <= 0 || !b->d_feat[e]))
      return fail(IGN_ERR_INVALID, "backward scenarios: entity %d has no features", e);
  if ((rc = scen_check_scope(p, b, kWhat)) || (rc = adj_check_layout(p, b, kWhat))) return rc;
  return backward_scenarios(p, b, n_scen, feat, cot, pred, dfeat_out);
}

extern "C" int ign_backward_scenarios_params(ign_batch* b, int32_t n_scen, const float* const* feat, int n_ents, const float* cot,
                                             float* pred, float* grads) {
  if (!b || !cot || !grads) return fail(IGN_ERR_INVALID, "%s: null argument", kWhatParams);
  ign_plan* p = b->plan;
  int rc = check_pb(p, b);
  if (rc) return rc;
  if (n_scen < 1) return fail(IGN_ERR_INVALID, "%s: %d scenarios", kWhatParams, n_scen);
  if (n_ents != (int)p->ents.size())
    return fail(IGN_ERR_INVALID, "%s: %d arrays for a plan of %d entities", kWhatParams, n_ents, (int)p->ents.size());
  for (int e = 0; e < n_ents; ++e)
    if (feat && feat[e] && (p->ents[e].feature_total <= 0 || !b->d_feat[e]))
      return fail(IGN_ERR_INVALID, "%s: entity %d has no features", kWhatParams, e);
  if ((rc = scen_check_scope(p, b, kWhatParams)) || (rc = adj_check_layout(p, b, kWhatParams))) return rc;
  const std::vector<float*> no_features(p->ents.size(), nullptr);
  return backward_scenarios(p, b, n_scen, feat, cot, pred, no_features.data(), grads);
}
