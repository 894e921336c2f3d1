// scenario.cpp — ign_forward_scenarios: S feature sets on the batch's topology in one pass (DESIGN.md
// §3m).  Every entity keeps ping-pong states [row][Sp][H] in scratch blocks of the batch's pool (Sp = S
// rounded up to 16); the MP instances run in the forward's order on scenario.hip's kernels, over the
// batch's own index tables, which are read and never copied; what works on independent rows runs the
// existing launches on the rows * Sp flat rows: project on the raw W fragments, and predict's Dense
// stack.  Nothing of the batch is written: its states, tables, feature buffer, predictions and
// captured graph stay as the last forward left them.

#include "jacobian_common.h"
#include "scenario.h"
#include "train_kernels.h"

namespace {

using namespace ign;

// scratch of one call: blocks of the batch's pool, handed back behind the plan's stream.  They are
// taken as scratch blocks (IGN_POOL_POISON=1 fills them with NaN): no kernel here may read what no
// kernel here wrote.
struct Scratch {
  ign_batch* b;
  hipStream_t st;
  std::vector<void*> blocks;
  ~Scratch() {
    if (!blocks.empty()) pool_release(b->pool.get(), blocks, st);
  }
  int get(float** out, int64_t n) {
    void* q = nullptr;
    const size_t bytes = (size_t)(std::max<int64_t>(n, 0) + 256) * sizeof(float);
    const hipError_t e = pool_alloc(b->pool.get(), &q, bytes, true);
    if (e != hipSuccess)
      return fail(IGN_ERR_OOM, "forward scenarios: device alloc (%zu bytes): %s", bytes, hipGetErrorString(e));
    blocks.push_back(q);
    *out = static_cast<float*>(q);
    return IGN_OK;
  }
};

struct RawCell {   // pack_gru's unscaled form of one cell, packed per call from the live parameters
  float *W = nullptr, *U = nullptr, *b = nullptr;
};

struct ScenStates {   // per entity: ping-pong states [rows][Sp][H]
  std::vector<float*> h[2];
  std::vector<int> cur;
  int64_t sp = 0;
};

// The projected table [sources' rows | hole | multi rows][Sp][3H]: project_kernel on each source's
// rows * Sp flat rows, then the two kinds of row no source projects.
int ordered_step(ign_plan* p, const MPP& mp, const MPB& mb, const RawCell& rc, const ScenStates& s, float* tab) {
  hipStream_t st = p->stream;
  const CellP& cp = p->cells[mp.cell];
  const int W3 = 3 * cp.H;
  for (size_t k = 0; k < mp.src.size(); ++k) {
    const int se = mp.src[k].entity;
    HIP_TRY(launch_project(s.h[s.cur[se]][se], mb.src_rows[k] * s.sp, rc.W, rc.b, tab + scen_offset(mb.src_off[k], 0, s.sp, W3),
                           nullptr, mp.din, cp.H, st));
  }
  HIP_TRY(launch_table_rows_scen(tab, mb.zero_row, mb.n_multi, mb.d_multi_ptr, mb.d_multi_rows, rc.b, W3, s.sp, st));
  const int c = s.cur[mp.dst];
  const SeqScenArgs a{s.h[c][mp.dst], s.h[1 - c][mp.dst], tab, mb.d_order, mb.d_len, mb.d_step_ptr, mb.d_step_code,
                      rc.U, rc.b, mb.n_dst, (int32_t)(s.sp / 16)};
  HIP_TRY(launch_seq_gru_scen(a, cp.H, st));
  return IGN_OK;
}

// The MP's own CSR for every destination, whatever its in-degree: no windowed or segmented class.
int sum_step(ign_plan* p, const MPP& mp, const MPB& mb, const RawCell& rc, const ScenStates& s) {
  const CellP& cp = p->cells[mp.cell];
  SrcBases sb{};
  for (size_t k = 0; k < mp.src.size(); ++k) sb.base[k] = s.h[s.cur[mp.src[k].entity]][mp.src[k].entity];
  const int c = s.cur[mp.dst];
  const SumScenArgs a{s.h[c][mp.dst], s.h[1 - c][mp.dst], sb, mb.d_order, mb.d_msg_ptr, mb.d_msg_src,
                      rc.W, rc.U, rc.b, mb.n_dst, (int32_t)(s.sp / 16)};
  HIP_TRY(launch_sum_gru_scen(a, mp.din, cp.H, p->stream));
  return IGN_OK;
}

int forward_scenarios(ign_plan* p, ign_batch* b, int64_t n_scen, const float* const* feat, float* pred) {
  hipStream_t st = p->stream;
  const int E = (int)p->ents.size();
  const int64_t sp = scen_padded(n_scen), P = b->n_pred, rows_pred = P * sp;
  Scratch sc{b, st, {}};
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
  ScenStates s;
  s.sp = sp;
  s.cur.assign(E, 0);
  std::vector<float*> fcopy(E, nullptr);
  for (int k = 0; k < 2; ++k) s.h[k].assign(E, nullptr);
  for (int e = 0; e < E; ++e) {
    const int H = p->ents[e].hidden_dim, F = p->ents[e].feature_total;
    for (int k = 0; k < 2; ++k)
      if ((rc = sc.get(&s.h[k][e], scen_floats(b->rows[e], sp, H)))) return rc;
    if (feat && feat[e] && b->rows[e] > 0 && (rc = sc.get(&fcopy[e], n_scen * b->rows[e] * F))) return rc;
  }
  std::vector<float*> tab(p->mps.size(), nullptr);
  for (size_t mi = 0; mi < p->mps.size(); ++mi)
    if (p->mps[mi].sorted &&
        (rc = sc.get(&tab[mi], scen_floats(b->mp[mi].zero_row + 1 + b->mp[mi].n_multi, sp, 3 * p->cells[p->mps[mi].cell].H))))
      return rc;
  float* cat = nullptr;
  if (p->ro_in.size() > 1 && (rc = sc.get(&cat, rows_pred * p->ro_width))) return rc;
  std::vector<float*> ys(p->dense.size(), nullptr);
  for (size_t l = 0; l < p->dense.size(); ++l)
    if ((rc = sc.get(&ys[l], rows_pred * p->dense[l].out))) return rc;
  float* out = nullptr;
  if ((rc = sc.get(&out, n_scen * P * b->out_units))) return rc;
  HIP_TRY(hipStreamSynchronize(upload_stream()));

  // ---- raw fragments of every cell an MP runs, from the parameters as they are now ----
  for (size_t ci = 0; ci < raw.size(); ++ci) {
    const CellP& cp = p->cells[ci];
    if (raw[ci].W)
      HIP_TRY(launch_pack_gru(p->d_params + cp.off_k, p->d_params + cp.off_rk, p->d_params + cp.off_b, raw[ci].W, raw[ci].U,
                              raw[ci].b, cp.din, cp.H, kPackGruRaw | cp.bias_rows(), st));
  }
  // ---- h0 = [features | 0] per scenario: the caller's values, or the batch's for every scenario ----
  for (int e = 0; e < E; ++e) {
    const int H = p->ents[e].hidden_dim, F = p->ents[e].feature_total;
    if (fcopy[e])
      HIP_TRY(hipMemcpyAsync(fcopy[e], feat[e], (size_t)(n_scen * b->rows[e] * F) * sizeof(float), hipMemcpyDefault, st));
    HIP_TRY(launch_init_state_scen(s.h[0][e], fcopy[e], fcopy[e] ? nullptr : b->d_feat[e], b->rows[e], n_scen, H, F, st));
  }
  // ---- the MP loop ----
  for (int it = 0; it < p->T; ++it)
    for (size_t mi = 0; mi < p->mps.size(); ++mi) {
      const MPP& mp = p->mps[mi];
      if (it + 1 == p->T && mp.dead_in_last_iter) continue;   // nothing reads this update (§3e)
      if ((rc = mp.sorted ? ordered_step(p, mp, b->mp[mi], raw[mp.cell], s, tab[mi]) : sum_step(p, mp, b->mp[mi], raw[mp.cell], s)))
        return rc;
      s.cur[mp.dst] ^= 1;
    }
  // ---- predict on the flat rows (a Dropout layer is the identity), then [S][predictions][units] ----
  const float* x = s.h[s.cur[p->ro_in[0]]][p->ro_in[0]];
  if (cat) {
    int col = 0;
    for (int id : p->ro_in) {
      const int w = p->ro_t[id].width;
      HIP_TRY(launch_concat_cols(cat, rows_pred, p->ro_width, col, s.h[s.cur[id]][id], w, st));
      col += w;
    }
    x = cat;
  }
  int stride = p->ro_width;
  for (size_t l = 0; l < p->dense.size(); ++l) {
    const DenseP& d = p->dense[l];
    HIP_TRY(launch_dense_fwd(x, rows_pred, d.pk_w >= 0 ? stride : d.in, stride, d.pk_w >= 0 ? p->d_packed + d.pk_w : nullptr,
                             p->d_params + d.off_w, d.use_bias ? p->d_params + d.off_b : nullptr, d.out, d.act, ys[l], st));
    x = ys[l];
    stride = d.out;
  }
  HIP_TRY(launch_gather_pred_scen(x, P, n_scen, (int)b->out_units, out, st));
  HIP_TRY(hipMemcpyAsync(pred, out, (size_t)(n_scen * P * b->out_units) * sizeof(float), hipMemcpyDefault, st));
  HIP_TRY(hipStreamSynchronize(st));   // the caller's arrays (features in, predictions out) are done with
  return IGN_OK;
}

}  // namespace

extern "C" int ign_forward_scenarios(ign_batch* b, int32_t n_scen, const float* const* feat, int n_ents, float* pred) {
  if (!b || !pred) return fail(IGN_ERR_INVALID, "null argument");
  ign_plan* p = b->plan;
  int rc = check_pb(p, b);
  if (rc) return rc;
  if (n_scen < 1) return fail(IGN_ERR_INVALID, "forward scenarios: %d scenarios", n_scen);
  if (n_ents != (int)p->ents.size())
    return fail(IGN_ERR_INVALID, "forward scenarios: %d feature arrays for a plan of %d entities", n_ents, (int)p->ents.size());
  for (int e = 0; feat && e < n_ents; ++e)
    if (feat[e] && (p->ents[e].feature_total <= 0 || !b->d_feat[e]))
      return fail(IGN_ERR_INVALID, "forward scenarios: entity %d has no features", e);
  if ((rc = scen_check_scope(p, b, "forward scenarios"))) return rc;
  return forward_scenarios(p, b, n_scen, feat, pred);
}
