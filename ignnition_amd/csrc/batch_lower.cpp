// batch_lower.cpp — host-side lowering of a batch into the kernels' index tables (batch_lower.h).
//
// Reference behaviour restated here (generate_model.py = GM, auxilary_classes.py = AUX):
//  * per-graph dense padding semantics of the combine step:
//      lens = in-degree, Lmax = max(seq)+1 per graph and source,
//      source k's slots start after sources 0..k-1's Lmax           GM:477-543
//      interleave permutes slots through indices_<src>_to_<dst>    AUX:421-440, GM:507-519
//      sorted update consumes positions 0..final_len-1 (holes are
//      zero inputs, later positions dropped)                       AUX:767-796
//    These become per-destination step tables (CSR) built here on the host, once per batch.
// Errors the reference raises at run time (e.g. gather_nd(-1) when final_len = 0, scatter_nd
// with an out-of-range interleave index, an adjacency with no edges) are returned as
// IGN_ERR_INVALID with a message.
// Size limits no small input reaches: an entity of >= 2^29 rows ("too many rows"), a graph of
// >= 2^31 padded slots ("sequences too long"), an MP of >= 2^31 steps or 2^32 table rows ("MP too
// large"), a message network over >= 2^29 edges ("too many edges for a message network").

#include "batch_lower.h"

#include <atomic>
#include <numeric>

namespace ign {

void sort_order(hvec<int32_t>& order, const hvec<int64_t>& cnt) {
  const int64_t n = (int64_t)order.size();
  int64_t mx = 0;
  for (int32_t r : order) mx = std::max(mx, cnt[r]);
  if (mx > (int64_t)16 * n + 4096) {
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return cnt[x] > cnt[y]; });
    return;
  }
  hvec<int64_t> start(mx + 2, 0);   // bucket c holds count mx - c (descending)
  for (int32_t r : order) start[mx - cnt[r] + 1]++;
  for (int64_t c = 0; c <= mx; ++c) start[c + 1] += start[c];
  hvec<int32_t> out(n);
  for (int32_t r : order) out[start[mx - cnt[r]]++] = r;
  order.swap(out);
}

int lower_batch_shape(int E, int n_adj, int n_il, const std::vector<MPP>& mps, const ign_batch_desc* d,
                      BatchShape* b) {
  const int G = d->num_graphs;
  b->d = d;
  b->G = G;
  b->rows.assign(E, 0);
  b->row_off.assign(E, std::vector<int64_t>(G + 1, 0));
  for (int e = 0; e < E; ++e) {
    for (int g = 0; g < G; ++g) {
      int64_t n = d->num_nodes[(int64_t)g * E + e];
      if (n < 0) return fail(IGN_ERR_INVALID, "graph %d: negative num_ for entity %d", g, e);
      b->row_off[e][g + 1] = b->row_off[e][g] + n;
    }
    b->rows[e] = b->row_off[e][G];
  }
  b->halo.assign(E, 0);
  if (d->halo_rows) {
    // a partition holds only its own destinations: the attention softmax normalises over all of the
    // graph's destinations per position (AUX:327-336), and the sorted updates pad per graph
    // (GM:477-543).  Sum / convolution MPs, with or without message networks, are destination-local.
    for (auto& mp : mps)
      if (mp.aggr == IGN_AGGR_ATTENTION || mp.sorted)
        return fail(IGN_ERR_UNSUPPORTED, "edge-cut partitions support sum and convolution MPs only (attention "
                    "normalises over the whole graph, AUX:327-336; ordered updates pad per graph, GM:477-543)");
    for (int e = 0; e < E; ++e) {
      if (d->halo_rows[e] < 0) return fail(IGN_ERR_INVALID, "entity %d: negative halo_rows", e);
      b->halo[e] = d->halo_rows[e];
      if (b->halo[e] && G != 1) return fail(IGN_ERR_INVALID, "halo rows need num_graphs == 1 (one partition)");
    }
  }
  for (int e = 0; e < E; ++e)
    if (b->rows[e] + b->halo[e] >= (int64_t)IGN_ROW_MASK) return fail(IGN_ERR_UNSUPPORTED, "entity %d: too many rows", e);
  // edge offsets per adjacency
  b->eoff.assign(n_adj, hvec<int64_t>(G + 1, 0));
  for (int a = 0; a < n_adj; ++a)
    for (int g = 0; g < G; ++g) {
      int64_t n = d->adj_edges[(int64_t)g * n_adj + a];
      if (n < 0) return fail(IGN_ERR_INVALID, "negative edge count");
      b->eoff[a][g + 1] = b->eoff[a][g] + n;
    }
  b->asrc.resize(n_adj), b->adst.resize(n_adj), b->aseq.resize(n_adj), b->ilx.resize(n_il);
  if (d->index_bytes != 0 && d->index_bytes != 4 && d->index_bytes != 8)
    return fail(IGN_ERR_INVALID, "index_bytes %d (0 / 8: int64 index arrays, 4: int32)", (int)d->index_bytes);
  for (int a = 0; a < n_adj; ++a) {
    b->asrc[a] = IdxArr(d->adj_src[a], d->index_bytes);
    b->adst[a] = IdxArr(d->adj_dst[a], d->index_bytes);
    b->aseq[a] = IdxArr(d->adj_seq[a], d->index_bytes);
  }
  for (int i = 0; i < n_il; ++i) b->ilx[i] = IdxArr(d->interleave_idx[i], d->index_bytes);
  b->ioff.assign(n_il, hvec<int64_t>(G + 1, 0));
  for (int i = 0; i < n_il; ++i)
    for (int g = 0; g < G; ++g) b->ioff[i][g + 1] = b->ioff[i][g] + d->interleave_len[(int64_t)g * n_il + i];
  return IGN_OK;
}

// ---------------------------------------------------------------------------------------------
// lower_messages' lists for one (graph, source) of a plain MP (no interleave, attention or axis-2
// concat), T the desc's index type: false at the first index out of range, before any store for that
// message (the caller's checked loop then reports it; fl covers the graph's ndst > 0 rows only)
template <class T>
static bool plain_messages(const T* __restrict as, const T* __restrict ad, const T* __restrict aq, int64_t n,
                           int64_t nsrc, int64_t ndst, int64_t rd, int64_t rs, int64_t slot_off, uint32_t sb, bool net,
                           int64_t e0, hvec<int32_t>& mdst, hvec<int32_t>& mpos, hvec<uint32_t>& mcode,
                           int64_t* __restrict fl) {
  for (int64_t k = 0; k < n; ++k) {
    const int64_t si = as[k], di = ad[k];
    if ((uint64_t)si >= (uint64_t)nsrc || (uint64_t)di >= (uint64_t)ndst) return false;
    mdst.push_back((int32_t)(rd + di));
    mpos.push_back((int32_t)(slot_off + (int64_t)aq[k]));
    mcode.push_back(sb | (uint32_t)(net ? e0 + k : rs + si));
    fl[di] += 1;
  }
  return true;
}

int lower_messages(const MPP& mp, const BatchShape& sh, MsgLists* out) {
  const BatchShape* b = &sh;
  const ign_batch_desc* d = sh.d;
  const auto &eoff = sh.eoff, &ioff = sh.ioff;
  const auto &asrc = sh.asrc, &adst = sh.adst, &aseq = sh.aseq, &ilx = sh.ilx;
  const int G = sh.G, S = (int)mp.src.size(), dst = mp.dst;
  const int64_t ND = b->rows[dst];
  hvec<int32_t>& mdst = out->mdst;
  hvec<int32_t>& mpos = out->mpos;
  hvec<uint32_t>& mcode = out->mcode;
  int64_t tot = 0;
  for (int s = 0; s < S; ++s) tot += eoff[mp.src[s].adjacency][G];
  out->tot = tot;
  mdst.reserve(tot);
  mpos.reserve(tot);
  mcode.reserve(tot);
  hvec<int64_t>& flen = out->flen;
  flen.assign(ND, 0);
  for (int g = 0; g < G; ++g) {
    int64_t slot_off = 0;  // sum of Lmax of previous sources in this graph (GM:533)
    hvec<int64_t> ilflat;
    if (mp.aggr == IGN_AGGR_INTERLEAVE) {
      // tf.stack([indices_a, indices_b]) then reshape [-1,1] (GM:518, AUX:433)
      int64_t len0 = -1;
      for (int s = 0; s < S; ++s) {
        int il = mp.src[s].interleave;
        int64_t n = ioff[il][g + 1] - ioff[il][g];
        if (len0 >= 0 && n != len0)
          return fail(IGN_ERR_INVALID, "graph %d: interleave index lists have different lengths (%lld vs %lld;"
                      " tf.stack fails, GM:518)", g, (long long)len0, (long long)n);
        len0 = n;
        for (int64_t k = ioff[il][g]; k < ioff[il][g + 1]; ++k) ilflat.push_back(ilx[il][k]);
      }
    }
    int64_t total_slots = 0;
    hvec<int64_t> lmax(S, 0);
    for (int s = 0; s < S; ++s) {
      const int a = mp.src[s].adjacency;
      const int64_t e0 = eoff[a][g], e1 = eoff[a][g + 1];
      if (e1 == e0)
        return fail(IGN_ERR_INVALID, "graph %d: adjacency slot %d has no edges (the reference's scatter_nd shape"
                    " max(seq)+1 is undefined, GM:484-490)", g, a);
      int64_t mx = -1;
      for (int64_t k = e0; k < e1; ++k) {
        int64_t sq = aseq[a][k];
        if (sq < 0) return fail(IGN_ERR_INVALID, "graph %d: negative seq value", g);
        mx = std::max(mx, sq);
      }
      lmax[s] = mx + 1;
      total_slots += lmax[s];
    }
    if (total_slots >= INT32_MAX) return fail(IGN_ERR_UNSUPPORTED, "graph %d: sequences too long", g);
    if (mp.feature_concat) {   // tf.concat on axis 2 needs every source's [N, Lmax] to match
      for (int s = 1; s < S; ++s)
        if (lmax[s] != lmax[0])
          return fail(IGN_ERR_INVALID, "graph %d: concat on axis 2 of sequences of length %lld and %lld "
                      "(ConcatOp dimension mismatch, GM:503)", g, (long long)lmax[0], (long long)lmax[s]);
      total_slots = lmax[0];
    }
    if (mp.aggr == IGN_AGGR_INTERLEAVE && (int64_t)ilflat.size() != total_slots)
      return fail(IGN_ERR_INVALID, "graph %d: interleave indices cover %lld slots but the messages need %lld"
                  " (scatter_nd shape mismatch, AUX:435)", g, (long long)ilflat.size(), (long long)total_slots);
    for (int s = 0; s < S; ++s) {
      const int a = mp.src[s].adjacency;
      const int se = mp.src[s].entity;
      const int64_t e0 = eoff[a][g], e1 = eoff[a][g + 1];
      const int64_t nsrc = b->row_off[se][g + 1] - b->row_off[se][g] + b->halo[se];   // halo: G == 1
      const int64_t ndst = b->row_off[dst][g + 1] - b->row_off[dst][g];
      // attention: comb_seq of source s > 0 is seq + that source's own in-degree (GM:539-540)
      hvec<int64_t> lens_s;
      if (mp.aggr == IGN_AGGR_ATTENTION && s > 0) {
        lens_s.assign(ndst, 0);
        for (int64_t k = e0; k < e1; ++k) {
          const int64_t di = adst[a][k];
          if (di >= 0 && di < ndst) lens_s[di]++;
        }
      }
      if (mp.aggr != IGN_AGGR_INTERLEAVE && mp.aggr != IGN_AGGR_ATTENTION && !mp.feature_concat && ndst > 0) {
        // the common case (sum, ordered, convolution; no axis-2 concat): the loop below without its
        // per-message branches on the MP's kind, whose fields it reloaded on every message (the
        // stores may alias them), reading the desc's own index width.  An index out of range
        // reruns the checked loop, which reports the first one.  (A graph without destination rows
        // has no flen range to count into and only indices out of range: the checked loop at once.)
        const int64_t rd = b->row_off[dst][g], rs = b->row_off[se][g];
        const uint32_t sb = (uint32_t)s << IGN_SLOT_SHIFT;
        const bool net = !mp.nn[s].layers.empty();
        const bool ok = d->index_bytes == 4
            ? plain_messages(static_cast<const int32_t*>(asrc[a].p) + e0, static_cast<const int32_t*>(adst[a].p) + e0,
                             static_cast<const int32_t*>(aseq[a].p) + e0, e1 - e0, nsrc, ndst, rd, rs, slot_off, sb,
                             net, e0, mdst, mpos, mcode, flen.data() + rd)
            : plain_messages(d->adj_src[a] + e0, d->adj_dst[a] + e0, d->adj_seq[a] + e0, e1 - e0, nsrc, ndst, rd, rs,
                             slot_off, sb, net, e0, mdst, mpos, mcode, flen.data() + rd);
        if (ok) {
          slot_off += lmax[s];
          continue;
        }
      }
      for (int64_t k = e0; k < e1; ++k) {
        int64_t si = asrc[a][k], di = adst[a][k], sq = aseq[a][k];
        if (si < 0 || si >= nsrc) return fail(IGN_ERR_INVALID, "graph %d: src index %lld out of range [0,%lld)", g, (long long)si, (long long)nsrc);
        if (di < 0 || di >= ndst) return fail(IGN_ERR_INVALID, "graph %d: dst index %lld out of range [0,%lld)", g, (long long)di, (long long)ndst);
        int64_t pos = slot_off + sq;
        if (mp.aggr == IGN_AGGR_INTERLEAVE) {
          pos = ilflat[pos];
          if (pos < 0 || pos >= total_slots)
            return fail(IGN_ERR_INVALID, "graph %d: interleave index %lld outside [0,%lld) (scatter_nd, AUX:435)",
                        g, (long long)pos, (long long)total_slots);
        }
        if (mp.aggr == IGN_AGGR_ATTENTION) pos = sq + (s > 0 ? lens_s[di] : 0);
        if (mp.feature_concat) pos = sq;   // all sources share the positions (axis-2 concat)
        int64_t drow = b->row_off[dst][g] + di;
        mdst.push_back(drow);
        mpos.push_back(pos);
        // a message network's messages live per edge: the code addresses the edge (GM:440-475)
        const int64_t mrow = mp.nn[s].layers.empty() ? b->row_off[se][g] + si : k;
        mcode.push_back(((uint32_t)s << IGN_SLOT_SHIFT) | (uint32_t)mrow);
        // final_len = sum of lens over sources (GM:505/519/543); axis-2 concat keeps the first
        // source's lens (GM:503-505)
        if (!mp.feature_concat || s == 0) flen[drow] += 1;
      }
      slot_off += lmax[s];
    }
    if (mp.sorted) {
      // gather_nd(outputs, [d, final_len-1]) needs final_len <= sum of Lmax (AUX:793-795)
      int64_t max_flen = 0;
      for (int64_t r = b->row_off[dst][g]; r < b->row_off[dst][g + 1]; ++r) {
        if (flen[r] > total_slots)
          return fail(IGN_ERR_INVALID, "graph %d: destination row %lld has final_len %lld > %lld padded slots"
                      " (gather_nd out of range, AUX:793-795)", g, (long long)(r - b->row_off[dst][g]),
                      (long long)flen[r], (long long)total_slots);
        max_flen = std::max(max_flen, flen[r]);
      }
      // RNN(mask=tf.sequence_mask(final_len)) (AUX:785-790): the mask is max(final_len) wide, and
      // K.rnn unstacks it into a TensorList that its while loop reads at every one of the
      // total_slots time steps -> InvalidArgument at step max(final_len) when that is narrower
      // ("masked-RNN time length")
      if (b->row_off[dst][g + 1] > b->row_off[dst][g] && max_flen < total_slots)
        return fail(IGN_ERR_INVALID, "graph %d: sequence_mask(final_len) is %lld steps wide but the padded "
                    "sequence has %lld (K.rnn reads the mask TensorList past its end, AUX:785-790)", g,
                    (long long)max_flen, (long long)total_slots);
    }
  }
  return IGN_OK;
}

int lower_edge_rows(const MPP& mp, size_t mi, int s, const BatchShape& sh, hvec<int32_t>* es, hvec<int32_t>* ed) {
  const BatchShape* b = &sh;
  const MsgNN& nn = mp.nn[s];
  const int a = mp.src[s].adjacency, se = mp.src[s].entity, dst = mp.dst, G = sh.G;
  const auto& eoff = sh.eoff;
  const int64_t ne = eoff[a][G];
  if (ne >= (int64_t)IGN_ROW_MASK) return fail(IGN_ERR_UNSUPPORTED, "too many edges for a message network");
  es->resize(ne), ed->resize(ne);
  for (int g = 0; g < G; ++g)
    for (int64_t k = eoff[a][g]; k < eoff[a][g + 1]; ++k) {
      (*es)[k] = (int32_t)(b->row_off[se][g] + sh.asrc[a][k]);
      (*ed)[k] = (int32_t)(b->row_off[dst][g] + sh.adst[a][k]);
    }
  if (std::find(nn.inputs.begin(), nn.inputs.end(), (int)IGN_MSG_EDGE_PARAMS) != nn.inputs.end() &&
      (!sh.d->adj_params || !sh.d->adj_params[a]))
    return fail(IGN_ERR_INVALID, "message network of mp %zu reads edge_params but params_<adj> is missing", mi);
  return IGN_OK;
}

int64_t source_rows(const MPP& mp, int s, const BatchShape& sh) {
  const int se = mp.src[s].entity;
  return mp.nn[s].layers.empty() ? sh.rows[se] + sh.halo[se] : sh.eoff[mp.src[s].adjacency][sh.G];
}

int lower_ordered(const MPP& mp, int H, const BatchShape& sh, const MsgLists& ml, BuildMarks& bm, OrderedTables* out) {
  OrderedTables& mb = *out;
  const auto &mdst = ml.mdst, &mpos = ml.mpos;
  const auto& mcode = ml.mcode;
  const auto& flen = ml.flen;
  const int S = (int)mp.src.size();
  const int64_t ND = sh.rows[mp.dst];
  hvec<int32_t>& order = mb.order;
  order.resize(ND);
  std::iota(order.begin(), order.end(), 0);
  for (int64_t r = 0; r < ND; ++r)
    if (flen[r] == 0)   // AUX:793-795: gather_nd(outputs, [d, final_len-1]) with -1
      return fail(IGN_ERR_INVALID, "destination row %lld receives no message: the reference's sorted update"
                  " gathers position -1 (AUX:793-795)", (long long)r);
  sort_order(order, flen);
  bm.mark("sort");
  // combined projected table: source s occupies rows [src_off[s], src_off[s] + rows_s)
  int64_t trow = 0;
  for (int s = 0; s < S; ++s) {
    mb.src_off.push_back(trow);
    const int64_t rows_s = source_rows(mp, s, sh);
    mb.src_rows.push_back(rows_s);
    trow += rows_s;
  }
  mb.zero_row = trow;
  auto table_row = [&](uint32_t code) -> int64_t {
    return mb.src_off[code >> IGN_SLOT_SHIFT] + (code & IGN_ROW_MASK);
  };
  // Step t of the destination at sorted position i is slot step_ptr[i] + t.  A slot holds its
  // message's table row, the zero row (a hole), or a pre-summed "multi" row when several
  // messages share the position (scatter_nd adds them); messages at positions >= final_len
  // are dropped (the masked RNN never reads them).  Multi rows are numbered in slot order and
  // list their messages in message order.  maxL + 8 trailing zero-row slots: the kernels read
  // codes past a row's end unconditionally.
  hvec<int32_t>&len = mb.len, &step_ptr = mb.step_ptr, &multi_ptr = mb.multi_ptr;
  len.resize(ND), step_ptr.resize(ND), multi_ptr.assign(1, 0);
  hvec<int32_t> where(ND);
  int64_t steps = 0, maxL = 0;
  for (int64_t i = 0; i < ND; ++i) {
    const int64_t r = order[i];
    where[r] = (int32_t)i;
    len[i] = (int32_t)flen[r];
    step_ptr[i] = (int32_t)steps;
    maxL = std::max(maxL, flen[r]);
    steps += flen[r];
  }
  if (steps >= INT32_MAX) return fail(IGN_ERR_UNSUPPORTED, "MP too large");
  hvec<uint32_t>& scode = mb.step_code;
  scode.assign((size_t)(steps + maxL + 8), (uint32_t)mb.zero_row);
  hvec<int32_t> slot_of(mdst.size(), -1), scount(steps, 0);
  int64_t n_msgs = 0;
  for (size_t k = 0; k < mdst.size(); ++k) {
    const int64_t r = mdst[k];
    if (mpos[k] >= flen[r]) continue;
    const int64_t slot = step_ptr[where[r]] + mpos[k];
    slot_of[k] = (int32_t)slot;
    if (++scount[slot] == 1) scode[slot] = (uint32_t)table_row(mcode[k]);
    ++n_msgs;
  }
  hvec<uint32_t>& multi_rows = mb.multi_rows;
  hvec<int32_t> multi_of(steps, -1);
  for (int64_t slot = 0; slot < steps; ++slot)
    if (scount[slot] > 1) {
      multi_of[slot] = (int32_t)mb.n_multi;
      scode[slot] = (uint32_t)(mb.zero_row + 1 + mb.n_multi);
      multi_ptr.push_back(multi_ptr.back() + scount[slot]);
      mb.n_multi++;
    }
  if (mb.n_multi) {
    multi_rows.resize(multi_ptr.back());
    hvec<int32_t> fill(multi_ptr.begin(), multi_ptr.end() - 1);
    for (size_t k = 0; k < mdst.size(); ++k)
      if (slot_of[k] >= 0 && multi_of[slot_of[k]] >= 0)
        multi_rows[fill[multi_of[slot_of[k]]]++] = (uint32_t)table_row(mcode[k]);
  }
  bm.mark("slots");
  for (int64_t i = 0; i < ND; i += 16) mb.wave_steps += len[i];   // sorted: a tile's first row is its longest
  {   // the ordered update's tile headers: one 16-B load per position, no dependent code load
    const int64_t NDp = (ND + 15) / 16 * 16;
    hvec<int32_t>& hdr = mb.hdr;
    hdr.resize((size_t)(4 * NDp));
    for (int64_t i = 0; i < NDp; ++i) {
      const bool v = i < ND;
      hdr[4 * i] = v ? order[i] : 0;
      hdr[4 * i + 1] = v ? len[i] : 0;
      hdr[4 * i + 2] = v ? step_ptr[i] : (int32_t)steps;
      hdr[4 * i + 3] = (int32_t)scode[v ? step_ptr[i] : steps];
    }
  }
  bm.mark("headers");
  if (mb.zero_row + 1 + mb.n_multi >= (int64_t)UINT32_MAX) return fail(IGN_ERR_UNSUPPORTED, "MP too large");
  mb.n_steps = steps;
  mb.n_msgs = n_msgs;
  // per launch of the recurrence: h.U + gates per step; one projected row (3H floats) per step
  // FLOPs executed (fp32-equivalent): h.U + gates per step (x.W is hoisted into project);
  // bytes per SURVEY §8d, B_stage = E (4 + 4H) + 2 N_d 4H + 4 (N_d + 1): one message row and
  // code per step, the state read and written once per destination
  mb.flops = (double)steps * (2.0 * H * 3 * H + 14.0 * H);
  mb.bytes = (double)steps * (4.0 * H + 4) + (double)ND * 8.0 * H + 4.0 * (ND + 1);
  return IGN_OK;
}

void lower_sum_csr(const MPP& mp, const BatchShape& sh, const MsgLists& ml, BuildMarks& bm, SumCsr* out) {
  const BatchShape* b = &sh;
  SumCsr& mb = *out;
  const auto& mdst = ml.mdst;
  const auto& mcode = ml.mcode;
  const int64_t ND = sh.rows[mp.dst];
  hvec<int32_t>& order = mb.order;
  order.resize(ND);
  std::iota(order.begin(), order.end(), 0);
  sort_order(order, ml.flen);
  // edge-cut partitions: destinations reading a halo row go last (they wait for the exchange)
  // (a message network's codes address edges, and its per-edge pass reads every source row
  // before any destination runs: no interior destinations then)
  bool nets = false;
  for (auto& nn : mp.nn) nets = nets || !nn.layers.empty();
  bool halo = false;
  for (auto& sd : mp.src) halo = halo || b->halo[sd.entity] > 0;
  mb.halo = halo;
  hvec<char> bnd(ND, nets && halo ? 1 : 0);
  for (size_t k = 0; k < mdst.size() && !nets; ++k) {
    const uint32_t c = mcode[k];
    const int se = mp.src[c >> IGN_SLOT_SHIFT].entity;
    if ((int64_t)(c & IGN_ROW_MASK) >= b->rows[se]) bnd[mdst[k]] = 1;
  }
  std::stable_partition(order.begin(), order.end(), [&](int32_t r) { return !bnd[r]; });
  bm.mark("sort");
  mb.n_interior = std::count(bnd.begin(), bnd.end(), 0);
  hvec<int32_t> where(ND);
  for (int64_t i = 0; i < ND; ++i) where[order[i]] = (int32_t)i;
  hvec<int32_t>& ptr = mb.ptr;
  ptr.assign(ND + 1, 0);
  for (size_t k = 0; k < mdst.size(); ++k) ptr[where[mdst[k]] + 1]++;
  for (int64_t i = 0; i < ND; ++i) ptr[i + 1] += ptr[i];
  hvec<uint32_t>& msrc = mb.msrc;
  msrc.resize(mdst.size());
  hvec<int32_t>& csr_pos = mb.csr_pos;   // message -> CSR slot
  csr_pos.resize(mp.aggr == IGN_AGGR_ATTENTION ? mdst.size() : 0);
  {
    hvec<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (size_t k = 0; k < mdst.size(); ++k) {
      const int32_t q = fill[where[mdst[k]]]++;
      if (!csr_pos.empty()) csr_pos[k] = q;
      msrc[q] = mcode[k];
    }
  }
}

void lower_attention(const MPP& mp, const BatchShape& sh, const MsgLists& ml, const SumCsr& csr, AttnTables* out) {
  const BatchShape* b = &sh;
  AttnTables& mb = *out;
  const auto &mdst = ml.mdst, &mpos = ml.mpos;
  const auto& csr_pos = csr.csr_pos;
  const int G = sh.G, dst = mp.dst;
  const int64_t ND = sh.rows[dst];
  // dense (destination, position) cells of the scatter_nd (AUX:327-331); duplicates share one
  // cell.  Groups = (graph, position): the softmax runs over a graph's destinations (AUX:336)
  hvec<int> gof(ND);
  for (int g = 0; g < G; ++g)
    for (int64_t r = b->row_off[dst][g]; r < b->row_off[dst][g + 1]; ++r) gof[r] = g;
  hvec<int64_t> gmax(G, 0);
  for (size_t k = 0; k < mdst.size(); ++k) gmax[gof[mdst[k]]] = std::max<int64_t>(gmax[gof[mdst[k]]], mpos[k] + 1);
  hvec<int64_t> gbase(G + 1, 0);   // group index base per graph
  for (int g = 0; g < G; ++g) gbase[g + 1] = gbase[g] + gmax[g];
  hvec<size_t> ord(mdst.size());
  std::iota(ord.begin(), ord.end(), 0);
  std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) {
    const int64_t gx = gbase[gof[mdst[x]]] + mpos[x], gy = gbase[gof[mdst[y]]] + mpos[y];
    return gx != gy ? gx < gy : mdst[x] < mdst[y];
  });
  hvec<int32_t>&group_ptr = mb.group_ptr, &group_empty = mb.group_empty, &cell_dst = mb.cell_dst,
  &cell_ptr = mb.cell_ptr, &cell_msgs = mb.cell_msgs;
  group_ptr.assign(gbase[G] + 1, 0), group_empty.assign(gbase[G], 0), cell_ptr.assign(1, 0);
  for (size_t q = 0; q < ord.size();) {
    const size_t k = ord[q];
    const int64_t grp = gbase[gof[mdst[k]]] + mpos[k];
    size_t q2 = q;
    while (q2 < ord.size() && mdst[ord[q2]] == mdst[k] && mpos[ord[q2]] == mpos[k]) cell_msgs.push_back(csr_pos[ord[q2++]]);
    cell_dst.push_back((int32_t)mdst[k]);
    cell_ptr.push_back((int32_t)cell_msgs.size());
    group_ptr[grp + 1]++;
    q = q2;
  }
  for (int64_t q = 0; q < gbase[G]; ++q) group_ptr[q + 1] += group_ptr[q];
  for (int g = 0; g < G; ++g)
    for (int64_t pq = 0; pq < gmax[g]; ++pq) {
      const int64_t grp = gbase[g] + pq;
      group_empty[grp] = (int32_t)((b->row_off[dst][g + 1] - b->row_off[dst][g]) - (group_ptr[grp + 1] - group_ptr[grp]));
    }
  mb.n_groups = gbase[G];
  mb.n_cells = (int64_t)cell_dst.size();
}

int lower_sum_agg(const MPP& mp, size_t mi, int sum_window, const BatchShape& sh, const MsgLists& ml,
                  const SumCsr& csr, SumAgg* out) {
  const BatchShape* b = &sh;
  SumAgg& mb = *out;
  const auto& mdst = ml.mdst;
  const auto& mcode = ml.mcode;
  const auto& flen = ml.flen;
  const auto &order = csr.order, &ptr = csr.ptr;
  const auto& msrc = csr.msrc;
  const bool halo = csr.halo;
  const int G = sh.G, S = (int)mp.src.size(), dst = mp.dst, DIN = mp.din;
  const int64_t ND = sh.rows[dst];
  // windowed sum: one workgroup per (graph, chunk of <= 256 destinations by message count), the
  // destination's source rows ascending (a fixed summation order), LDS windows over the graph's
  // source rows; the GRU step then reads x through an identity CSR over the same order
  // (small graphs only: a workgroup walks all of its graph's windows, at most 4 of them)
  int64_t max_src_rows = 0;
  if (S == 1)
    for (int g = 0; g < G; ++g)
      max_src_rows = std::max(max_src_rows, b->row_off[mp.src[0].entity][g + 1] - b->row_off[mp.src[0].entity][g]);
  const int64_t win_rows = DIN == 16 ? 2400 : DIN == 32 ? 1200 : 600;   // sum_win_kernel's windows
  // IGN_SUM_WINDOW: -1 auto, 0 off below 128 messages (one lane group per destination walks its
  // messages in the GRU-step kernel), 1 windowed, 2 segmented for every destination.  Auto takes the segmented
  // sum (one wave per destination) for the destinations whose lane walk would be a long dependent
  // chain: >= 64 messages (seg_min_messages; Q-size's path -> node update, ~140 per node: 4.36-4.39
  // ms/step against 5.19 windowed and 5.51 lane-walk in round 4).  The rule reads each
  // destination's own in-degree, a property of its graph, so a graph's predictions stay bitwise
  // the same alone and in any batch (the two kernels add a destination's messages in different
  // orders), and the graph-resident forward takes the same order per row (resident.hip B1).
  const bool window = sum_window == 1;
  int64_t n_seg = 0;   // order is sorted by message count, descending: the segmented rows lead
  if (sum_window == 0 && ND > 0 && ptr[1] - ptr[0] >= kSegMinMessages)   // (order: by count, descending)
    return fail(IGN_ERR_UNSUPPORTED, "IGN_SUM_WINDOW=0 (every sum a lane walk): mp %d has a destination of %lld "
                "messages; a float32 chain of >= %lld terms leaves the fp32 class, so this switch is for batches "
                "below that", (int)mi, (long long)(ptr[1] - ptr[0]), (long long)kSegMinMessages);
  if (!window && !halo)
    while (n_seg < ND && ptr[n_seg + 1] - ptr[n_seg] >= seg_min_messages(sum_window)) ++n_seg;
  const bool seg = n_seg > 0;
  const bool plain_sum = mp.aggr == IGN_AGGR_SUM && S == 1 && mp.nn[0].layers.empty() &&
                         b->halo[mp.src[0].entity] == 0 && (DIN == 16 || DIN == 32 || DIN == 64);
  if (window && plain_sum && max_src_rows <= 4 * win_rows) {
    const int se = mp.src[0].entity;
    hvec<int64_t> dstart(ND + 1, 0);
    for (size_t k = 0; k < mdst.size(); ++k) dstart[mdst[k] + 1]++;
    for (int64_t r = 0; r < ND; ++r) dstart[r + 1] += dstart[r];
    hvec<int32_t> rows_by(mdst.size());
    {
      hvec<int64_t> fill(dstart.begin(), dstart.end() - 1);
      for (size_t k = 0; k < mdst.size(); ++k) rows_by[fill[mdst[k]]++] = (int32_t)(mcode[k] & IGN_ROW_MASK);
    }
    for (int64_t r = 0; r < ND; ++r) std::sort(rows_by.begin() + dstart[r], rows_by.begin() + dstart[r + 1]);
    hvec<int64_t>& wg = mb.wg;
    hvec<int32_t>&wdst = mb.wdst, &wptr = mb.wptr, &wsrc = mb.wsrc;
    wptr.assign(1, 0);
    wdst.reserve(ND);
    wsrc.reserve(mdst.size());
    for (int g = 0; g < G; ++g) {
      hvec<int32_t> ds;
      for (int64_t r = b->row_off[dst][g]; r < b->row_off[dst][g + 1]; ++r) ds.push_back((int32_t)r);
      std::stable_sort(ds.begin(), ds.end(), [&](int32_t x, int32_t y) { return flen[x] > flen[y]; });
      for (size_t c0 = 0; c0 < ds.size(); c0 += 256) {
        const size_t c1 = std::min(ds.size(), c0 + 256);
        wg.push_back((int64_t)wdst.size());
        wg.push_back((int64_t)(wdst.size() + (c1 - c0)));
        wg.push_back(b->row_off[se][g]);
        wg.push_back(b->row_off[se][g + 1]);
        for (size_t q = c0; q < c1; ++q) {
          const int32_t r = ds[q];
          wdst.push_back(r);
          wsrc.insert(wsrc.end(), rows_by.begin() + dstart[r], rows_by.begin() + dstart[r + 1]);
          wptr.push_back((int32_t)wsrc.size());
        }
      }
    }
    hvec<int32_t>& id_ptr = mb.id_ptr;
    hvec<uint32_t>& id_src = mb.id_src;
    id_ptr.resize(ND + 1), id_src.resize(ND);
    for (int64_t i = 0; i <= ND; ++i) id_ptr[i] = (int32_t)i;
    for (int64_t i = 0; i < ND; ++i) id_src[i] = (uint32_t)order[i];   // slot 0: the x table
    mb.window = true;
    mb.n_win_wg = (int64_t)wg.size() / 4;
  } else if (seg && plain_sum) {
    // segmented sum (sum_seg_kernel over the MP's own CSR, one wave per destination) for order
    // positions [0, n_seg), then the GRU step over a mixed CSR: those positions read their x
    // from the xsum table (one message, slot 1; the lane walk adds it to zero exactly), the
    // others their own messages (slot 0)
    hvec<int32_t>& id_ptr = mb.id_ptr;
    hvec<uint32_t>& id_src = mb.id_src;
    id_ptr.assign(ND + 1, 0);
    id_src.reserve((size_t)(n_seg + (ptr[ND] - ptr[n_seg])));
    for (int64_t i = 0; i < ND; ++i) {
      if (i < n_seg) id_src.push_back((1u << IGN_SLOT_SHIFT) | (uint32_t)order[i]);
      else id_src.insert(id_src.end(), msrc.begin() + ptr[i], msrc.begin() + ptr[i + 1]);
      id_ptr[i + 1] = (int32_t)id_src.size();
    }
    mb.seg = true;
    mb.n_seg = n_seg;
  }
  return IGN_OK;
}

// ---------------------------------------------------------------------------------------------
// dynamic LDS of one graph in a form: union-row states and projected table always; the sum MPs' CSR
// rows unless CL is off; the path states and step codes in the all-LDS form
static size_t resident_lds_bytes(const ResidentParams& rp, int64_t paths, int64_t urows, int64_t msgs, int64_t codes,
                                 int form) {
  const size_t order = (size_t)((urows + 1) & ~int64_t(1)) * sizeof(uint16_t);   // the row order, padded
  size_t b = (size_t)(urows * rp.state_stride + (urows + 1) * rp.table_stride) * sizeof(float) +
             (size_t)(urows + 1) * sizeof(int32_t) + order;
  if (form != kResPathCsrGlobal) b += (size_t)msgs * sizeof(uint16_t);
  if (form == kResAllLds) b += (size_t)paths * rp.state_stride * sizeof(float) + (size_t)codes * sizeof(uint16_t);
  return b;
}

void lower_resident(const ResidentParams& sh, int K, const BatchRows& bb, const ResOrderedIn& ma,
                    const std::vector<ResSumIn>& sums, ResidentTables* out) {
  const BatchRows* b = &bb;
  out->eligible = false;
  const int path = sh.path, S = sh.n_src;
  if (b->halo[path] || ma.n_multi || (int)ma.src_off.size() != S) return;
  for (int s = 0; s < S; ++s)
    if (b->halo[sh.src_ent[s]]) return;
  // a workgroup's "graph" is a group of K consecutive graphs of the batch (round 6, IGN_RES_GROUP):
  // their disjoint union is one graph to the kernel (concatenated local rows, one tile counter, one
  // set of union-row tiles), so small graphs fill the 16 waves -- GEANT2's 35 path tiles and 5
  // union-row tiles per graph leave most waves idle in phase A's tail and in phase B.  Every row is
  // computed as before (tiles of paths sorted by length across the group: the scale caveat above)
  const int G = (b->G + K - 1) / K;
  std::vector<int64_t>& po_g = out->path_off;
  std::vector<int64_t>* so_g = out->src_off;
  po_g.resize(G + 1);
  for (int k = 0; k <= G; ++k) po_g[k] = b->row_off[path][std::min(k * K, b->G)];
  for (int s = 0; s < S; ++s) {
    so_g[s].resize(G + 1);
    for (int k = 0; k <= G; ++k) so_g[s][k] = b->row_off[sh.src_ent[s]][std::min(k * K, b->G)];
  }
  const auto& po = po_g;
  const std::vector<int64_t>* so[kResMaxSrc] = {&so_g[0], S > 1 ? &so_g[1] : nullptr};
  auto Ls = [&](int s, int g) -> int64_t { return s < S ? (*so[s])[g + 1] - (*so[s])[g] : 0; };
  // union rows: per graph, source entity 0's rows, then entity 1's
  std::vector<int64_t>& uo = out->urow_off;
  uo.assign(G + 1, 0);
  for (int g = 0; g < G; ++g) {
    uo[g + 1] = uo[g] + Ls(0, g) + Ls(1, g);
    if (po[g + 1] - po[g] > 65535 || uo[g + 1] - uo[g] > 65535) return;   // local rows are 16-bit
    if ((Ls(0, g) + 15) / 16 + (Ls(1, g) + 15) / 16 > sh.max_tiles) return;   // B2/B3: two tiles per wave
  }
  // the graph of every row (rows are graph-contiguous)
  auto graph_of = [&](const std::vector<int64_t>& off, int64_t r) {
    return (int)(std::upper_bound(off.begin(), off.end(), r) - off.begin()) - 1;
  };
  auto urow = [&](int s, int g, int64_t row) { return uo[g] + (s ? Ls(0, g) : 0) + (row - (*so[s])[g]); };
  // the sum MPs: each graph's CSR by local union row, its messages in the MP's order (local path rows)
  hvec<int32_t>&lmsg_ptr = out->lmsg_ptr, &lmsg_off = out->lmsg_off;
  lmsg_ptr.assign((size_t)(uo[G] + G), 0), lmsg_off.assign(G + 1, 0);
  std::vector<int64_t> nmsg(G, 0);
  for (int s = 0; s < S; ++s) {
    const ResSumIn& ms = sums[s];
    for (int64_t q = 0; q < (int64_t)ms.h_order.size(); ++q) {
      const int64_t row = ms.h_order[q];
      const int g = graph_of(*so[s], row);
      const int32_t cnt = ms.h_msg_ptr[q + 1] - ms.h_msg_ptr[q];
      lmsg_ptr[urow(s, g, row) + g + 1] = cnt;   // counts, prefix-summed below
      nmsg[g] += cnt;
    }
  }
  const int64_t seg_min = seg_min_messages(sh.sum_window);
  hvec<uint16_t>& lorder = out->lorder;
  lorder.resize(std::max<int64_t>(uo[G], 1));
  hvec<int32_t>& lnseg = out->lnseg;
  lnseg.assign(G, 0);
  int64_t seg_rows = 0;
  for (int g = 0; g < G; ++g) {
    lmsg_off[g + 1] = lmsg_off[g] + (int32_t)nmsg[g];
    int32_t* cp = lmsg_ptr.data() + uo[g] + g;
    const int64_t U = uo[g + 1] - uo[g];
    // its local rows by message count, descending (stable): the rows of >= seg_min messages first
    // (the segmented sums), then the lane walks, long chains first
    std::vector<int32_t> ord(U);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return cp[x + 1] > cp[y + 1]; });
    for (int64_t r = 0; r < U; ++r) {
      lorder[uo[g] + r] = (uint16_t)ord[r];
      if (cp[ord[r] + 1] >= seg_min) lnseg[g]++;
    }
    seg_rows += lnseg[g];
    for (int64_t r = 0; r < U; ++r) cp[r + 1] += cp[r];
  }
  hvec<uint16_t>& lmsg_src = out->lmsg_src;
  lmsg_src.resize(std::max<int32_t>(lmsg_off[G], 1));
  for (int s = 0; s < S; ++s) {
    const ResSumIn& ms = sums[s];
    for (int64_t q = 0; q < (int64_t)ms.h_order.size(); ++q) {
      const int64_t row = ms.h_order[q];
      const int g = graph_of(*so[s], row);
      int32_t pos = lmsg_off[g] + lmsg_ptr[urow(s, g, row) + g];
      for (int32_t m = ms.h_msg_ptr[q]; m < ms.h_msg_ptr[q + 1]; ++m) {
        const int64_t pr = (int64_t)(ms.h_msg_src[m] & IGN_ROW_MASK) - po[g];
        if ((ms.h_msg_src[m] >> IGN_SLOT_SHIFT) != 0 || pr < 0 || pr >= po[g + 1] - po[g]) return;
        lmsg_src[pos++] = (uint16_t)pr;
      }
    }
  }
  // ordered MP: each graph's positions in the batch's length-sorted order (stable, so still sorted
  // by length, descending), padded to whole tiles; their step codes as local union rows (U_g: the
  // hole), then max_len + 8 hole codes (the tile loop reads codes past a row's end)
  // (positions by graph: a counting sort keyed by a row -> graph table, the batch order kept)
  const int64_t ND = (int64_t)ma.h_order.size();
  hvec<int32_t> pstart(G + 1, 0), plist(std::max<int64_t>(ND, 1));
  {
    hvec<int32_t> gid(std::max<int64_t>(po[G], 1));
    for (int g = 0; g < G; ++g)
      for (int64_t r = po[g]; r < po[g + 1]; ++r) gid[r] = g;
    for (int64_t i = 0; i < ND; ++i) pstart[gid[ma.h_order[i]] + 1]++;
    for (int g = 0; g < G; ++g) pstart[g + 1] += pstart[g];
    hvec<int32_t> fill(pstart.begin(), pstart.end() - 1);
    for (int64_t i = 0; i < ND; ++i) plist[fill[gid[ma.h_order[i]]]++] = (int32_t)i;
  }
  // two passes over the graphs, the second on IGN_BUILD_THREADS threads (the tables are ~10^7
  // entries for 512 synth50 graphs, ~20 ms on one builder thread): each graph's sizes, their
  // prefix sums, then every graph fills its own ranges
  std::vector<int64_t> npad(G), ncode(G), maxl_g(G, 0);
  hvec<int32_t>&ptile_off = out->ptile_off, &lcode_off = out->lcode_off;
  ptile_off.assign(G + 1, 0), lcode_off.assign(G + 1, 0);
  double tile_steps = 0;
  for (int g = 0; g < G; ++g) {
    const int64_t n = pstart[g + 1] - pstart[g];
    npad[g] = (n + 15) / 16 * 16;
    int64_t codes = 0, maxl = 0;
    for (int64_t k = pstart[g]; k < pstart[g + 1]; ++k) {
      const int32_t len = ma.h_len[plist[k]];
      codes += len;
      maxl = std::max<int64_t>(maxl, len);
    }
    for (int64_t k = pstart[g]; k < pstart[g + 1]; k += 16) tile_steps += ma.h_len[plist[k]];   // a tile's first row is its longest
    maxl_g[g] = maxl;
    ncode[g] = codes + maxl + 8;
    ptile_off[g + 1] = ptile_off[g] + (int32_t)npad[g];
    if ((int64_t)lcode_off[g] + ncode[g] >= INT32_MAX) return;
    lcode_off[g + 1] = lcode_off[g] + (int32_t)ncode[g];
  }
  hvec<int32_t>&hdr = out->hdr, &hsb = out->hsb;
  hdr.resize((size_t)4 * ptile_off[G]), hsb.resize((size_t)ptile_off[G]);
  hvec<uint16_t>& lcode = out->lcode;
  lcode.resize((size_t)lcode_off[G]);
  std::atomic<bool> foreign{false};   // a code of another graph's row or a multi-message row: not resident
  parallel_ranges(G, 16, [&](int64_t g0, int64_t g1) {
    for (int64_t g = g0; g < g1 && !foreign.load(std::memory_order_relaxed); ++g) {
      const int64_t U = uo[g + 1] - uo[g];
      int32_t* h = hdr.data() + (size_t)4 * ptile_off[g];
      int32_t* hs = hsb.data() + ptile_off[g];
      uint16_t* lc = lcode.data() + lcode_off[g];
      int32_t c = 0;   // the graph's next local code
      for (int64_t k = pstart[g]; k < pstart[g + 1]; ++k) {
        const int64_t i = plist[k];
        const int32_t len = ma.h_len[i], sp = ma.h_step_ptr[i];
        *h++ = (int32_t)(ma.h_order[i] - po[g]);
        *h++ = len;
        *hs++ = sp + (int32_t)i;   // the training forward's hs_save rows of position i
        *h++ = c;
        const int32_t c_first = c;
        for (int32_t t = 0; t < len; ++t) {
          const uint32_t cd = ma.h_step_code[sp + t];
          uint16_t code = (uint16_t)U;   // the zero row: a hole
          if (cd < (uint32_t)ma.zero_row) {
            const int s = S > 1 && (int64_t)cd >= ma.src_off[1] ? 1 : 0;
            const int64_t lr = (int64_t)cd - ma.src_off[s] - (*so[s])[g];
            if (lr < 0 || lr >= Ls(s, (int)g)) { foreign = true; return; }
            code = (uint16_t)((s ? Ls(0, (int)g) : 0) + lr);
          } else if (cd != (uint32_t)ma.zero_row) {
            foreign = true;   // a multi-message row (n_multi == 0: unreachable)
            return;
          }
          lc[c++] = code;
        }
        *h++ = len > 0 ? lc[c_first] : (int32_t)U;
      }
      const int32_t pad = c;
      for (int64_t q = 0; q < maxl_g[g] + 8; ++q) lc[c++] = (uint16_t)U;
      for (int64_t k = pstart[g + 1] - pstart[g]; k < npad[g]; ++k) {   // padding: row -1, length 0, hole codes, hs_save's pad row (unwritten)
        *hs++ = (int32_t)(ma.n_steps + ND);
        *h++ = -1;
        *h++ = 0;
        *h++ = pad;
        *h++ = (int32_t)U;
      }
    }
  });
  if (foreign) return;
  size_t* lds = out->lds;
  lds[0] = lds[1] = lds[2] = 0;
  for (int g = 0; g < G; ++g)
    for (int f = 0; f < 3; ++f)
      lds[f] = std::max(lds[f], resident_lds_bytes(sh, po[g + 1] - po[g], uo[g + 1] - uo[g], nmsg[g], ncode[g], f));
  // the workgroups' graphs, longest first (round 6): a launch of more graphs than CUs -- or the second
  // of two sub-batch launches, whose workgroups take the CUs the first one frees -- is a list
  // schedule in workgroup order, so longest-first is LPT.  The estimate, in cycles of one workgroup:
  // phase A's tile-steps over 4 SIMDs at ~1 300 cycles each, phase B's messages at ~6
  hvec<int32_t>& gorder = out->gorder;
  gorder.resize(G);
  {
    std::vector<double> cost(G, 0.0);
    for (int g = 0; g < G; ++g) {
      double ts = 0;
      for (int64_t k = pstart[g]; k < pstart[g + 1]; k += 16) ts += ma.h_len[plist[k]];
      cost[g] = ts * 325.0 + (double)nmsg[g] * 6.0;
    }
    std::iota(gorder.begin(), gorder.end(), 0);
    std::stable_sort(gorder.begin(), gorder.end(), [&](int32_t x, int32_t y) { return cost[x] > cost[y]; });
  }
  // every state in LDS where the largest graph's fit, else the path states in global memory, else
  // also the sum MPs' CSR
  int form = kResAllLds;
  if (lds[0] > sh.max_dyn_lds || sh.force_path_global) {
    if (!sh.path_global_ok) return;
    form = lds[1] <= sh.max_dyn_lds ? kResPathGlobal : kResPathCsrGlobal;
    if (lds[form] > sh.max_dyn_lds) return;
  }
  // the training forward's form: path states in global memory always (their versions)
  out->train_form = lds[1] <= sh.max_dyn_lds ? kResPathGlobal : kResPathCsrGlobal;
  out->form = form;
  out->G = G;
  out->K = K;
  // the cost model of one launch (ign_batch_resident_info): source s's sum MP runs Ts[s] times, T
  // less the last iteration's update where it is dead
  double utiles_s[kResMaxSrc] = {0, 0}, utiles = 0, ptiles = 0;
  for (int g = 0; g < G; ++g) {
    for (int s = 0; s < S; ++s) utiles_s[s] += (double)((Ls(s, g) + 15) / 16);
    ptiles += (double)((uo[g + 1] - uo[g] + 15) / 16);
  }
  for (int s = 0; s < S; ++s) utiles += utiles_s[s];
  const int64_t P = b->rows[path], Urows = uo[G];
  auto cost = [&](const bool* dead, ign_resident_info_t& ri) {
    ri = ign_resident_info_t{};
    ri.active = 1;
    ri.form = form;
    ri.lds_bytes = (int64_t)lds[form];
    ri.tile_steps = (int64_t)(tile_steps * sh.T);
    ri.seg_rows = seg_rows;
    ri.messages = lmsg_off[G];
    ri.union_tiles = (int64_t)utiles;
    // compulsory: the features, tile headers, step codes and the sum CSR read once, the final states
    // written once
    double feat = 4.0 * P * sh.feature_total[path];
    for (int s = 0; s < S; ++s) feat += 4.0 * b->rows[sh.src_ent[s]] * sh.feature_total[sh.src_ent[s]];
    ri.bytes_compulsory = feat + 4.0 * hdr.size() + 2.0 * (double)lcode.size() + 4.0 * lmsg_ptr.size() +
                          2.0 * lmsg_src.size() + 4.0 * 32 * (P + Urows);
    // global-path forms: every iteration moves each path row once in and out of the ordered update and
    // once per message into the sums (rows of 128 B) and reads the step codes again; the CSR-global
    // form also reads the message rows every iteration.  SURVEY §8(d): B_stage of every MP
    // (MPB::bytes), as often as it runs; the MPs' FLOPs likewise, plus the ordered MP's input
    // projection of every union row (T times: before iteration 0, then after every update but the last)
    double msg_trips = 0, stage = sh.T * ma.bytes, mflops = sh.T * ma.flops, step_tiles = 0;
    for (int s = 0; s < S; ++s) {
      const int Ts = sh.T - (dead[s] ? 1 : 0);
      msg_trips += Ts * (double)sums[s].h_msg_src.size();
      stage += Ts * sums[s].bytes;
      mflops += Ts * sums[s].flops;
      step_tiles += Ts * utiles_s[s];
    }
    if (form != kResAllLds)
      ri.bytes_roundtrip = 128.0 * (sh.T * 2.0 * P + msg_trips) + sh.T * 2.0 * (double)lcode.size();
    if (form == kResPathCsrGlobal) ri.bytes_roundtrip += 2.0 * msg_trips;
    ri.bytes_stage = stage;
    ri.flops = mflops + sh.T * 2.0 * Urows * 32 * 96;
    // the matrix pipe: phase A's split-fp16 h.U (3 products x 3 gates x 2 tiles per tile-step), the
    // split-bf16 GRU step (2 x 36 per tile), the projection (3 gates x 2 x 6, T - 1 times), all
    // 16x16x32; iteration 0's projection on f32 MFMA (3 gates x 2 tiles x 8 k-steps per union tile;
    // the projection's tiles straddle the entities, ceil(U / 16) per graph)
    ri.mfma_bf16 = (sh.T * tile_steps * 18.0 + step_tiles * 72.0 + (sh.T - 1) * utiles * 36.0) * kMfmaBf16Flops;
    ri.mfma_f32 = ptiles * 48.0 * kMfmaF32Flops;
    ri.workgroups = G;
    ri.graphs_per_workgroup = K;
  };
  const bool none[kResMaxSrc] = {false, false};
  cost(sh.dead_last, out->info);
  cost(none, out->info_full);
  out->eligible = true;
}

}  // namespace ign
