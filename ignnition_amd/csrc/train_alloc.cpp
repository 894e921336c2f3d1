// train_alloc.cpp — ign_batch_enable_training: everything a batch needs before its first training
// step (train_state.h's TrainState).  Per entity the hidden-state versions and gradient buffers, per
// MP what its forward saves into and the transposed tables its backward walks (lowered on the host
// by train_lower.cpp, or sorted on the GPU by train_csr.hip), the scratch the MP instances and
// readout layers of a backward share, and the deferred weight-gradient slots.  The device pool hands
// out its blocks by request order: the order of the talloc / tupload / pool_alloc calls below is
// part of what a reused pool's batches depend on.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "train_state.h"
#include "train_kernels.h"
#include "train_lower.h"

void train_state_destroy(TrainState* t) {
  if (!t) return;
  if (t->pool) pool_release(t->pool, t->allocs, t->stream);
  delete t;
}

namespace ign {

int talloc(TrainState* t, float** out, int64_t n) {
  void* p = nullptr;
  hipError_t e = pool_alloc(t->pool, &p, (std::max<int64_t>(n, 0) + 256) * sizeof(float), true);
  if (e != hipSuccess) return fail(IGN_ERR_OOM, "training buffers: device alloc (%lld floats): %s", (long long)n,
                                   hipGetErrorString(e));
  t->allocs.push_back(p);
  *out = static_cast<float*>(p);
  return IGN_OK;
}

}  // namespace ign

namespace {

// The transposed CSRs of MP mb on the GPU (train_csr.hip; IGN_TRAIN_CSR_GPU=0: build_csrs on the
// host): a stable radix sort of the step (seq) or message keys on the upload stream, the same
// arrays as the host's.  ptr[s]: row pointers of source slot s into idx, the sorted values every
// slot shares.  The keys and the sort's scratch go back to the pool behind a fence.
int tcsr_gpu(TrainState* t, const MPB& mb, int S, const int64_t* tkeys, bool seq, std::vector<int32_t*>& ptr,
             int32_t*& idx) {
  hipStream_t st = upload_stream();
  const int64_t n = seq ? mb.n_steps : mb.n_msgs;
  int rc;
  float* f = nullptr;
  if ((rc = talloc(t, &f, std::max<int64_t>(n, 1)))) return rc;
  idx = reinterpret_cast<int32_t*>(f);
  ptr.assign(S, nullptr);
  for (int s = 0; s < S; ++s) {
    if ((rc = talloc(t, &f, tkeys[s] + 1))) return rc;
    ptr[s] = reinterpret_cast<int32_t*>(f);
  }
  const size_t nb = (size_t)std::max<int64_t>(n, 1) * 4, tb = tcsr_temp_bytes(std::max<int64_t>(n, 1));
  std::vector<void*> scratch(4, nullptr);
  for (int k = 0; k < 4; ++k) {
    const hipError_t e = pool_alloc(t->pool, &scratch[k], k < 3 ? nb : std::max<size_t>(tb, 256), false);
    if (e != hipSuccess) {
      scratch.resize(k);
      pool_release(t->pool, scratch, st);
      return fail(IGN_ERR_OOM, "training CSR scratch: device alloc: %s", hipGetErrorString(e));
    }
  }
  uint32_t* keys_in = static_cast<uint32_t*>(scratch[0]);
  uint32_t* keys_out = static_cast<uint32_t*>(scratch[1]);
  int32_t* vals_in = static_cast<int32_t*>(scratch[2]);
  uint32_t max_key = 0;
  hipError_t e;
  if (seq) {
    e = launch_tcsr_keys_seq(mb.d_step_code, n, (uint32_t)mb.zero_row, keys_in, vals_in, st);
    max_key = (uint32_t)mb.zero_row;
  } else {
    e = launch_tcsr_keys_sum(mb.d_msg_ptr, mb.d_order, mb.n_dst, mb.d_msg_src, keys_in, vals_in, st);
    // one slot: the codes are the rows (radix passes over the row bits only); else slot bits above
    max_key = S == 1 ? (uint32_t)std::max<int64_t>(tkeys[0], 1) : ((uint32_t)(S - 1) << IGN_SLOT_SHIFT) | IGN_ROW_MASK;
  }
  if (e == hipSuccess) e = launch_tcsr_sort(scratch[3], tb, keys_in, keys_out, vals_in, idx, n, max_key, st);
  for (int s = 0; s < S && e == hipSuccess; ++s) {
    const uint32_t key0 = seq ? (uint32_t)mb.src_off[s] : (uint32_t)s << IGN_SLOT_SHIFT;
    e = launch_tcsr_ptr(keys_out, n, key0, tkeys[s], ptr[s], st);
  }
  pool_release(t->pool, scratch, st);
  if (e != hipSuccess) return fail(IGN_ERR_DEVICE, "training CSR sort: %s", hipGetErrorString(e));
  return IGN_OK;
}

// every used GRU cell has its backward fragments
int check_train_shapes(const ign_plan* p) {
  for (size_t c = 0; c < p->cells.size(); ++c) {
    const CellP& cp = p->cells[c];
    if (!cp.used) continue;
    bool concat_only = true;   // W^T is not needed by a cell fed only by axis-2 concat MPs
    for (auto& mp : p->mps)
      if (mp.cell == (int)c && !mp.feature_concat) concat_only = false;
    if (cp.pk_ut < 0 || (cp.pk_wt < 0 && !concat_only))
      return fail(IGN_ERR_UNSUPPORTED, "no backward kernel for GRU shape (input %d, units %d)", cp.din, cp.H);
  }
  return IGN_OK;
}

// per entity: the hidden-state versions, 1 + T x (MPs updating the entity), and the two dS buffers
int alloc_states(const ign_plan* p, const ign_batch* b, TrainState* t) {
  const int E = (int)p->ents.size();
  int rc;
  hvec<int> nver(E, 1);
  for (auto& mp : p->mps) nver[mp.dst] += p->T;
  t->ver.resize(E);
  t->cur.assign(E, 0);
  t->ent.assign(E, nullptr);
  for (int e = 0; e < E; ++e) {
    const int64_t n = (b->rows[e] + b->halo[e]) * p->ents[e].hidden_dim;   // owned rows, then halo rows
    for (int v = 0; v < nver[e]; ++v) {
      float* f = nullptr;
      if ((rc = talloc(t, &f, n))) return rc;
      t->ver[e].push_back(f);
    }
    for (int k = 0; k < 2; ++k) {
      float* f = nullptr;
      if ((rc = talloc(t, &f, n))) return rc;
      t->dS[k].push_back(f);
    }
  }
  return IGN_OK;
}

TrainMpIn host_tables(const MPB& mb) {
  return {mb.h_order, mb.h_len, mb.h_step_ptr, mb.h_msg_ptr, mb.h_multi_ptr, mb.h_step_code,
          mb.h_msg_src, mb.h_multi_rows, mb.src_off, mb.zero_row, mb.n_dst, mb.n_msgs};
}

// message network of source s (GM:440-475): the state row -> edge CSRs of its backward, from the
// edge rows the batch keeps on the device
int enable_msg_net(const ign_batch* b, TrainState* t, const MPP& mp, const MPB& mb, int s, MPTrain& mt) {
  const int se = mp.src[s].entity;
  const int64_t ne = mb.n_edges[s];
  int rc;
  hvec<int32_t> es(ne), ed(ne);
  HIP_TRY(hipMemcpyAsync(es.data(), mb.d_edge_src[s], ne * sizeof(int32_t), hipMemcpyDeviceToHost, upload_stream()));
  HIP_TRY(hipMemcpyAsync(ed.data(), mb.d_edge_dst[s], ne * sizeof(int32_t), hipMemcpyDeviceToHost, upload_stream()));
  HIP_TRY(hipStreamSynchronize(upload_stream()));
  HIP_TRY(upload_flush());
  hvec<int32_t> p1, i1, p2, i2;
  lower_row_edges(b->rows[se] + b->halo[se], es.data(), ne, &p1, &i1);   // sources may be halo rows (edge-cut)
  lower_row_edges(b->rows[mp.dst], ed.data(), ne, &p2, &i2);
  if ((rc = tupload(t, &mt.nsrc_ptr[s], p1)) || (rc = tupload(t, &mt.nsrc_idx[s], i1)) ||
      (rc = tupload(t, &mt.ndst_ptr[s], p2)) || (rc = tupload(t, &mt.ndst_idx[s], i2)))
    return rc;
  return IGN_OK;
}

// MP mi: the buffers its forward saves into and the tables its backward walks.  The transposed
// CSRs (source row -> steps / destinations reading it) are built on the GPU (mt.tptr, gidx) or on
// the host (tptr, tidx, uploaded with the slots)
int enable_mp(const ign_plan* p, const ign_batch* b, TrainState* t, size_t mi, bool tcsr_on) {
  const MPP& mp = p->mps[mi];
  const MPB& mb = b->mp[mi];
  const int H = p->cells[mp.cell].H, DIN = mp.din, S = (int)mp.src.size();
  const TrainMpIn in = host_tables(mb);
  int rc;
  MPTrain mt;
  std::vector<hvec<int32_t>> tptr, tidx;
  int32_t* gidx = nullptr;
  int64_t tkeys[IGN_MAX_SLOTS] = {0, 0, 0, 0};
  for (int s = 0; s < S; ++s) tkeys[s] = train_keys(mp, s, b->rows, b->halo, mb.n_edges);
  if (mb.sorted) {
    mt.hs_rows = mb.n_steps + mb.n_dst;
    for (int it = 0; it < p->T; ++it) {
      float* f = nullptr;
      // + one pad row: the resident training forward's tile headers point padding positions there
      // (resident.hip, hsb; its stores skip them, so the row stays unwritten)
      if ((rc = talloc(t, &f, (mt.hs_rows + 1) * H))) return rc;
      mt.hs.push_back(f);
    }
    {
      const int64_t n_pos = (mb.n_dst + 15) / 16 * 16;
      float* f = nullptr;
      if ((rc = talloc(t, &f, 4 * n_pos))) return rc;
      mt.hdrb = reinterpret_cast<int32_t*>(f);
      // on the upload stream, behind the block's IGN_POOL_POISON fill (pool_alloc) and before the
      // synchronisation at the end of this call: a launch on the plan stream could land first
      HIP_TRY(launch_seq_bwd_hdr(mb.d_seq_hdr, mb.d_step_code, n_pos, mt.hdrb, upload_stream()));
    }
    // a pre-summed row expands into its source rows on the host only
    if (tcsr_on && mb.n_multi == 0) {
      if ((rc = tcsr_gpu(t, mb, S, tkeys, true, mt.tptr, gidx))) return rc;
    } else lower_train_ordered(S, tkeys, in, tptr, tidx);
  } else {
    for (int it = 0; it < p->T; ++it) {
      float* f = nullptr;
      if ((rc = talloc(t, &f, mb.n_dst * DIN))) return rc;
      mt.xs.push_back(f);
      if (mp.aggr == IGN_AGGR_CONVOLUTION) {
        if ((rc = talloc(t, &f, mb.n_dst * DIN))) return rc;
        mt.ss.push_back(f);
      }
    }
    if (mp.aggr == IGN_AGGR_ATTENTION) {
      // (no halo rows under attention; a message network's codes address its edges, the per-edge message rows)
      TrainAttn at;
      lower_train_attention(S, tkeys, in, &at);
      if ((rc = tupload(t, &mt.amdst, at.mdst))) return rc;
      for (int s = 0; s < S; ++s) {
        int32_t *dp = nullptr, *di = nullptr;
        if ((rc = tupload(t, &dp, at.ptr[s])) || (rc = tupload(t, &di, at.idx[s]))) return rc;
        mt.asptr.push_back(dp);
        mt.asidx.push_back(di);
      }
    }
    if (mp.aggr == IGN_AGGR_CONVOLUTION) {
      hvec<float> deg;
      lower_train_degree(in, &deg);
      if ((rc = tupload(t, &mt.deg, deg))) return rc;
    }
    if (tcsr_on) {
      if ((rc = tcsr_gpu(t, mb, S, tkeys, false, mt.tptr, gidx))) return rc;
    } else lower_train_sum(S, tkeys, in, tptr, tidx);
  }
  for (int s = 0; s < S; ++s) {
    if (gidx) {
      mt.tidx.push_back(gidx);   // (mt.tptr[s] set by tcsr_gpu)
    } else {
      int32_t *dp = nullptr, *di = nullptr;
      if ((rc = tupload(t, &dp, tptr[s])) || (rc = tupload(t, &di, tidx[s]))) return rc;
      mt.tptr.push_back(dp);
      mt.tidx.push_back(di);
    }
    mt.trows.push_back(tkeys[s]);
    if (!mp.nn[s].layers.empty() && (rc = enable_msg_net(b, t, mp, mb, s, mt))) return rc;
  }
  t->mp.push_back(std::move(mt));
  return IGN_OK;
}

// floats of the scratch buffers the MP instances / readout layers of a backward share: the largest need of each
struct TrainScratch {
  int64_t ga = 0, gu = 0, dx = 0, dtab = 0, part = 0, rsrc = 0, gu2 = 0, rh = 0;
  int64_t dmsg = 0, mz = 0, mdin = 0;            // message networks
  int64_t amsg = 0, arows = 0;                   // attention
  int64_t dz = 0, rz = 0, rcat = 0, ties = 0;    // readout
  std::vector<int64_t> drop;                     // per Dropout site: rows x units
  std::vector<int64_t> norm, norm_rows;          // per LayerNormalization site: rows x units, rows
};
TrainScratch train_scratch(const ign_plan* p, const ign_batch* b) {
  TrainScratch z;
  auto need_part = [&](int64_t rows, int M, int N) { z.part = std::max(z.part, tsgemm_partial_floats(rows, M, N)); };
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {
    const MPP& mp = p->mps[mi];
    const MPB& mb = b->mp[mi];
    const int H = p->cells[mp.cell].H, DIN = mp.din, S = (int)mp.src.size();
    if (mb.sorted) {
      const int64_t hs_rows = mb.n_steps + mb.n_dst;
      z.ga = std::max(z.ga, (mb.n_steps + 1) * 3 * H);   // + the pad slot row (seq_gru_bwd_kernel)
      z.gu = std::max(z.gu, hs_rows * 3 * H);
      if (!p->cells[mp.cell].reset_after) {
        z.gu2 = std::max(z.gu2, hs_rows * 3 * H);
        z.rh = std::max(z.rh, hs_rows * H);
      }
      need_part(hs_rows, H, 3 * H);
      if (p->bwd_fuse && seq_bwd_fused_supported(H)) z.part = std::max(z.part, seq_bwd_partial_floats(H));
      for (int s = 0; s < S; ++s) {
        z.dtab = std::max(z.dtab, mb.src_rows[s] * 3 * H);
        if (p->conv_F && mp.nn[s].layers.empty())
          z.rsrc = std::max(z.rsrc, train_keys(mp, s, b->rows, b->halo, mb.n_edges) *
                                        (mp.feature_concat ? p->ents[mp.src[s].entity].hidden_dim : DIN));
        need_part(mb.src_rows[s], mp.feature_concat ? p->ents[mp.src[s].entity].hidden_dim : DIN, 3 * H);
      }
    } else {
      if (mp.aggr == IGN_AGGR_ATTENTION) {
        for (int s = 0; s < S; ++s) {
          const int64_t rows_s = train_keys(mp, s, b->rows, b->halo, mb.n_edges);
          z.arows = std::max(z.arows, rows_s);
          need_part(rows_s, DIN, 1);
        }
        z.amsg = std::max(z.amsg, mb.n_msgs);
        z.arows = std::max(z.arows, mb.n_dst);
        need_part(mb.n_dst, H, 1);
      }
      if (mp.aggr == IGN_AGGR_CONVOLUTION) {
        z.dtab = std::max(z.dtab, 2 * mb.n_dst * DIN);   // du and d(sum) of the convolution
        need_part(mb.n_dst, DIN, DIN);
      }
      z.ga = std::max(z.ga, mb.n_dst * 3 * H);
      z.gu = std::max(z.gu, mb.n_dst * 3 * H);
      if (!p->cells[mp.cell].reset_after) {
        z.gu2 = std::max(z.gu2, mb.n_dst * 3 * H);
        z.rh = std::max(z.rh, mb.n_dst * H);
      }
      z.dx = std::max(z.dx, mb.n_dst * DIN);
      need_part(mb.n_dst, std::max(DIN, H), 3 * H);
    }
    need_part(std::max<int64_t>(mb.n_steps, mb.n_dst), 1, 3 * H);   // colsum
    for (int s = 0; s < S; ++s) {
      const MsgNN& nn = mp.nn[s];
      if (nn.layers.empty()) continue;
      const int64_t ne = mb.n_edges[s];
      int widest = nn.din_pad;
      for (size_t l = 0; l < nn.layers.size(); ++l) {
        widest = std::max(widest, nn.layers[l].out);
        need_part(ne, l == 0 ? nn.din : nn.layers[l].in, nn.layers[l].out);
      }
      z.dmsg = std::max(z.dmsg, ne * nn.dout());
      z.mz = std::max(z.mz, ne * widest);
      z.mdin = std::max(z.mdin, ne * nn.din);
    }
  }
  const int64_t P = b->n_pred;
  int64_t widest = p->ro_width;
  for (auto& d : p->dense) {
    widest = std::max<int64_t>(widest, d.out);
    need_part(P, d.in, d.out);
  }
  z.dz = P * widest;
  for (auto& op : p->ro_ops) {   // readout operations (GM:605-655)
    const int64_t n = space_rows(p, b, p->ro_t[op.in[0]]);
    if (op.type == IGN_RO_NEURAL_NETWORK) {
      int widest = op.in_width, K = op.in_width;
      for (auto& d : op.layers) {
        widest = std::max(widest, d.out);
        need_part(n, K, d.out);
        K = d.out;
      }
      z.rz = std::max(z.rz, n * widest);
      if (op.in.size() > 1) z.rcat = std::max(z.rcat, n * op.in_width);
    } else if (op.type == IGN_RO_POOLING) {
      z.ties = std::max(z.ties, (int64_t)b->G * p->ro_t[op.in[0]].width);
    }
  }
  for (const DropSite& d : p->drops) z.drop.push_back(stack_rows(p, b, d.stack) * d.units);
  for (const NormSite& ns : p->norms) {
    const int64_t rows = stack_rows(p, b, ns.stack);
    z.norm.push_back(rows * ns.units);
    z.norm_rows.push_back(rows);
    z.part = std::max(z.part, layernorm_partial_floats(rows, ns.units));
  }
  return z;
}

int alloc_mp_scratch(const ign_plan* p, TrainState* t, const TrainScratch& z) {
  int rc;
  if ((rc = talloc(t, &t->ga, z.ga)) || (rc = talloc(t, &t->gu, z.gu)) || (rc = talloc(t, &t->dx, z.dx)) ||
      (rc = talloc(t, &t->dtab, z.dtab)))
    return rc;
  if (z.gu2 && ((rc = talloc(t, &t->gu2, z.gu2)) || (rc = talloc(t, &t->rh, z.rh)))) return rc;
  if (z.rsrc && (rc = talloc(t, &t->rsrc, z.rsrc))) return rc;
  if (z.amsg && ((rc = talloc(t, &t->adw, z.amsg)) || (rc = talloc(t, &t->adv, z.amsg)) ||
                 (rc = talloc(t, &t->ads_src, z.arows)) || (rc = talloc(t, &t->ads_dst, z.arows)) ||
                 (rc = talloc(t, &t->adw12, 2 * p->attn_F))))
    return rc;
  if (z.dmsg && ((rc = talloc(t, &t->dmsg, z.dmsg)) || (rc = talloc(t, &t->mz[0], z.mz)) ||
                 (rc = talloc(t, &t->mz[1], z.mz)) || (rc = talloc(t, &t->mdin, z.mdin))))
    return rc;
  return IGN_OK;
}

// the readout's saved activations and gradient buffers; per extend op, its two input row -> edge CSRs
int alloc_readout(const ign_plan* p, const ign_batch* b, TrainState* t, const TrainScratch& z) {
  const int64_t P = b->n_pred;
  int rc;
  for (size_t l = 0; l + 1 < p->dense.size(); ++l) {
    float* f = nullptr;
    if ((rc = talloc(t, &f, P * p->dense[l].out))) return rc;
    t->act.push_back(f);
  }
  if ((rc = talloc(t, &t->dz[0], z.dz)) || (rc = talloc(t, &t->dz[1], z.dz))) return rc;
  if (p->ro_in.size() > 1 &&
      ((rc = talloc(t, &t->ro_x, P * p->ro_width)) || (rc = talloc(t, &t->dro, P * p->ro_width))))
    return rc;
  // readout operations (GM:605-655)
  t->dT.assign(p->ro_t.size(), nullptr);
  for (size_t k = 0; k < p->ro_ops.size(); ++k) {
    const RoOp& op = p->ro_ops[k];
    const int nout = op.type == IGN_RO_EXTEND ? 2 : 1;
    for (int j = 0; j < nout; ++j) {
      const RoTensor& to = p->ro_t[op.out + j];
      if ((rc = talloc(t, &t->dT[op.out + j], space_rows(p, b, to) * to.width))) return rc;
    }
    if (op.type != IGN_RO_EXTEND) continue;
    for (int j = 0; j < 2; ++j) {
      const std::vector<int32_t>& ix = b->ro[k].h_idx[j];
      hvec<int32_t> ptr, idx;
      lower_row_edges(space_rows(p, b, p->ro_t[op.in[j]]), ix.data(), (int64_t)ix.size(), &ptr, &idx);
      int32_t *dp = nullptr, *di = nullptr;
      if ((rc = tupload(t, &dp, ptr)) || (rc = tupload(t, &di, idx))) return rc;
      t->rx_ptr.push_back(dp);
      t->rx_idx.push_back(di);
    }
  }
  if ((z.rz && ((rc = talloc(t, &t->rz[0], z.rz)) || (rc = talloc(t, &t->rz[1], z.rz)))) ||
      (z.rcat && (rc = talloc(t, &t->rcat, z.rcat))) || (z.ties && (rc = talloc(t, &t->rties, z.ties))))
    return rc;
  for (int64_t n : z.drop) {   // one [rows][units] buffer per Dropout site
    float* f = nullptr;
    if ((rc = talloc(t, &f, n))) return rc;
    t->dbuf.push_back(f);
  }
  for (size_t s = 0; s < z.norm.size(); ++s) {
    float *f = nullptr, *m = nullptr;
    if ((rc = talloc(t, &f, z.norm[s])) || (rc = talloc(t, &m, 2 * z.norm_rows[s]))) return rc;
    t->nbuf.push_back(f);
    t->nstats.push_back(m);
  }
  return IGN_OK;
}

// IGN_DEFER_WGRAD (default on): the per-instance weight gradients of the plain sum and ordered MPs
// (ign_backward_mp): one slot per (gradient tensor, shape), room for every instance of a backward
int alloc_deferred(const ign_plan* p, const ign_batch* b, TrainState* t) {
  int rc;
  struct Want { int64_t c, cb; int M, N, ones; int64_t chunks; };
  std::vector<Want> want;
  auto add = [&](int64_t c, int64_t cb, int M, int N, int64_t rows, int64_t min_slots = 0) {
    const int ones = cb >= 0;
    const int64_t ch = std::max(tsgemm_chunks(rows, M, N, ones), min_slots) * p->T;
    for (auto& w : want)
      if (w.c == c && w.cb == cb && w.M == M && w.N == N) { w.chunks += ch; return; }
    want.push_back({c, cb, M, N, ones, ch});
  };
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {
    const MPP& mp = p->mps[mi];
    const MPB& mb = b->mp[mi];
    const CellP& cp = p->cells[mp.cell];
    bool nets = false;
    for (auto& nn : mp.nn) nets = nets || !nn.layers.empty();
    if (nets || mp.feature_concat) continue;
    const int H = cp.H, H3 = 3 * cp.H, DIN = mp.din;
    if (mp.sorted) {
      for (size_t s2 = 0; s2 < mp.src.size(); ++s2) add(cp.off_k, -1, DIN, H3, t->mp[mi].trows[s2]);
    } else if (mp.aggr == IGN_AGGR_SUM && cp.is_default()) {   // (a cell with options reduces per instance)
      const int64_t fw = sum_bwd_fused_waves(mb.n_dst, DIN, H);   // the fused sum backward's partials
      add(cp.off_k, cp.off_b, DIN, H3, mb.n_dst, fw);
      add(cp.off_rk, cp.off_b + H3, H, H3, mb.n_dst, fw);
    }
  }
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {   // the fused ordered backward's partials
    const MPP& mp = p->mps[mi];
    const CellP& cp = p->cells[mp.cell];
    if (!mp.sorted || !p->bwd_fuse || !seq_bwd_fused_supported(cp.H) || !cp.is_default()) continue;
    const int64_t tiles = (b->mp[mi].n_dst + 15) / 16;
    const int64_t waves = std::min<int64_t>((tiles + 3) / 4 * 4, kBwdPartialWaves) * p->T;   // upper bound
    bool found = false;
    for (auto& d : t->defer_seq)
      if (d.cell == mp.cell) { d.cap += waves; found = true; }
    if (!found) t->defer_seq.push_back({mp.cell, cp.H, nullptr, waves, 0});
  }
  for (auto& d : t->defer_seq)
    if ((rc = talloc(t, &d.part, (d.cap + kTsReduceSegs) * (int64_t)(d.H + 2) * 3 * d.H))) return rc;
  for (auto& w : want) {
    TrainState::DeferredGrad d{w.c, w.cb, w.M, w.N, w.ones, nullptr, w.chunks, 0};
    if ((rc = talloc(t, &d.part, (w.chunks + kTsReduceSegs) * (int64_t)(w.M + w.ones) * w.N))) return rc;
    t->defer.push_back(d);
  }
  return IGN_OK;
}

}  // namespace

extern "C" {

int ign_batch_enable_training(ign_plan* p, ign_batch* b) {
  if (!p || !b) return fail(IGN_ERR_INVALID, "null argument");
  if (b->plan != p) return fail(IGN_ERR_INVALID, "batch was created for another plan");
  if (b->train) return IGN_OK;
  int rc = ensure_device(p);
  if (rc) return rc;
  UploadScope scope("ign_batch_enable_training");
  BuildMarks bm(env_flag("IGN_BUILD_PROF_FINE", false));   // IGN_BUILD_PROF_FINE=1: host sections of this build
  if ((rc = check_train_shapes(p))) return rc;
  std::unique_ptr<TrainState, void (*)(TrainState*)> t(new TrainState(), train_state_destroy);
  t->pool = b->pool.get();
  t->stream = p->stream;
  if ((rc = alloc_states(p, b, t.get()))) return rc;
  for (size_t mi = 0; mi < p->mps.size(); ++mi) {
    if ((rc = enable_mp(p, b, t.get(), mi, p->train_csr_gpu))) return rc;
    bm.mark(mi == 0 ? "mp0" : mi == 1 ? "mp1" : "mp2+");
  }
  const TrainScratch z = train_scratch(p, b);
  if ((rc = alloc_mp_scratch(p, t.get(), z)) || (rc = alloc_readout(p, b, t.get(), z))) return rc;
  if ((rc = talloc(t.get(), &t->part, z.part)) || (rc = talloc(t.get(), &t->bsum, (32 + 1) * 3 * 32))) return rc;
  if (p->defer_wgrad && (rc = alloc_deferred(p, b, t.get()))) return rc;
  bm.mark("rest");
  HIP_TRY(hipStreamSynchronize(upload_stream()));   // IGN_POOL_POISON fills have landed
  HIP_TRY(upload_flush());                           // (and every staged copy)
  bm.mark("wait");
  bm.print("ign_batch_enable_training fine");
  b->train = t.release();
  return IGN_OK;
}

int ign_batch_enable_edge_param_gradients(ign_plan* p, ign_batch* b) {
  if (!p || !b) return fail(IGN_ERR_INVALID, "null argument");
  if (b->plan != p) return fail(IGN_ERR_INVALID, "batch was created for another plan");
  if (!b->train) return fail(IGN_ERR_INVALID, "training not enabled on this batch (ign_batch_enable_training)");
  TrainState* t = b->train;
  if (t->edge_grads) return IGN_OK;
  int rc = set_device(p->device);
  if (rc) return rc;
  for (size_t mi = 0; mi < p->mps.size(); ++mi)
    for (size_t s = 0; s < p->mps[mi].src.size(); ++s) {
      const MsgNN& nn = p->mps[mi].nn[s];
      if (nn.layers.empty() || std::find(nn.inputs.begin(), nn.inputs.end(), (int)IGN_MSG_EDGE_PARAMS) == nn.inputs.end())
        continue;
      if (!t->mp[mi].dprm[s] && (rc = talloc(t, &t->mp[mi].dprm[s], b->mp[mi].n_edges[s] * nn.param_dim))) return rc;
    }
  t->edge_grads = true;
  return IGN_OK;
}

}  // extern "C"
