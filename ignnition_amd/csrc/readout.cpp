// readout.cpp — the readout program of ComnetModel.call (GM:605-655): the operations that run
// before predict, each writing a named tensor the later operations read (get_global_var_or_input,
// GM:660-675), and the head of predict that the inference and the training forward share: the tensor
// lookup, predict's input rows and the fused three-layer launch.
//
//   neural_network       Readout_nn (AUX:1188-1211): Dense stack on the axis-1 concatenation of
//                        its inputs; weights readout_model_<op index> (GM:352-358).  The stack
//                        itself, with its Dropout sites in training, is dense_stack.cpp's walk
//                        (the one predict and the message networks take); its backward and the
//                        other operations' are train.cpp's readout_ops_backward
//   pooling              Pooling_operation (AUX:1136-1185): sum / mean / max over axis 0 of one
//                        graph's rows -> [1, F]
//   product              Product_operation element_wise (AUX:1054-1094): tf.multiply
//   extend_adjacencies   Extend_adjacencies (AUX:1214-1265): gather the adjacency's source and
//                        destination rows per edge
//
// The reference runs them once per graph (model_fn's loop, GM:712-724).  In the batch every
// tensor lives on a row space whose rows are graph-contiguous: an entity's rows, one row per
// graph, or an adjacency's edges.  Pooling reduces per graph and a per-graph operand broadcasts
// over its own graph's rows, so the batch equals the per-graph loop.
//
// Not lowered: product dot_product (tf.tensordot axes=0 is an outer product of rank 4, while the
// reference records its width as 1, GM:374-375), products or concatenations across different
// entity row spaces (TF accepts them only when the row counts happen to agree), raw input
// features as readout inputs.
#include <algorithm>
#include <cstring>

#include "dense_stack.h"
#include "mp_step.h"
#include "readout_kernels.h"
#include "train_kernels.h"

namespace ign {

int64_t space_rows(const ign_plan* p, const ign_batch* b, const RoTensor& t) {
  (void)p;
  if (t.space == RS_ENTITY) return b->rows[t.sid];
  if (t.space == RS_GRAPH) return b->G;
  return b->adj_rows[t.sid];
}

// graph offsets of a row space ([G + 1])
static std::vector<int64_t> space_offsets(const ign_batch* b, const RoTensor& t) {
  std::vector<int64_t> off(b->G + 1);
  for (int g = 0; g <= b->G; ++g) {
    if (t.space == RS_GRAPH) off[g] = g;
    else if (t.space == RS_ADJ) off[g] = b->adj_off[t.sid][g];
    else off[g] = g < b->G ? b->row_off[t.sid][g] : b->rows[t.sid];
  }
  return off;
}

int64_t stack_rows(const ign_plan* p, const ign_batch* b, int stack) {
  return space_rows(p, b, p->ro_t[stack < 0 ? p->ro_in[0] : p->ro_ops[stack].in[0]]);
}

const float* readout_tensor(const ign_plan* p, const ign_batch* b, int id, const float* const* ent) {
  if (id >= (int)p->ents.size()) return b->ro_buf[id];
  return ent ? ent[id] : b->d_state[b->cur[id]][id];
}

int predict_input(const ign_plan* p, const ign_batch* b, const float* const* ent, float* cat, const float** x,
                  hipStream_t st) {
  *x = readout_tensor(p, b, p->ro_in[0], ent);
  if (p->ro_in.size() == 1) return IGN_OK;
  int col = 0;
  for (int id : p->ro_in) {
    const int w = p->ro_t[id].width;
    HIP_TRY(launch_concat_cols(cat, b->n_pred, p->ro_width, col, readout_tensor(p, b, id, ent), w, st));
    col += w;
  }
  *x = cat;
  return IGN_OK;
}

int readout_fused(ign_plan* p, const ign_batch* b, const float* x, float* save1, float* save2, Timer& tm,
                  hipStream_t st) {
  const int64_t P = b->n_pred;
  const float* prm = p->d_params;
  const DenseP &l1 = p->dense[0], &l2 = p->dense[1], &l3 = p->dense[2];
  Readout3Args a{x, P, p->ro_width,
                 p->d_packed + l1.pk_w, l1.use_bias ? prm + l1.off_b : nullptr,
                 p->d_packed + l2.pk_w, l2.use_bias ? prm + l2.off_b : nullptr,
                 prm + l3.off_w, l3.use_bias ? prm + l3.off_b : nullptr,
                 l1.act, l2.act, l3.act, b->d_pred, save1, save2};
  if (!a.b1 || !a.b2) return fail(IGN_ERR_UNSUPPORTED, "fused readout requires use_bias on hidden layers");
  double flops = 2.0 * P * ((double)l1.in * l1.out + (double)l2.in * l2.out + l3.in);
  const bool bf = p->readout_variant >= 2 && l1.pk_bf >= 0 && l2.pk_bf >= 0;
  const bool h32 = p->readout_variant == 5 && bf && l2.pk_h32 >= 0;
  const bool h16 = (p->readout_variant == 4 || (p->readout_variant == 5 && !h32)) && bf && l2.pk_h >= 0;
  const double tiles = (double)((P + 15) / 16);
  // per 16-row tile: layer 1 out/16 x in/32 and layer 2 out/16 x in/32 MFMAs of 16x16x32, x6 or x9
  // products (readout_bf); f32 (readout3): out/16 x in/4 each of 16x16x4
  const double k1 = (double)(l1.out / 16) * (l1.in / 32) + (double)(l2.out / 16) * (l2.in / 32);
  const double k1f = (double)(l1.out / 16) * (l1.in / 4) + (double)(l2.out / 16) * (l2.in / 4);
  // variant 4: both layers x3 (16x16x32 f16, the bf16 rate)
  const double kh = 3.0 * k1;
  tm.begin(K_READOUT, flops, (double)P * (4.0 * l1.in + 4.0),
           h16 || h32 ? tiles * kh * kMfmaBf16Flops : bf ? tiles * k1 * 6 * kMfmaBf16Flops : 0,
           bf ? 0 : tiles * k1f * kMfmaF32Flops);
  if (h32)   // variant 5: the same piece products on 32x32x16 (16-row-tile equivalent counted above)
    HIP_TRY(launch_readout_h32(a, p->d_packed + l2.pk_h32, l1.in, st));
  else if (h16)
    HIP_TRY(launch_readout_h16(a, p->d_packed + l2.pk_h, l1.in, st));
  else if (bf)
    HIP_TRY(launch_readout_bf(a, p->d_packed + l1.pk_bf, p->d_packed + l2.pk_bf, l1.in, 6, st));
  else
    HIP_TRY(launch_readout3(a, l1.in, l1.out, l2.out, st));
  tm.end();
  return IGN_OK;
}

int readout_batch(ign_plan* p, ign_batch* b, const ign_batch_desc* d) {
  const int G = b->G, NA = p->n_adj;
  b->adj_rows.assign(NA, 0);
  b->adj_off.assign(NA, std::vector<int64_t>(G + 1, 0));
  for (int a = 0; a < NA; ++a) {
    for (int g = 0; g < G; ++g) b->adj_off[a][g + 1] = b->adj_off[a][g] + d->adj_edges[(int64_t)g * NA + a];
    b->adj_rows[a] = b->adj_off[a][G];
  }
  b->ro_buf.assign(p->ro_t.size(), nullptr);
  b->ro.clear();
  b->ro.resize(p->ro_ops.size());
  if (!p->ro_ops.empty() && d->halo_rows)
    for (size_t e = 0; e < p->ents.size(); ++e)
      if (d->halo_rows[e] > 0) return fail(IGN_ERR_UNSUPPORTED, "readout operations on an edge-cut partition");
  int rc;
  for (size_t k = 0; k < p->ro_ops.size(); ++k) {
    const RoOp& op = p->ro_ops[k];
    RoBatchOp& bo = b->ro[k];
    const int nout = op.type == IGN_RO_EXTEND ? 2 : 1;
    for (int j = 0; j < nout; ++j) {
      const RoTensor& t = p->ro_t[op.out + j];
      if ((rc = dev_alloc(b, &bo.out[j], std::max<int64_t>(1, space_rows(p, b, t) * t.width)))) return rc;
      b->ro_buf[op.out + j] = bo.out[j];
    }
    const RoTensor& t0 = p->ro_t[op.in[0]];
    const int64_t n_in = space_rows(p, b, t0);
    switch (op.type) {
      case IGN_RO_NEURAL_NETWORK:
        if (op.in.size() > 1 && (rc = dev_alloc(b, &bo.cat, std::max<int64_t>(1, n_in * op.in_width)))) return rc;
        for (size_t l = 0; l + 1 < op.layers.size(); ++l) {
          float* t = nullptr;
          if ((rc = dev_alloc(b, &t, std::max<int64_t>(1, n_in * op.layers[l].out)))) return rc;
          bo.tmp.push_back(t);
        }
        break;
      case IGN_RO_POOLING: {
        const std::vector<int64_t> off = space_offsets(b, t0);
        std::vector<int64_t> chunk, count(G);
        std::vector<int32_t> cptr(G + 1, 0);
        for (int g = 0; g < G; ++g) {
          count[g] = off[g + 1] - off[g];
          for (int64_t r = off[g]; r < off[g + 1]; r += POOL_CHUNK) {
            chunk.push_back(r);
            chunk.push_back(std::min(off[g + 1], r + POOL_CHUNK));
          }
          cptr[g + 1] = (int32_t)(chunk.size() / 2);
        }
        bo.n_chunks = (int64_t)chunk.size() / 2;
        if ((rc = dev_upload(b, &bo.d_chunk, chunk)) || (rc = dev_upload(b, &bo.d_chunk_ptr, cptr)) ||
            (rc = dev_upload(b, &bo.d_count, count)) || (rc = dev_upload(b, &bo.d_inoff, off)))
          return rc;
        if ((rc = dev_alloc(b, &bo.d_partial, std::max<int64_t>(1, bo.n_chunks * t0.width)))) return rc;
        break;
      }
      case IGN_RO_PRODUCT:
        if ((rc = dev_upload(b, &bo.d_seg, space_offsets(b, p->ro_t[op.out])))) return rc;
        break;
      case IGN_RO_EXTEND: {
        const int a = op.adj;
        const int se = p->adj_src_ent[a], de = p->adj_dst_ent[a];
        std::vector<int32_t> is(b->adj_rows[a]), id(b->adj_rows[a]);
        for (int g = 0; g < G; ++g)
          for (int64_t e = b->adj_off[a][g]; e < b->adj_off[a][g + 1]; ++e) {
            const int64_t s = IdxArr(d->adj_src[a], d->index_bytes)[e], t = IdxArr(d->adj_dst[a], d->index_bytes)[e];
            const int64_t ns = d->num_nodes[(int64_t)g * p->ents.size() + se];
            const int64_t nd = d->num_nodes[(int64_t)g * p->ents.size() + de];
            if (s < 0 || s >= ns || t < 0 || t >= nd)   // the reference logs and exits (AUX:1253-1263)
              return fail(IGN_ERR_INVALID, "extend_adjacencies: graph %d edge %lld of adjacency %d indexes outside "
                          "its entities", g, (long long)(e - b->adj_off[a][g]), a);
            is[e] = (int32_t)(b->row_off[se][g] + s);
            id[e] = (int32_t)(b->row_off[de][g] + t);
          }
        if ((rc = dev_upload(b, &bo.idx[0], is)) || (rc = dev_upload(b, &bo.idx[1], id))) return rc;
        bo.h_idx[0] = std::move(is);
        bo.h_idx[1] = std::move(id);
        break;
      }
    }
  }
  return IGN_OK;
}

int readout_ops_run(ign_plan* p, ign_batch* b, hipStream_t st, const float* const* ent, const DropRun* drop,
                    const NormRun* norm) {
  const NormRun own{b->d_norm.data(), nullptr};   // inference: the batch's buffers, no statistics kept
  if (!norm) norm = &own;
  for (size_t k = 0; k < p->ro_ops.size(); ++k) {
    const RoOp& op = p->ro_ops[k];
    RoBatchOp& bo = b->ro[k];
    const RoTensor& t0 = p->ro_t[op.in[0]];
    const int64_t n = space_rows(p, b, t0);
    switch (op.type) {
      case IGN_RO_NEURAL_NETWORK: {   // GM:612-628
        const float* x = readout_tensor(p, b, op.in[0], ent);
        if (op.in.size() > 1) {
          int col = 0;
          for (int id : op.in) {
            HIP_TRY(launch_concat_cols(bo.cat, n, op.in_width, col, readout_tensor(p, b, id, ent), p->ro_t[id].width, st));
            col += p->ro_t[id].width;
          }
          x = bo.cat;
        }
        const DenseStackRun r{op.layers.data(), (int)op.layers.size(), n, x, op.in_width, bo.tmp.data(), bo.out[0],
                              drop, &op.seq, norm};
        if (int rc = dense_stack_forward(p, r, st)) return rc;
        break;
      }
      case IGN_RO_POOLING:            // GM:632-637
        HIP_TRY(launch_pool(readout_tensor(p, b, op.in[0], ent), t0.width, bo.n_chunks, bo.d_chunk, bo.d_chunk_ptr,
                            bo.d_count, b->G, op.mode, bo.d_partial, bo.out[0], st));
        break;
      case IGN_RO_PRODUCT: {          // GM:640-645
        const RoTensor& t1 = p->ro_t[op.in[1]];
        const RoTensor& to = p->ro_t[op.out];
        ProductArgs a{readout_tensor(p, b, op.in[0], ent), readout_tensor(p, b, op.in[1], ent), t0.width, t1.width, to.width,
                      t0.space == RS_GRAPH && to.space != RS_GRAPH, t1.space == RS_GRAPH && to.space != RS_GRAPH,
                      bo.d_seg, b->G, space_rows(p, b, to), bo.out[0]};
        HIP_TRY(launch_product(a, st));
        break;
      }
      case IGN_RO_EXTEND: {           // GM:647-655
        const int64_t e = b->adj_rows[op.adj];
        HIP_TRY(launch_gather(readout_tensor(p, b, op.in[0], ent), t0.width, bo.idx[0], e, bo.out[0], st));
        HIP_TRY(launch_gather(readout_tensor(p, b, op.in[1], ent), p->ro_t[op.in[1]].width, bo.idx[1], e, bo.out[1], st));
        break;
      }
    }
  }
  return IGN_OK;
}

}  // namespace ign
