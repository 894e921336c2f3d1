// dense_stack.cpp — the training step's Dense stacks, forward and backward (dense_stack.h).
#include "dense_stack.h"
#include "train_kernels.h"

namespace ign {

int add_l2_grad(const ign_plan* p, const DenseP& d, float* grads, float scale, hipStream_t st) {
  if (d.l2 != 0.f)
    HIP_TRY(launch_axpy(grads + d.off_w, p->d_params + d.off_w, 2.f * d.l2 * scale, (int64_t)d.in * d.out, st));
  return IGN_OK;
}

namespace {

// Run r's Dropout and LayerNormalization layers are the entries of r.seq it takes: a Dropout only
// with a mask stream (r.drop), a LayerNormalization only with buffers (r.norm).  A group of them
// stands between two Dense entries (or after the last); the walks step through a group with these.
bool taken(const DenseStackRun& r, const StackLayer& e) {
  return e.kind == SL_DROPOUT ? r.drop != nullptr : e.kind == SL_LAYERNORM && r.norm != nullptr;
}
// the first taken entry at or after i, short of the next Dense entry; -1: none
int site_from(const DenseStackRun& r, int i) {
  for (const int n = r.seq ? (int)r.seq->size() : 0; i < n && (*r.seq)[i].kind != SL_DENSE; ++i)
    if (taken(r, (*r.seq)[i])) return i;
  return -1;
}
// the last taken entry before i, short of the Dense entry below; -1: none
int site_before(const DenseStackRun& r, int i) {
  while (r.seq && i > 0 && (*r.seq)[--i].kind != SL_DENSE)
    if (taken(r, (*r.seq)[i])) return i;
  return -1;
}
// entry i's buffer (DropRun::buf, NormRun::buf)
float* site_buf(const DenseStackRun& r, int i) {
  const StackLayer& e = (*r.seq)[i];
  return e.kind == SL_LAYERNORM ? r.norm->buf[e.idx] : r.drop->buf[e.idx];
}

// one layer forward: n rows of `units` from x (ldx apart) into y (contiguous)
int site_forward(const ign_plan* p, const DenseStackRun& r, const StackLayer& s, const float* x, int ldx, float* y, int units,
                 hipStream_t st) {
  if (s.kind == SL_LAYERNORM) {
    HIP_TRY(norm_fwd(p, s.idx, x, ldx, r.n, y, r.norm->stats ? r.norm->stats[s.idx] : nullptr, st));
    return IGN_OK;
  }
  if (ldx != units) return fail(IGN_ERR_RUNTIME, "Dropout on rows that are not contiguous");
  const DropSite& d = p->drops[s.idx];
  HIP_TRY(launch_dropout_fwd(x, y, r.n * units, d.rate, d.scale, r.drop->seed ^ d.seed, (uint32_t)s.idx, r.drop->step, st));
  return IGN_OK;
}

// and back: g = d(its output) -> gx = d(its input) (gx may be g; acc: added to gx, LayerNormalization
// only); x = the layer's input rows.  A LayerNormalization adds its gamma / beta gradients to grads.
int site_backward(const ign_plan* p, const DenseStackRun& r, const StackLayer& s, const float* x, const float* g, float* gx,
                  int units, int acc, hipStream_t st) {
  if (s.kind == SL_LAYERNORM) {
    const NormSite& ns = p->norms[s.idx];
    const float* stats = r.norm->stats[s.idx];
    HIP_TRY(launch_layernorm_bwd_params(g, x, stats, r.n, units, r.part, ns.off_gamma >= 0 ? r.grads + ns.off_gamma : nullptr,
                                        ns.off_beta >= 0 ? r.grads + ns.off_beta : nullptr, st));
    HIP_TRY(launch_layernorm_bwd_dx(g, x, stats, ns.off_gamma >= 0 ? p->d_params + ns.off_gamma : nullptr, r.n, units, gx,
                                    acc, st));
    return IGN_OK;
  }
  const DropSite& d = p->drops[s.idx];
  HIP_TRY(launch_dropout_bwd(g, gx, r.n * units, d.rate, d.scale, r.drop->seed ^ d.seed, (uint32_t)s.idx, r.drop->step, st));
  return IGN_OK;
}

}  // namespace

int dense_stack_forward(const ign_plan* p, const DenseStackRun& r, hipStream_t st) {
  const float* in = r.x;
  int stride = r.ldx, rc;
  int at = 0;   // into r.seq: where the entries in front of layer l begin
  for (int l = 0; l < r.L; ++l) {
    const DenseP& d = r.layers[l];
    // in front of a layer each one writes its own buffer, never the tensor another operation reads
    for (int s = site_from(r, at); s >= 0; s = site_from(r, s + 1)) {
      if ((rc = site_forward(p, r, (*r.seq)[s], in, stride, site_buf(r, s), d.in, st))) return rc;
      in = site_buf(r, s);
      stride = d.in;
    }
    while (r.seq && (*r.seq)[at++].kind != SL_DENSE) {}   // past this layer's own entry
    // the layers after the last Dense layer turn its output into y: it writes the first one's buffer
    const int tail = l + 1 < r.L ? -1 : site_from(r, at);
    float* o = l + 1 < r.L ? r.hid[l] : tail >= 0 ? site_buf(r, tail) : r.y;
    const float* bias = d.use_bias ? p->d_params + d.off_b : nullptr;
    if (p->train_dense_bf && p->train_dense_h16 && d.pk_hn >= 0 && stride % 4 == 0)   // split-fp16 (x3)
      HIP_TRY(launch_dense_h16(in, r.n, d.in, stride, p->d_packed + d.pk_hn, bias, d.out, d.act, o, st));
    else if (p->train_dense_bf && d.pk_bfn >= 0 && stride % 4 == 0 && act_first_five(d.act))   // split-bf16, fp32-exact operands
      HIP_TRY(launch_dense_bf(in, r.n, d.in, stride, p->d_packed + d.pk_bfn, bias, d.out, d.act, o, st));
    else   // (MFMA fragments cover the whole row: a message network's layer 0 contracts its zero-padded stride)
      HIP_TRY(launch_dense_fwd(in, r.n, d.pk_w >= 0 ? stride : d.in, stride, d.pk_w >= 0 ? p->d_packed + d.pk_w : nullptr,
                               p->d_params + d.off_w, bias, d.out, d.act, o, st));
    in = o;
    stride = d.out;
  }
  // ... each of them reads its own and writes the next one's, the last y
  for (int s = site_from(r, at), nx; s >= 0; s = nx) {
    nx = site_from(r, s + 1);
    if ((rc = site_forward(p, r, (*r.seq)[s], site_buf(r, s), stride, nx >= 0 ? site_buf(r, nx) : r.y, stride, st))) return rc;
  }
  return IGN_OK;
}

int dense_stack_backward(const ign_plan* p, const DenseStackRun& r, hipStream_t st) {
  const int L = r.L;
  const int64_t n = r.n;
  float* const* gz = r.gz;
  int rc, zi = 0;
  // Dropout and LayerNormalization layers: the masks and statistics of this forward.  One in front
  // of layer l sits between hid[l - 1] = y (the layer below's activation derivative reads it) and
  // its own buffer z (layer l's input: its weight gradient reads it); the fusions below that form a
  // layer's gradient rows from the layer above's decline across one
  int at = r.seq ? (int)r.seq->size() : 0;   // into r.seq, walked down: where the entries in front of layer l end
  const DenseP& top = r.layers[L - 1];
  const float *dy = r.dy, *y = r.y;
  // after the last layer: d(y behind them) -> d(y), last first; y ends as the first one's buffer
  for (int s = site_before(r, at); s >= 0; s = site_before(r, s)) {
    if ((rc = site_backward(p, r, (*r.seq)[s], site_buf(r, s), dy, gz[1], top.out, 0, st))) return rc;
    dy = gz[1];
    y = site_buf(r, s);
  }
  HIP_TRY(launch_act_bwd(dy, y, n * top.out, top.act, gz[0], st));
  // a 1-unit output layer's backward rows, dz[r][k] = dz_out[r] w[k] act'(a[r][k]), are formed by
  // the layer below's input-gradient kernel (dense_bf) as it loads a, and written over a in place
  // for that layer's weight gradient: row_outer_t's separate read of a is gone
  OuterRows xo{};
  auto dense_t_bf = [&](const DenseP& d) { return p->train_dense_bf && (p->train_dense_h16 ? d.pk_ht >= 0 : d.pk_bft >= 0); };
  for (int l = L - 1; l >= 0; --l) {
    const DenseP& d = r.layers[l];
    while (r.seq && (*r.seq)[--at].kind != SL_DENSE) {}   // down to this layer's own entry
    const int last = site_before(r, at);   // in front of this layer: its input is the last one's z
    const bool ns = last >= 0;
    if (ns && l == 0 && r.ldx != d.in) return fail(IGN_ERR_RUNTIME, "a layer in front of a padded Dense input");
    const float* A = ns ? site_buf(r, last) : l == 0 ? r.x : r.hid[l - 1];
    auto wgrad = [&](const float* dz) {   // the layer's weight / bias gradient from its dz rows, then its l2 term
      HIP_TRY(launch_tsgemm_add(A, ns || l > 0 ? d.in : r.ldx, dz, d.out, n, d.in, d.out, r.part, r.grads + d.off_w,
                                d.use_bias ? r.grads + d.off_b : nullptr, st));
      return r.l2_scale ? add_l2_grad(p, d, r.grads, *r.l2_scale, st) : IGN_OK;
    };
    const bool outer = xo.s != nullptr;   // this layer's dz is formed by its dense_t from hid[l]
    if (!outer && (rc = wgrad(gz[zi]))) return rc;
    if (l > 0 && d.out == 1 && d.in % 4 == 0 && p->fuse_outer_bwd && dense_t_bf(r.layers[l - 1]) && !ns &&
        act_first_five(r.layers[l - 1].act)) {
      xo = OuterRows{gz[zi], p->d_params + d.off_w, r.layers[l - 1].act, r.hid[l - 1]};
      continue;   // zi stays: gz[zi] holds dz_out for the layer below
    }
    // the layer below's activation derivative rides on the input-gradient kernel, except across a
    // Dropout or LayerNormalization: d(z) there, its backward and the derivative below
    const int act = l > 0 && !ns ? r.layers[l - 1].act : -1;
    const float* aprev = l > 0 && !ns ? r.hid[l - 1] : nullptr;
    // d(x) of layer 0 goes to dx; behind such a layer, a dx that is added to takes the rows below
    const bool to_dx = l == 0 && !(r.dx_acc && ns);
    float* out = to_dx ? r.dx : gz[1 - zi];
    const int acc = to_dx ? r.dx_acc : 0;
    const float* dzin = outer ? xo.out : gz[zi];
    // dense_h16_t / dense_bf_t apply linear .. tanh's derivative themselves; another activation's
    // follows as its own launch (never beside an added-to dx: act >= 0 only above layer 0)
    const bool late = act >= 0 && !act_first_five(act) && p->train_dense_bf &&
                      ((p->train_dense_h16 && d.pk_ht >= 0) || d.pk_bft >= 0);
    const int act_t = late ? -1 : act;
    if (p->train_dense_bf && p->train_dense_h16 && d.pk_ht >= 0)   // split-fp16 (x3)
      HIP_TRY(launch_dense_h16_t(dzin, n, d.out, p->d_packed + d.pk_ht, d.in, out, acc, act_t, aprev, st, xo));
    else if (p->train_dense_bf && d.pk_bft >= 0)   // split-bf16, fp32-exact operands
      HIP_TRY(launch_dense_bf_t(dzin, n, d.out, p->d_packed + d.pk_bft, d.in, out, acc, act_t, aprev, st, xo));
    else if (outer)
      return fail(IGN_ERR_RUNTIME, "on-the-fly output-layer gradient without a dense_bf backward");
    else if (d.pk_wt >= 0)
      HIP_TRY(launch_row_gemm_t(gz[zi], n, d.out, p->d_packed + d.pk_wt, d.in, out, acc, act, aprev, st));
    else
      HIP_TRY(launch_row_gemm_t_generic(gz[zi], n, d.out, p->d_params + d.off_w, d.in, out, acc, act, aprev, st));
    if (outer && (rc = wgrad(xo.out))) return rc;   // on the rows dense_t just wrote over hid[l]
    xo = OuterRows{};
    if (late) {
      HIP_TRY(launch_act_bwd(out, aprev, n * d.in, act, gz[zi], st));
      continue;   // the layer below's dz is in gz[zi]: zi stays
    }
    if (ns) {   // d(z) -> d(y) through them, last first, in place
      // a LayerNormalization that stands first in front of layer 0 adds its rows to an added-to dx itself
      bool norm_to_dx = false;
      for (int s = last, below; s >= 0; s = below) {
        below = site_before(r, s);
        const float* xin = below >= 0 ? site_buf(r, below) : l == 0 ? r.x : r.hid[l - 1];
        norm_to_dx = below < 0 && l == 0 && r.dx_acc && (*r.seq)[s].kind == SL_LAYERNORM;
        if ((rc = site_backward(p, r, (*r.seq)[s], xin, out, norm_to_dx ? r.dx : out, d.in, norm_to_dx, st))) return rc;
      }
      if (l > 0) {
        HIP_TRY(launch_act_bwd(out, r.hid[l - 1], n * d.in, r.layers[l - 1].act, gz[zi], st));
        continue;   // the layer below's dz is in gz[zi]: zi stays
      }
      if (r.dx_acc && !norm_to_dx) HIP_TRY(launch_split_cols_add(r.dx, n, d.in, out, d.in, 0, st));
    }
    zi = 1 - zi;
  }
  return IGN_OK;
}

}  // namespace ign
