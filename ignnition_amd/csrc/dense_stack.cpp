// dense_stack.cpp — the training step's Dense stacks, forward and backward (dense_stack.h).
#include "dense_stack.h"
#include "train_kernels.h"

namespace ign {

int add_l2_grad(const ign_plan* p, const DenseP& d, float* grads, float scale, hipStream_t st) {
  if (d.l2 != 0.f)
    HIP_TRY(launch_axpy(grads + d.off_w, p->d_params + d.off_w, 2.f * d.l2 * scale, (int64_t)d.in * d.out, st));
  return IGN_OK;
}

int dense_stack_forward(const ign_plan* p, const DenseStackRun& r, hipStream_t st) {
  const float* in = r.x;
  int stride = r.ldx;
  int tail0 = 0;
  const int tail = r.drop ? drop_range(p, r.stack, r.L, &tail0) : 0;   // sites after the last layer mask y
  for (int l = 0; l < r.L; ++l) {
    const DenseP& d = r.layers[l];
    int s0 = 0;
    // in front of a layer each site masks into its own buffer, never the tensor another operation reads
    if (const int ns = r.drop ? drop_range(p, r.stack, l, &s0) : 0)
      HIP_TRY(drop_fwd_chain(p, *r.drop, s0, ns, in, r.n * d.in, st, &in));
    float* o = l + 1 < r.L ? r.hid[l] : tail ? r.drop->buf[tail0] : r.y;
    const float* bias = d.use_bias ? p->d_params + d.off_b : nullptr;
    if (p->train_dense_bf && p->train_dense_h16 && d.pk_hn >= 0 && stride % 4 == 0)   // split-fp16 (x3)
      HIP_TRY(launch_dense_h16(in, r.n, d.in, stride, p->d_packed + d.pk_hn, bias, d.out, d.act, o, st));
    else if (p->train_dense_bf && d.pk_bfn >= 0 && stride % 4 == 0)   // split-bf16, fp32-exact operands
      HIP_TRY(launch_dense_bf(in, r.n, d.in, stride, p->d_packed + d.pk_bfn, bias, d.out, d.act, o, st));
    else   // (MFMA fragments cover the whole row: a message network's layer 0 contracts its zero-padded stride)
      HIP_TRY(launch_dense_fwd(in, r.n, d.pk_w >= 0 ? stride : d.in, stride, d.pk_w >= 0 ? p->d_packed + d.pk_w : nullptr,
                               p->d_params + d.off_w, bias, d.out, d.act, o, st));
    in = o;
    stride = d.out;
  }
  // the last layer wrote the first site's buffer; the masked result goes to y
  if (tail) HIP_TRY(drop_fwd_tail(p, *r.drop, tail0, tail, r.y, r.n * r.layers[r.L - 1].out, st));
  return IGN_OK;
}

int dense_stack_backward(const ign_plan* p, const DenseStackRun& r, hipStream_t st) {
  const int L = r.L;
  const int64_t n = r.n;
  float* const* gz = r.gz;
  int rc, zi = 0;
  // Dropout sites: the masks of this forward, regenerated.  A site in front of layer l sits between
  // hid[l - 1] = y (the layer below's activation derivative reads it) and its own buffer z (layer
  // l's input: its weight gradient reads it); the fusions below that form a layer's gradient rows
  // from the layer above's decline across one
  int s0 = 0, ns = r.drop ? drop_range(p, r.stack, L, &s0) : 0;
  const DenseP& top = r.layers[L - 1];
  const float *dy = r.dy, *y = r.y;
  if (ns) {   // after the last layer: d(masked y) -> d(y), y in the first site's buffer
    HIP_TRY(drop_bwd_chain(p, *r.drop, s0, ns, dy, gz[1], n * top.out, st));
    dy = gz[1];
    y = r.drop->buf[s0];
  }
  HIP_TRY(launch_act_bwd(dy, y, n * top.out, top.act, gz[0], st));
  // a 1-unit output layer's backward rows, dz[r][k] = dz_out[r] w[k] act'(a[r][k]), are formed by
  // the layer below's input-gradient kernel (dense_bf) as it loads a, and written over a in place
  // for that layer's weight gradient: row_outer_t's separate read of a is gone
  OuterRows xo{};
  auto dense_t_bf = [&](const DenseP& d) { return p->train_dense_bf && (p->train_dense_h16 ? d.pk_ht >= 0 : d.pk_bft >= 0); };
  for (int l = L - 1; l >= 0; --l) {
    const DenseP& d = r.layers[l];
    ns = r.drop ? drop_range(p, r.stack, l, &s0) : 0;   // sites in front of this layer: its input is the last one's z
    const float* A = ns ? r.drop->buf[s0 + ns - 1] : l == 0 ? r.x : r.hid[l - 1];
    auto wgrad = [&](const float* dz) {   // the layer's weight / bias gradient from its dz rows, then its l2 term
      HIP_TRY(launch_tsgemm_add(A, ns || l > 0 ? d.in : r.ldx, dz, d.out, n, d.in, d.out, r.part, r.grads + d.off_w,
                                d.use_bias ? r.grads + d.off_b : nullptr, st));
      return r.l2_scale ? add_l2_grad(p, d, r.grads, *r.l2_scale, st) : IGN_OK;
    };
    const bool outer = xo.s != nullptr;   // this layer's dz is formed by its dense_t from hid[l]
    if (!outer && (rc = wgrad(gz[zi]))) return rc;
    if (l > 0 && d.out == 1 && d.in % 4 == 0 && p->fuse_outer_bwd && dense_t_bf(r.layers[l - 1]) && !ns) {
      xo = OuterRows{gz[zi], p->d_params + d.off_w, r.layers[l - 1].act, r.hid[l - 1]};
      continue;   // zi stays: gz[zi] holds dz_out for the layer below
    }
    // the layer below's activation derivative rides on the input-gradient kernel, except across a
    // site: d(z) there, the mask and the derivative below
    const int act = l > 0 && !ns ? r.layers[l - 1].act : -1;
    const float* aprev = l > 0 && !ns ? r.hid[l - 1] : nullptr;
    // d(x) of layer 0 goes to dx; behind a site, a dx that is added to takes the masked rows below
    const bool to_dx = l == 0 && !(r.dx_acc && ns);
    float* out = to_dx ? r.dx : gz[1 - zi];
    const int acc = to_dx ? r.dx_acc : 0;
    const float* dzin = outer ? xo.out : gz[zi];
    if (p->train_dense_bf && p->train_dense_h16 && d.pk_ht >= 0)   // split-fp16 (x3)
      HIP_TRY(launch_dense_h16_t(dzin, n, d.out, p->d_packed + d.pk_ht, d.in, out, acc, act, aprev, st, xo));
    else if (p->train_dense_bf && d.pk_bft >= 0)   // split-bf16, fp32-exact operands
      HIP_TRY(launch_dense_bf_t(dzin, n, d.out, p->d_packed + d.pk_bft, d.in, out, acc, act, aprev, st, xo));
    else if (outer)
      return fail(IGN_ERR_RUNTIME, "on-the-fly output-layer gradient without a dense_bf backward");
    else if (d.pk_wt >= 0)
      HIP_TRY(launch_row_gemm_t(gz[zi], n, d.out, p->d_packed + d.pk_wt, d.in, out, acc, act, aprev, st));
    else
      HIP_TRY(launch_row_gemm_t_generic(gz[zi], n, d.out, p->d_params + d.off_w, d.in, out, acc, act, aprev, st));
    if (outer && (rc = wgrad(xo.out))) return rc;   // on the rows dense_t just wrote over hid[l]
    xo = OuterRows{};
    if (ns) {   // d(z) -> d(y) through the sites, last first
      HIP_TRY(drop_bwd_chain(p, *r.drop, s0, ns, out, out, n * d.in, st));
      if (l > 0) {
        HIP_TRY(launch_act_bwd(out, r.hid[l - 1], n * d.in, r.layers[l - 1].act, gz[zi], st));
        continue;   // the layer below's dz is in gz[zi]: zi stays
      }
      if (r.dx_acc) HIP_TRY(launch_split_cols_add(r.dx, n, d.in, out, d.in, 0, st));
    }
    zi = 1 - zi;
  }
  return IGN_OK;
}

}  // namespace ign
