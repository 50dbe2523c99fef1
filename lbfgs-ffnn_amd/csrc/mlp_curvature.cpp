// Mlp: the curvature products, Hessian and Gauss-Newton, and Gauss-Newton CG (see runtime.hpp).
#include "runtime.hpp"

#include <algorithm>
#include <cmath>

namespace lbf {

namespace {
struct AbortScope { // ctx->abort points at a solver's own word for the duration of its run (gn_cg, lanczos)
  Ctx *c;
  const int *prev;
  ~AbortScope() { c->abort = prev; }
};
} // namespace

// The products of the R-pass (hvp, gnvp): the engine's GEMM plans on the R-pass workspace.
void Mlp::rpass_ensure(long long B) {
  if (B <= rcap_) return;
  RZ_.clear();
  RA_.clear();
  RD_.clear();
  DL_.clear();
  size_t wmax = 1, segmax = 1;
  for (auto &L : layers_) {
    RZ_.emplace_back(size_t(B) * L.out);
    RA_.emplace_back(size_t(B) * L.out);
    RD_.emplace_back(size_t(B) * L.out);
    DL_.emplace_back(act_has_d2(L.act) ? size_t(B) * L.out : size_t(1));
    // T1_ holds R{A} W_l (B x out) in the R-forward and (dZ W^T) (B x in) in the R-backward
    wmax = std::max(wmax, size_t(std::max(L.in, L.out)));
    segmax = std::max(segmax, size_t(L.in + 1) * L.out);
  }
  T1_.resize(size_t(B) * wmax);
  T2_.resize(size_t(B) * wmax);
  seg_.resize(segmax);
  rcap_ = B;
}

// Z = in * W + bias (no activation) for layer l, with the forward's tile / split-K plan
void Mlp::rpass_linear_fwd(long long B, int l, const float *Wsrc, const float *in, const int *rows, bool with_bias,
                           float *out) {
  hipStream_t s = ctx_->stream;
  const Layer &L = layers_[size_t(l)];
  GemmDesc d = fwd_launch_desc(size_t(l), Wsrc, in, rows, B);
  d.act = ACT_LINEAR;
  if (!with_bias) d.bias = nullptr;
  if (L.fsplits > 1) {
    d.C = fslab_.get(); // on purpose not fslab_buf(l): summed right below, so no second buffer to alternate with
    gemm(s, d);
    fwd_reduce_act(s, fslab_.get(), L.fsplits, B * L.out, int(B), L.out, d.bias, ACT_LINEAR, out, ctx_->abort);
  } else {
    d.C = out;
    gemm(s, d);
  }
}

// [in | ones?]^T dZ for layer l into dst (the dW GEMM's plan: split-K slabs summed in split order)
void Mlp::rpass_weight_grad(long long B, int l, const float *in, const int *rows, bool ones, const float *dZ,
                            float *dst) {
  hipStream_t s = ctx_->stream;
  const Layer &L = layers_[size_t(l)];
  GemmDesc d = dw_desc(l, in, rows, ones, dZ, B);
  const long long seg = (long long)(L.in + 1) * L.out;
  if (L.splits > 1) {
    d.C = slab_.get() + L.slab_off;
    d.slab_stride = seg;
    gemm(s, d);
    reduce_slabs(s, slab_.get() + L.slab_off, L.splits, seg, seg, dst, ctx_->abort);
  } else {
    d.C = dst;
    gemm(s, d);
  }
}

// (dZ W^T) .* act'(aux) for layer l, aux = A_[l - 1] (aux_act linear: the plain product)
void Mlp::rpass_back_prod(long long B, int l, const float *dZ, const float *Wsrc, int aux_act, float *out) {
  gemm(ctx_->stream, dx_desc(l, dZ, Wsrc, aux_act, out, B));
}

// A product's end: the all-reduce under a communicator, then out += lambda V (abort: lincomb's word, nullable)
void Mlp::curv_finish(float *out, double lambda, const float *V, const int *abort) {
  if (ctx_->dp()) ctx_->allreduce(out, nparams_);
  if (lambda != 0.0) lincomb(ctx_->stream, (long long)nparams_, out, lambda, V, out, abort);
}

// A data-parallel rank with an empty share still joins the all-reduce: its product is zeros.
void Mlp::curv_empty(float *out, double lambda, const float *V, const int *abort) {
  LBF_HIP(hipMemsetAsync(out, 0, nparams_ * sizeof(float), ctx_->stream));
  curv_finish(out, lambda, V, abort);
}

// Exact Hessian-vector product (R-operator; hvp.hip has the derivation). An unfused forward/backward
// of the batch, then the R-forward and R-backward with the same GEMM kernels: every product that
// involves the direction V is one more GEMM whose B operand is V's layer block.
void Mlp::hvp(const float *P, const float *V, const float *X, const float *Y, const int *idx, long long B,
              double inv_scale, double lambda, float *Hv) {
  LBF_REQUIRE(P && V && Hv && B >= 0 && (B == 0 || (X && Y)), "hvp: bad argument");
  hipStream_t s = ctx_->stream;
  const int nl = int(layers_.size());
  if (B == 0) return curv_empty(Hv, lambda, V, nullptr);
  ensure(B);
  rpass_ensure(B);
  // ---- forward and the plain backward (dZ_l; delta_l where act'' != 0) ----
  forward(P, X, idx, B, nl);
  const Layer &Lo = layers_[size_t(nl - 1)];
  out_loss(Y, idx, B, inv_scale);
  for (int l = nl - 1; l >= 1; --l) {
    const int pa = layers_[size_t(l - 1)].act;
    rpass_back_prod(B, l, D_[size_t(l)].get(), P, pa, D_[size_t(l - 1)].get());
    if (act_has_d2(pa)) rpass_back_prod(B, l, D_[size_t(l)].get(), P, ACT_LINEAR, DL_[size_t(l - 1)].get());
  }
  // ---- R-forward ----
  for (int l = 0; l < nl; ++l) {
    const Layer &L = layers_[size_t(l)];
    const long long nz = B * L.out;
    if (l == 0) {
      rpass_linear_fwd(B, 0, V, X, idx, true, RZ_[0].get()); // X V_0 + v_0
    } else {
      rpass_linear_fwd(B, l, V, A_[size_t(l - 1)].get(), nullptr, true, RZ_[size_t(l)].get()); // A V_l + v_l
      rpass_linear_fwd(B, l, P, RA_[size_t(l - 1)].get(), nullptr, false, T1_.get());          // R{A} W_l
      lincomb(s, nz, RZ_[size_t(l)].get(), 1.0, T1_.get(), RZ_[size_t(l)].get());
    }
    rop_act(s, nz, A_[size_t(l)].get(), RZ_[size_t(l)].get(), L.act, RA_[size_t(l)].get());
  }
  // ---- R-backward ----
  if (loss_ == LOSS_XENT)
    rop_out_xent(s, B, Lo.out, A_[size_t(nl - 1)].get(), Y, idx, RZ_[size_t(nl - 1)].get(), inv_scale,
                 RD_[size_t(nl - 1)].get());
  else
    rop_out(s, B, Lo.out, A_[size_t(nl - 1)].get(), Y, idx, RZ_[size_t(nl - 1)].get(), Lo.act, inv_scale,
            RD_[size_t(nl - 1)].get());
  for (int l = nl - 1; l >= 0; --l) {
    const Layer &L = layers_[size_t(l)];
    float *dst = Hv + L.off;
    const long long seg = (long long)(L.in + 1) * L.out;
    rpass_weight_grad(B, l, l == 0 ? X : A_[size_t(l - 1)].get(), l == 0 ? idx : nullptr, true, RD_[size_t(l)].get(),
                      dst);
    if (l > 0) {
      rpass_weight_grad(B, l, RA_[size_t(l - 1)].get(), nullptr, false, D_[size_t(l)].get(), seg_.get());
      lincomb(s, seg, dst, 1.0, seg_.get(), dst);
      const int pa = layers_[size_t(l - 1)].act;
      rpass_back_prod(B, l, RD_[size_t(l)].get(), P, pa, T1_.get());
      rpass_back_prod(B, l, D_[size_t(l)].get(), V, pa, T2_.get());
      rop_back(s, B * L.in, T1_.get(), T2_.get(), act_has_d2(pa) ? DL_[size_t(l - 1)].get() : nullptr,
               A_[size_t(l - 1)].get(), RZ_[size_t(l - 1)].get(), pa, RD_[size_t(l - 1)].get());
    }
  }
  curv_finish(Hv, lambda, V, nullptr);
}

// Gauss-Newton vector product Gv = J^T H_L J V (+ lambda V) of the same batch loss (hvp.hip has the
// definition): the forward, the R-forward of hvp with the sum and act' fused into one elementwise launch,
// the convex loss's Hessian applied to R{Z_L}, and an ordinary backward pass from that output delta. No
// out_loss, no plain backward, no second-order products: a subset of hvp's GEMMs on hvp's workspace.
void Mlp::gnvp(const float *P, const float *V, const float *X, const float *Y, const int *idx, long long B,
               double inv_scale, double lambda, float *Gv) {
  LBF_REQUIRE(P && V && Gv && B >= 0 && (B == 0 || (X && Y)), "gnvp: bad argument");
  gn_prepare(P, X, idx, B);
  gn_apply(P, V, X, Y, idx, B, inv_scale, lambda, Gv);
}

void Mlp::gn_prepare(const float *P, const float *X, const int *idx, long long B) {
  if (B == 0) return; // an empty share has no activations
  ensure(B);
  rpass_ensure(B);
  forward(P, X, idx, B, int(layers_.size()));
}

void Mlp::gn_apply(const float *P, const float *V, const float *X, const float *Y, const int *idx, long long B,
                   double inv_scale, double lambda, float *Gv) {
  hipStream_t s = ctx_->stream;
  const int nl = int(layers_.size());
  const int *ab = ctx_->abort;
  if (B == 0) return curv_empty(Gv, lambda, V, ab);
  // ---- R-forward: T0 = A_{l-1} V_l + v_l in RZ_[l], T1 = R{A_{l-1}} W_l in T1_; only R{A_l} is kept ----
  const Layer &Lo = layers_[size_t(nl - 1)];
  for (int l = 0; l < nl; ++l) {
    const Layer &L = layers_[size_t(l)];
    float *t0 = RZ_[size_t(l)].get(), *t1 = nullptr;
    if (l == 0) {
      rpass_linear_fwd(B, 0, V, X, idx, true, t0); // X V_0 + v_0
    } else {
      t1 = T1_.get();
      rpass_linear_fwd(B, l, V, A_[size_t(l - 1)].get(), nullptr, true, t0);   // A V_l + v_l
      rpass_linear_fwd(B, l, P, RA_[size_t(l - 1)].get(), nullptr, false, t1); // R{A} W_l
    }
    // ---- the loss's Hessian on R{Z_L}: the output delta M_L of the backward pass ----
    if (l == nl - 1) {
      if (loss_ == LOSS_XENT)
        gn_out_xent(s, B, Lo.out, A_[size_t(l)].get(), Y, idx, t0, t1, inv_scale, RD_[size_t(l)].get(), ab);
      else
        gn_out_mse(s, B * Lo.out, A_[size_t(l)].get(), t0, t1, Lo.act, inv_scale, RD_[size_t(l)].get(), ab);
    } else {
      gn_act(s, B * L.out, A_[size_t(l)].get(), t0, t1, L.act, RA_[size_t(l)].get(), ab);
    }
  }
  // ---- backward: (G v)_l = [A_{l-1} | 1]^T M_l, M_{l-1} = (M_l W_l^T) .* act'(A_{l-1}) ----
  for (int l = nl - 1; l >= 0; --l) {
    rpass_weight_grad(B, l, l == 0 ? X : A_[size_t(l - 1)].get(), l == 0 ? idx : nullptr, true, RD_[size_t(l)].get(),
                      Gv + layers_[size_t(l)].off);
    if (l > 0) rpass_back_prod(B, l, RD_[size_t(l)].get(), P, layers_[size_t(l - 1)].act, RD_[size_t(l - 1)].get());
  }
  curv_finish(Gv, lambda, V, ab);
}

// Sum of squared per-example gradients (fisher.hip): the plain backward pass of hvp with the [dW ; db]
// GEMM replaced by the squared product. The deltas are taken at inv_scale = 1 and the scale is applied where the
// slabs are summed: squares of deltas pre-scaled by 1 / 60000 would sit needlessly close to the fp32 denormals.
void Mlp::grad_sq(const float *P, const float *X, const float *Y, const int *idx, long long B, double scale,
                  float *out) {
  LBF_REQUIRE(P && out && B >= 0 && (B == 0 || (X && Y)), "grad_sq: bad argument");
  LBF_REQUIRE(std::isfinite(scale) && scale >= 0.0, "grad_sq: scale must be finite and >= 0");
  hipStream_t s = ctx_->stream;
  const int nl = int(layers_.size());
  if (B == 0) return curv_empty(out, 0.0, nullptr, nullptr);
  gn_prepare(P, X, idx, B);
  size_t slab = 1;
  for (const Layer &L : layers_) slab = std::max(slab, size_t(grad_sq_splits(B, L.in, L.out)) * size_t(L.in + 1) * L.out);
  gsq_slab_.ensure(slab);
  out_loss(Y, idx, B, 1.0);
  for (int l = nl - 1; l >= 0; --l) {
    const Layer &L = layers_[size_t(l)];
    grad_sq_layer(s, l == 0 ? X : A_[size_t(l - 1)].get(), L.in, l == 0 ? idx : nullptr, D_[size_t(l)].get(), L.out, B,
                  scale, gsq_slab_.get(), out + L.off);
    if (l > 0) rpass_back_prod(B, l, D_[size_t(l)].get(), P, layers_[size_t(l - 1)].act, D_[size_t(l - 1)].get());
  }
  curv_finish(out, 0.0, nullptr, nullptr);
}

// Gauss-Newton conjugate gradients (cg.hip). Every launch of an iteration takes the solver's abort
// word through ctx_->abort, so the iterations enqueued past the stopping one change nothing: x, r and the status
// block stay bitwise what the stopping iteration left, whatever `check` is. Under a communicator a frozen
// iteration still joins its all-reduce; Ap is zeroed in front of every product there, so what the frozen
// collectives sum in place is zeros (a live product overwrites every element of Ap).
void Mlp::gn_cg(const float *P, const float *b, float bscale, const float *X, const float *Y, const int *idx,
                long long B, double inv_scale, double damping, int max_iters, double rtol, int check, float *x,
                CgInfo *info, const float *minv) {
  LBF_REQUIRE(P && b && x && B >= 0 && (B == 0 || (X && Y)), "gn_cg: bad argument");
  LBF_REQUIRE(max_iters >= 0 && rtol >= 0.0 && check >= 1, "gn_cg: max_iters >= 0, rtol >= 0, check >= 1");
  hipStream_t s = ctx_->stream;
  const long long n = (long long)nparams_;
  const int nwg = cg_nwg(n);
  cg_r_.ensure(size_t(n));
  cg_p_.ensure(size_t(n));
  cg_ap_.ensure(size_t(n));
  cg_part_.ensure(size_t(8) * size_t(nwg));
  cg_st_.ensure(CG_N);
  cg_abort_.ensure(1);
  cg_hst_.ensure(CG_N);
  CgArgs a;
  a.n = n;
  a.x = x;
  a.r = cg_r_.get();
  a.p = cg_p_.get();
  a.Ap = cg_ap_.get();
  a.b = b;
  a.bscale = bscale;
  a.pap = cg_part_.get();
  a.rr = cg_part_.get() + nwg;
  a.xd = cg_part_.get() + 3 * size_t(nwg);
  a.minv = minv;
  a.rz = cg_part_.get() + 6 * size_t(nwg);
  a.st = cg_st_.get();
  a.abort = cg_abort_.get();
  a.max_iters = max_iters;
  a.tol2 = rtol * rtol;
  AbortScope scope{ctx_, ctx_->abort};
  LBF_HIP(hipMemsetAsync(cg_abort_.get(), 0, sizeof(int), s));
  ctx_->abort = cg_abort_.get();
  gn_prepare(P, X, idx, B);
  cg_init(s, a);
  double *hst = cg_hst_.get();
  auto read_status = [&]() {
    LBF_HIP(hipMemcpyAsync(hst, cg_st_.get(), CG_N * sizeof(double), hipMemcpyDeviceToHost, s));
    LBF_HIP(hipStreamSynchronize(s));
  };
  int k = 0;
  for (;;) {
    const int m = std::min(check, max_iters - k);
    for (int i = 0; i < m; ++i, ++k) {
      if (ctx_->dp() && B > 0) zero_fill(s, n, cg_ap_.get());
      gn_apply(P, a.p, X, Y, idx, B, inv_scale, damping, cg_ap_.get());
      cg_pap(s, a);
      cg_step(s, a, k);
      cg_dir(s, a, k);
    }
    read_status();
    if (int(hst[CG_STATUS]) != CG_RUNNING || k >= max_iters) break;
  }
  ctx_->abort = scope.prev;
  LBF_HIP(hipMemsetAsync(cg_abort_.get(), 0, sizeof(int), s));
  cg_xdots(s, a);
  read_status();
  if (info) {
    info->iterations = int(hst[CG_ITER]);
    info->status = int(hst[CG_STATUS]) == CG_RUNNING ? int(CG_MAXITER) : int(hst[CG_STATUS]); // max_iters == 0
    info->rr0 = hst[CG_RR0];
    info->rr = hst[CG_RR];
    info->xb = hst[CG_XB];
    info->xr = hst[CG_XR];
    info->xx = hst[CG_XX];
  }
}

// Lanczos on H + l2 I or G + l2 I (lanczos.hip), enqueued ahead like gn_cg: every launch of a step takes
// the run's abort word, so the steps enqueued past a stop change nothing and the result does not depend on `check`.
// Under a communicator a frozen step still joins its all-reduce, so w is zeroed in front of every product there.
// gn_apply is frozen as a whole and the collective sums zeros. Of hvp the GEMMs and the slab sums are frozen (they
// take ctx->abort), its elementwise launches are not: its `dst += seg_` adds one stale segment to the zeros, so the
// collective sums at most that, the same on every step, and w cannot grow from one frozen step to the next. No
// launch of the run reads w after the stop.
void Mlp::lanczos(const float *P, const float *v0, const float *X, const float *Y, const int *idx, long long B,
                  double inv_scale, double l2, bool exact, int steps, bool reorth, int check, double breakdown_rtol,
                  double *h_alpha, double *h_beta, float *basis, long long ld, LanczosInfo *info) {
  const long long n = (long long)nparams_;
  LBF_REQUIRE(P && v0 && h_alpha && h_beta && B >= 0 && (B == 0 || (X && Y)), "lanczos: bad argument");
  LBF_REQUIRE(steps >= 1 && steps <= LZ_MAX_STEPS && check >= 1, "lanczos: steps in 1..128, check >= 1");
  LBF_REQUIRE(std::isfinite(l2) && l2 >= 0.0 && std::isfinite(breakdown_rtol) && breakdown_rtol >= 0.0,
              "lanczos: l2 and breakdown_rtol must be finite and >= 0");
  LBF_REQUIRE(!basis || ld >= n, "lanczos: ld < parameter count");
  hipStream_t s = ctx_->stream;
  const int nwg = cg_nwg(n);
  // the rows the run reads: the caller's basis, or a workspace of steps + 1 rows (reorth) or a ring of three
  const int ring = reorth ? 0 : 3;
  float *Q = basis;
  long long qld = ld;
  if (!reorth || !basis) {
    qld = round4(n);
    lz_q_.ensure(size_t(reorth ? steps + 1 : 3) * size_t(qld));
    Q = lz_q_.get();
  }
  float *out = reorth ? nullptr : basis; // reorth = 0 with a basis: every q_j is also copied out
  auto row = [&](int j) { return Q + size_t(ring ? j % ring : j) * size_t(qld); };
  auto out_row = [&](int j) { return out ? out + size_t(j) * size_t(ld) : nullptr; };
  lz_w_.ensure(size_t(n));
  lz_part_.ensure(2 * lz_pass_words(n) + size_t(nwg));
  lz_st_.ensure(LZ_N);
  lz_abort_.ensure(1);
  lz_hst_.ensure(LZ_N);
  LzArgs a;
  a.n = n;
  a.w = lz_w_.get();
  a.tab = lz_part_.get();
  a.wwtab = lz_part_.get() + 2 * lz_pass_words(n);
  a.st = lz_st_.get();
  a.abort = lz_abort_.get();
  a.steps = steps;
  a.breakdown_rtol = breakdown_rtol;
  AbortScope scope{ctx_, ctx_->abort};
  LBF_HIP(hipMemsetAsync(lz_abort_.get(), 0, sizeof(int), s));
  LBF_HIP(hipMemsetAsync(lz_st_.get(), 0, LZ_N * sizeof(double), s));
  ctx_->abort = lz_abort_.get();
  if (!exact) gn_prepare(P, X, idx, B);
  lz_start(s, a, v0, row(0), out_row(0));
  double *hst = lz_hst_.get();
  const int npass = reorth ? 2 : 1;
  int j = 0;
  for (;;) {
    const int m = std::min(check, steps - j);
    for (int i = 0; i < m; ++i, ++j) {
      if (ctx_->dp() && B > 0) zero_fill(s, n, a.w);
      if (exact) {
        hvp(P, row(j), X, Y, idx, B, inv_scale, l2, a.w);
      } else {
        gn_apply(P, row(j), X, Y, idx, B, inv_scale, l2, a.w);
      }
      LzRows R;
      R.Q = Q;
      R.ld = qld;
      R.ring = ring;
      const int r0 = reorth ? 0 : std::max(0, j - 1);
      R.slot0 = ring ? r0 % ring : r0;
      R.nrows = j - r0 + 1;
      for (int p = 0; p < npass; ++p) lz_orth(s, a, R, p, p + 1 == npass);
      lz_finish(s, a, j, npass, j - r0, row(j + 1), out_row(j + 1));
    }
    LBF_HIP(hipMemcpyAsync(hst, lz_st_.get(), LZ_N * sizeof(double), hipMemcpyDeviceToHost, s));
    LBF_HIP(hipStreamSynchronize(s));
    if (int(hst[LZ_STATUS]) != LZ_RUNNING || j >= steps) break;
  }
  const int done = int(hst[LZ_STEPS]);
  for (int i = 0; i < steps; ++i) {
    h_alpha[i] = i < done ? hst[LZ_ALPHA + i] : 0.0;
    h_beta[i] = i < done ? hst[LZ_BETA + i] : 0.0;
  }
  if (info) {
    info->steps = done;
    info->status = int(hst[LZ_STATUS]);
    info->v0_norm = hst[LZ_V0NORM];
  }
}

} // namespace lbf
