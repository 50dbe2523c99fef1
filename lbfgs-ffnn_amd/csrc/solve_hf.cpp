// Hessian-free driver (solvers.hpp run_hf): truncated Newton with the Gauss-Newton matrix (Martens 2010). The step
// solves (G + (l2 + lambda) I) p = -g by device-side CG (Mlp::gn_cg, one forward pass per solve); the host sees one
// status block per `cg_check` CG iterations and one loss per line-search trial. Every decision is taken on the
// host from fp64 words that are all-reduced (or replicated) under a communicator, so the ranks agree.
#include "solvers.hpp"

#include <algorithm>
#include <cmath>

// Host-side acceptance tests must round like ls_ctl_kernel (and the reference's host code).
#pragma clang fp contract(off)

namespace lbf {

// Preconditioned (pc, mode LBF_PRECOND_GRAD_SQ): D = sum of squared per-example gradients of the
// curvature rows (Mlp::grad_sq, all-reduced, refreshed every pc->refresh iterations), minv = (cinv D + l2 +
// lambda_k)^(-exponent) every iteration, and the CG is Mlp::gn_cg's preconditioned form. Nothing else changes: q,
// the ratio, the damping rule and the line search use x.b, x.r and x.x only.
int run_hf(Mlp *net, const lbf_hf_params &prm, float *d_params, const float *X, const float *Y, long long n_local,
           long long n_global, lbf_record *rec, lbf_solve_info *info, const lbf_hf_precond *pc) {
  LBF_REQUIRE(d_params && n_local >= 0 && n_global > 0 && (n_local == 0 || (X && Y)), "bad argument");
  LBF_REQUIRE(prm.max_iters >= 0 && prm.cg_iters >= 0 && prm.cg_rtol >= 0.0 && prm.cg_check >= 1 &&
                  prm.max_line_iters >= 1 && prm.damping0 >= 0.0 && prm.rho > 0.0 && prm.rho < 1.0,
              "hf: bad parameter");
  Ctx *c = net->ctx();
  LBF_REQUIRE(prm.curv_rows >= 0 && prm.curv_rows <= n_local, "hf: curv_rows must lie in [0, n_local]");
  LBF_REQUIRE(prm.curv_rows == 0 || !c->comm, "hf: curv_rows > 0 runs on one rank (the window has no shard split)");
  if (pc) {
    LBF_REQUIRE(pc->mode == LBF_PRECOND_NONE || pc->mode == LBF_PRECOND_GRAD_SQ, "hf: unknown preconditioner mode");
    LBF_REQUIRE(pc->exponent >= 0.0 && pc->exponent <= 1.0, "hf: preconditioner exponent must lie in [0, 1]");
    LBF_REQUIRE(pc->refresh >= 1, "hf: preconditioner refresh must be >= 1");
  }
  const bool pcon = pc && pc->mode == LBF_PRECOND_GRAD_SQ;
  c->set_device();
  hipStream_t s = c->stream;
  const long long n = (long long)net->nparams();
  const int In = net->layers().front().in, Out = net->layers().back().out;
  const int nww = ww_partials_n(n);
  DevBuf<float> g(size_t(round4(n + 2))), p(size_t(std::max(1LL, n))), trial(size_t(std::max(1LL, n)));
  DevBuf<double> scal(SC_N), wwp{size_t(nww)};
  DevBuf<float> dsq(size_t(pcon ? std::max(1LL, n) : 0)), minv(size_t(pcon ? std::max(1LL, n) : 0));
  StatusMirror hs;
  const SolveCounters<Mlp> cnt(net);
  const double l2 = net->l2(), inv = 1.0 / double(n_global);
  auto eval = [&]() {
    net->loss_grad(d_params, g.get(), X, Y, nullptr, n_local, inv, l2, nullptr, scal.get());
    hs.read(s, scal.get());
  };
  double lam = prm.damping0;
  const auto t0 = std::chrono::steady_clock::now();
  RecordWriter rw(rec);
  int done = 0;
  eval();
  for (int it = 0; it < prm.max_iters; ++it) {
    const double f = hs[SC_LOSS], gnorm = std::sqrt(hs[SC_TGG]);
    if (gnorm < prm.tol || !(hs[SC_TGG] > 0.0)) break;
    // ---- the step: CG on the curvature rows ----
    const float *Xc = X, *Yc = Y;
    long long Bc = n_local;
    double cinv = inv;
    if (prm.curv_rows > 0) {
      const long long off = ((long long)it * prm.curv_rows) % (n_local - prm.curv_rows + 1);
      Xc = X + off * In;
      Yc = Y + off * Out;
      Bc = prm.curv_rows;
      cinv = 1.0 / double(prm.curv_rows);
    }
    Mlp::CgInfo ci;
    if (pcon) {
      if (it % pc->refresh == 0) net->grad_sq(d_params, Xc, Yc, nullptr, Bc, cinv, dsq.get());
      precond_minv(s, n, dsq.get(), l2 + lam, pc->exponent, minv.get());
    }
    net->gn_cg(d_params, g.get(), -1.0f, Xc, Yc, nullptr, Bc, cinv, l2 + lam, prm.cg_iters, prm.cg_rtol, prm.cg_check,
               p.get(), &ci, pcon ? minv.get() : nullptr);
    const double q = -0.5 * (ci.xb + ci.xr) - 0.5 * lam * ci.xx; // g.p + 0.5 p^T (G + l2 I) p
    const double gp = -ci.xb;
    // ---- backtracking on the full objective ----
    double alpha = 1.0, f1 = f;
    int trials = 0, accepted = 0;
    for (int t = 0; t < prm.max_line_iters; ++t) {
      axpy_to(s, n, d_params, float(alpha), p.get(), trial.get(), wwp.get());
      net->loss_only(trial.get(), X, Y, nullptr, n_local, inv, scal.get(), l2, WwPart{wwp.get(), nww});
      hs.read(s, scal.get());
      const double ft = hs[SC_LOSS];
      if (t == 0) f1 = ft;
      ++trials;
      if (ft <= f + prm.c1 * alpha * gp) {
        accepted = 1;
        break;
      }
      alpha *= prm.rho;
    }
    if (accepted) LBF_HIP(hipMemcpyAsync(d_params, trial.get(), size_t(n) * sizeof(float), hipMemcpyDeviceToDevice, s));
    // ---- Levenberg-Marquardt damping from the first trial's reduction ratio ----
    const double ratio = q < 0.0 ? (f1 - f) / q : 0.0; // no model decrease (a CG breakdown at x = 0): damp more
    if (ratio < prm.ratio_lo) lam *= prm.damp_up;
    else if (ratio > prm.ratio_hi) lam *= prm.damp_down;
    if (it < prm.trace_cap) {
      if (prm.damping_trace) prm.damping_trace[it] = lam;
      if (prm.ratio_trace) prm.ratio_trace[it] = ratio;
      if (prm.cg_trace) prm.cg_trace[it] = ci.iterations;
    }
    rw.put(f, gnorm, ms_since(t0), accepted ? alpha : 0.0, trials, accepted); // alpha 0: the search failed
    ++done;
    eval(); // the next iteration's f and g; after the last one, the final point's
  }
  cnt.fill(info, done, hs[SC_LOSS], std::sqrt(hs[SC_TGG]));
  return done;
}

} // namespace lbf
