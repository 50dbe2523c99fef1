// OWL-QN driver (solvers.hpp run_owlqn; Andrew & Gao 2007): L-BFGS on F = f + l1 |w|_1, f the smooth objective of
// run_gd. The two-loop is the History's, fed the pseudo-gradient as the vector and the smooth gradients as the pair;
// the orthant machinery is owlqn.hip's two sweeps. The host reads one status block per trial (the loss-only
// evaluation's and the trial sweep's words in one synchronisation) and takes every decision from fp64 words that are
// the same on every rank.
#include "solvers.hpp"

#include <algorithm>
#include <cmath>

// Host-side acceptance tests must round like ls_ctl_kernel (and the reference's host code).
#pragma clang fp contract(off)

namespace lbf {

OwlCoef owl_coef(const Mlp &net, double l1, int l1_bias) {
  OwlCoef c;
  c.c = float(l1);
  if (l1_bias) return c;
  for (const Layer &L : net.layers()) { // a layer's segment is [W (in x out) | b (out)]
    LBF_REQUIRE(c.nfree < OWL_MAXFREE, "owlqn: too many layers");
    c.f0[c.nfree] = (long long)L.off + (long long)L.in * L.out;
    c.f1[c.nfree] = (long long)L.off + (long long)(L.in + 1) * L.out;
    ++c.nfree;
  }
  return c;
}

long long owl_penalised_count(const Mlp &net, int l1_bias) {
  long long k = (long long)net.nparams();
  if (!l1_bias)
    for (const Layer &L : net.layers()) k -= L.out;
  return k;
}

int run_owlqn(Mlp *net, const lbf_owlqn_params &prm, float *d_params, const float *X, const float *Y,
              long long n_local, long long n_global, lbf_record *rec, lbf_solve_info *info, lbf_owlqn_stats *stats) {
  LBF_REQUIRE(d_params && n_local >= 0 && n_global > 0 && (n_local == 0 || (X && Y)), "bad argument");
  LBF_REQUIRE(std::isfinite(prm.l1) && prm.l1 >= 0.0, "owlqn: l1 must be finite and >= 0");
  LBF_REQUIRE(prm.m >= 0 && prm.m <= 128 && prm.max_iters >= 0 && prm.rho > 0.0 && prm.rho < 1.0 &&
                  prm.max_line_iters >= 1,
              "owlqn: bad parameter");
  Ctx *c = net->ctx();
  c->set_device();
  hipStream_t s = c->stream;
  const long long n = (long long)net->nparams();
  const int nww = ww_partials_n(n);
  std::unique_ptr<History> hist; // m == 0: no ring, the direction is -pg (formed inside the trial sweep)
  if (prm.m > 0) hist.reset(new History(c, prm.m, n, read_switches().gram_fin));
  DevBuf<float> xbuf[2], gbuf[2], pg(size_t(round4(n))), d(size_t(hist ? round4(n) : 0));
  for (int i = 0; i < 2; ++i) {
    xbuf[i].resize(size_t(round4(n)));
    gbuf[i].resize(size_t(round4(n + 2)));
  }
  float *x = xbuf[0].get(), *xt = xbuf[1].get(), *g = gbuf[0].get(), *gt = gbuf[1].get();
  DevBuf<double> scal(SC_N), tab{size_t(owl_table_words(n))}, st(OWL_N);
  StatusMirror hs;
  PinnedBuf<double> ho;
  ho.ensure(OWL_N);
  const SolveCounters<Mlp> cnt(net);
  const double l2 = net->l2(), inv = 1.0 / double(n_global);
  OwlArgs oa;
  oa.n = n;
  oa.coef = owl_coef(*net, prm.l1, prm.l1_bias);
  oa.l1 = prm.l1;
  oa.tab = tab.get();
  oa.st = st.get();
  auto read_status = [&]() { // the evaluation's and the sweep's words, one synchronisation
    hs.enqueue(s, scal.get());
    LBF_HIP(hipMemcpyAsync(ho.get(), st.get(), OWL_N * sizeof(double), hipMemcpyDeviceToHost, s));
    LBF_HIP(hipStreamSynchronize(s));
  };
  auto pseudo = [&]() { // pg and its words at (x, g)
    OwlArgs a = oa;
    a.x = x;
    a.g = g;
    a.out = pg.get();
    {
      ProfScope ps(c, PK_OWL_PSEUDO);
      owl_pseudo(s, a);
    }
    owl_pseudo_finish(s, a);
  };
  LBF_HIP(hipMemcpyAsync(x, d_params, size_t(n) * sizeof(float), hipMemcpyDeviceToDevice, s));
  net->loss_grad(x, g, X, Y, nullptr, n_local, inv, l2, nullptr, scal.get());
  pseudo();
  read_status();
  double F = hs[SC_LOSS] + ho[OWL_L1], pgg = ho[OWL_PGPG], zeros = ho[OWL_ZEROS], l1x = ho[OWL_L1];
  bool pair = false; // (xt, gt) hold the previous point and gradient of a pair not yet in the ring
  const auto t0 = std::chrono::steady_clock::now();
  RecordWriter rw(rec);
  int done = 0;
  for (int it = 0; it < prm.max_iters; ++it) {
    const double pgn = std::sqrt(pgg);
    if (pgn < prm.tol || !(pgg > 0.0)) break;
    // ---- direction: the ring takes the pair of smooth gradients, the two-loop runs on pg ----
    if (hist) {
      GramArgs ga;
      ga.policy = POL_CPU; // y.s > 1e-10, gamma = s.y / y.y, no descent fallback (the sign test replaces it)
      ga.has_g = 1;
      ga.ga = pg.get();
      if (pair) {
        ga.has_pair = 1;
        ga.sa = x;
        ga.sb = xt;
        ga.ya = g;
        ga.yb = gt;
      }
      hist->update(ga, 1, it, -1.0);
      hist->combine(pg.get(), d.get(), nullptr, nullptr, nullptr, false, 0.0);
      pair = false;
    }
    // ---- backtracking on the projected trial points ----
    double alpha = it == 0 ? std::min(1.0, 1.0 / pgn) : 1.0, Ft = F, zt = zeros;
    int trials = 0, accepted = 0;
    for (int t = 0; t < prm.max_line_iters; ++t) {
      OwlArgs a = oa;
      a.x = x;
      a.d = hist ? d.get() : nullptr;
      a.pg = pg.get();
      a.alpha = float(alpha);
      a.out = xt;
      {
        ProfScope ps(c, PK_OWL_TRIAL);
        owl_trial(s, a);
      }
      owl_trial_finish(s, a);
      net->loss_only(xt, X, Y, nullptr, n_local, inv, scal.get(), l2, WwPart{tab.get(), nww});
      read_status();
      Ft = hs[SC_LOSS] + ho[OWL_L1];
      zt = ho[OWL_ZEROS];
      ++trials;
      if (Ft <= F + prm.c1 * ho[OWL_DEC]) {
        accepted = 1;
        break;
      }
      alpha *= prm.rho;
    }
    rw.put(F, pgn, ms_since(t0), accepted ? alpha : 0.0, trials, accepted); // alpha 0: the search failed
    ++done;
    if (accepted) {
      // the gradient from the accepted trial's forward state; the w.w table is still the trial sweep's
      net->grad_after_loss(xt, gt, X, nullptr, n_local, inv, l2, nullptr, scal.get(), nullptr, WwPart{tab.get(), nww});
      std::swap(x, xt);
      std::swap(g, gt);
      pair = prm.m > 0;
      pseudo();
      read_status();
      F = Ft;
      zeros = zt;
      pgg = ho[OWL_PGPG];
      l1x = ho[OWL_L1];
    }
    if (prm.zeros_trace && it < prm.trace_cap) prm.zeros_trace[it] = (long long)zeros;
    if (!accepted) break; // nothing changed: the next iteration would be this one again
  }
  LBF_HIP(hipMemcpyAsync(d_params, x, size_t(n) * sizeof(float), hipMemcpyDeviceToDevice, s));
  LBF_HIP(hipStreamSynchronize(s));
  cnt.fill(info, done, F, std::sqrt(pgg));
  if (stats) {
    stats->zeros = (long long)zeros;
    stats->penalised = owl_penalised_count(*net, prm.l1_bias);
    stats->l1_term = l1x;
    stats->pg_norm = std::sqrt(pgg);
  }
  return done;
}

} // namespace lbf
