// Device-resident L-BFGS history (see runtime.hpp).
#include "runtime.hpp"

#include <algorithm>

namespace lbf {

History::History(Ctx *ctx, int m, long long n, int gram_fin) : ctx_(ctx) {
  LBF_REQUIRE(m >= 0 && m <= 128, "history size m must be in [0, 128]");
  const int slots = m + 1;
  // Slot stride n rounded to 4 floats. (Rounded up to 2 MiB, the many-stream reads of the old combine pattern went
  // 5.45 -> 5.88 TB/s in profiles/micro/ring_ld.hip, but the Gram sweep slowed 5.43 -> 5.25 TB/s at n = 10.49M and the
  // chunked combine below needs no help: 65.4-65.7 % against 65.9-66.0 % of HBM at m = 50, profiles/r06/f/.)
  const long long ld = cdiv(n, 4) * 4;
  S_.resize(size_t(slots) * ld);
  Y_.resize(size_t(slots) * ld);
  ist_.resize(IST_ORDER + slots + 4);
  // dstate: rho | SS | SY | YY | gS | gY | coef(2*slots+1) | scal
  const size_t nd = slots + 3 * size_t(slots) * slots + 2 * slots + (2 * slots + 1) + SC_N;
  dstate_.resize(nd);
  part_.resize(size_t(gram_nwg(n)) * gram_ncols(m));
  red_.resize(size_t(kGramFold) * gram_ncols(m));
  v_.m = m;
  v_.slots = slots;
  v_.n = n;
  v_.ld = ld;
  v_.S = S_.get();
  v_.Y = Y_.get();
  v_.ist = ist_.get();
  double *p = dstate_.get();
  v_.rho = p;
  p += slots;
  v_.SS = p;
  p += size_t(slots) * slots;
  v_.SY = p;
  p += size_t(slots) * slots;
  v_.YY = p;
  p += size_t(slots) * slots;
  v_.gS = p;
  p += slots;
  v_.gY = p;
  p += slots;
  v_.coef = p;
  p += 2 * slots + 1;
  v_.scal = p;
  LBF_HIP(hipMemsetAsync(ist_.get(), 0, ist_.size() * sizeof(int), ctx_->stream));
  LBF_HIP(hipMemsetAsync(dstate_.get(), 0, dstate_.size() * sizeof(double), ctx_->stream));
  // the ring vectors are only ever read for live slots, but keep them defined
  LBF_HIP(hipMemsetAsync(S_.get(), 0, S_.size() * sizeof(float), ctx_->stream));
  LBF_HIP(hipMemsetAsync(Y_.get(), 0, Y_.size() * sizeof(float), ctx_->stream));
  dir_on_ = dir_supported(m, n);
  if (dir_on_) {
    const int nb = int(cdiv(n, dir_cols_per_block(m, n)));
    drows_.resize(size_t(dir_ncols(m)) * size_t(nb));
    ddots_.resize(size_t(dir_ncols(m)));
    dkmat_.resize(size_t(DIR_KMAT_N));
    LBF_HIP(hipMemsetAsync(dkmat_.get(), 0, dkmat_.size() * sizeof(double), ctx_->stream));
    dcount_.resize(1);
    LBF_HIP(hipMemsetAsync(dcount_.get(), 0, sizeof(unsigned), ctx_->stream));
  }
  // Column sums + last-block step (gram_fin) for short histories; for m > 20 the fold_rows + hist_step route, which
  // measured faster there (two-loop at n = 10.49M: m = 10 58.0 against 57.5 %, m = 50 67.7 against 68.1 %,
  // profiles/r06/j/). gram_fin = 1 / 0 (LBF_GRAM_FIN) forces either route (tests compare them).
  gfin_on_ = gram_fin_supported(m) && (gram_fin == 1 || (gram_fin < 0 && m <= 20));
  if (gfin_on_) {
    gdots_.resize(size_t(gram_ncols(m)));
    gcount_.resize(1);
    LBF_HIP(hipMemsetAsync(gcount_.get(), 0, sizeof(unsigned), ctx_->stream));
  }
}

void History::reset() { hist_reset(ctx_->stream, v_); }

bool History::update_impl(const GramArgs &g0, int want_dir, int iter, double dsign, const RedAllArgs *gred,
                          const CombineArgs *cmb) {
  GramArgs g = g0;
  g.h = v_;
  g.h.abort = ctx_->abort;
  hipStream_t s = ctx_->stream;
  const bool aligned = aligned16(g.sa, g.sb, g.ya, g.yb, g.ga, g.gb, g.gc, g.g_out); // 16-B lanes in dir_sweep
  const bool defer = gred && gred->nseg > 0;
  const bool dir = dir_on_ && aligned && g.policy == POL_SLBFGS && (want_dir == 0 || want_dir == 1);
  // the sweep reads a lane's four columns of a segment's slabs as one 16-B load per split
  bool quads = true;
  for (int i = 0; defer && i < gred->nseg; ++i) {
    const RedSeg &S = gred->seg[i];
    quads = quads && S.goff % 4 == 0 && S.parts == 1 &&
            (S.splits == 0 || (S.count % 4 == 0 && S.stride % 4 == 0 && aligned16(S.slab)));
  }
  const bool in_sweep = defer && dir && quads && g.has_g && !g.has_pair && gred->G == g.ga;
  if (defer && !in_sweep) { // only the fused sweep finishes deferred slabs
    ProfScope ps(ctx_, PK_SLAB, 0);
    reduce_all(s, *gred);
  }
  if (dir) {
    // S-LBFGS: sweep + column sums whose last block runs the step (dir.hip), two launches instead of
    // gram -> fold -> hist_step
    DirArgs d;
    d.g = g;
    if (in_sweep) { // g.ga finished inside the sweep from its split-K slabs
      d.gred = *gred;
      d.gred_on = 1;
    }
    d.want_dir = want_dir;
    d.iter = iter;
    d.dsign = dsign;
    d.rows = drows_.get();
    d.dots = ddots_.get();
    d.nb = int(cdiv(v_.n, dir_cols_per_block(v_.m, v_.n)));
    d.cols_done = dcount_.get();
    d.kmat = dkmat_.get();
    {
      ProfScope ps(ctx_, PK_GRAM);
      dir_sweep(s, d);
    }
    if (cmb && dir_combine_supported(d, *cmb)) {
      // direction-only step: column sums, then the coefficients computed in every block of the combine
      ProfScope ps(ctx_, PK_COMBINE);
      dir_cols_combine(s, d, *cmb);
      return true;
    }
    ProfScope ps(ctx_, PK_COEF);
    dir_fin(s, d);
    return false;
  }
  if (gfin_on_ && (want_dir == 0 || want_dir == 1)) {
    // Gram sweep with transposed partials, then one block per column whose last arrival runs the step:
    // two launches instead of gram -> fold_rows -> hist_step
    DirArgs d;
    d.g = g;
    d.want_dir = want_dir;
    d.iter = iter;
    d.dsign = dsign;
    d.rows = part_.get();
    d.dots = gdots_.get();
    d.nb = gram_nwg(v_.n);
    d.cols_done = gcount_.get();
    // the sweep's partial rows stored row-major (one contiguous row per workgroup): its transposed stores, three
    // scattered doubles per history vector per workgroup, cost the sweep 13 % in profiles/micro/ring_ld.hip
    // (gram3_tr1 / tr0) and 5.44 against 5.59 TB/s in the engine (LBF_GRAM_FIN=1 / 0, profiles/r06/i/)
    d.row_major = 1;
    {
      ProfScope ps(ctx_, PK_GRAM);
      gram_update(s, g, part_.get(), 0);
    }
    ProfScope ps(ctx_, PK_COEF);
    gram_fin(s, d);
    return false;
  }
  {
    ProfScope ps(ctx_, PK_GRAM);
    gram_update(s, g, part_.get());
  }
  CoefArgs c;
  c.h = v_;
  c.h.abort = ctx_->abort;
  c.partials = part_.get();
  c.nwg = gram_nwg(v_.n);
  // tall partial table (large n, or a large m whose rows fill the step's staging area): fold it on many
  // blocks first, so the single-workgroup history step reads one staging round of rows, not thousands
  const int fold_to = std::min(kGramFold, hist_stage_rows(v_.m));
  if (c.nwg > 2 * fold_to) {
    ProfScope pf(ctx_, PK_COEF);
    c.nwg = fold_rows(s, part_.get(), c.nwg, gram_ncols(v_.m), fold_to, red_.get());
    c.partials = red_.get();
  }
  c.has_pair = g.has_pair;
  c.has_g = g.has_g;
  c.reset = g.reset;
  c.policy = g.policy;
  c.want_dir = want_dir;
  c.iter = iter;
  c.dsign = dsign;
  ProfScope ps(ctx_, PK_COEF);
  hist_coef(s, c);
  return false;
}

bool History::update_combine(const GramArgs &g0, int iter, double dsign, const float *x_in, float *x_out,
                             float *x_out2, double alpha, const RedAllArgs *gred) {
  // (the combine inside the column-sum launch measured slower: its waiting blocks slowed the column sums
  // and the one-block step, profiles/r03b/README.md)
  CombineArgs c;
  c.h = v_;
  c.h.abort = ctx_->abort;
  c.g = g0.g_out;
  c.x_in = x_in;
  c.x_out = x_out;
  c.x_out2 = x_out2;
  c.alpha_from_state = 0;
  c.alpha = alpha;
  if (update_impl(g0, 1, iter, dsign, gred, &c)) return true; // dir_cols_combine ran (coefficients from K)
  combine(g0.g_out, nullptr, x_in, x_out, x_out2, false, alpha);
  return false;
}

void History::combine(const float *g, float *dir, const float *x_in, float *x_out, float *x_out2,
                      bool alpha_from_state, double alpha, double *ww_part) {
  CombineArgs a;
  a.ww_part = ww_part;
  a.h = v_;
  a.h.abort = ctx_->abort;
  a.g = g;
  a.dir = dir;
  a.x_in = x_in;
  a.x_out = x_out;
  a.x_out2 = x_out2;
  a.alpha_from_state = alpha_from_state ? 1 : 0;
  a.alpha = alpha;
  ProfScope ps(ctx_, PK_COMBINE);
  hist_combine(ctx_->stream, a);
}

} // namespace lbf
