// The objectives and the full-batch L-BFGS driver (see solvers.hpp).
#include "solvers.hpp"

#include <algorithm>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <limits>

// Host-side acceptance tests must round like ls_ctl_kernel (and the reference's host code).
#pragma clang fp contract(off)

namespace lbf {

void CallbackObjective::eval(const float *x, float *g, const float *pdir, double *scal, const TailFuse *) {
  LBF_HIP(hipStreamSynchronize(c->stream)); // x is complete before the host callback reads it
  hl[0] = fn(user, x, g);
  ++count;
  const int nd = dots_partials_wg(nn);
  finalize_grad_dots(c->stream, nn, g, x, 0.0, pdir, part.get());
  eval_tail(c->stream, part.get(), nd, part.get(), 0, nullptr, 0.0, 0.0, scal);
  LBF_HIP(hipMemcpyAsync(scal + SC_LOSS, hl.get(), sizeof(double), hipMemcpyHostToDevice, c->stream));
}

LbfgsSolver::LbfgsSolver(Objective *obj, const lbf_lbfgs_params &prm, float *d_params, const Switches &sw)
    : early_(sw.early), host_timing_(sw.host_timing), obj_(obj), ctx_(obj->ctx()), prm_(prm), user_params_(d_params),
      n_(obj->n()), hist_(obj->ctx(), prm.m, obj->n(), sw.gram_fin), cnt_(obj) {
  LBF_REQUIRE(d_params, "null pointer");
  LBF_REQUIRE(prm.max_line_iters >= 1, "max_line_iters >= 1");
  for (int i = 0; i < 3; ++i) {
    xbuf_[i].resize(size_t(round4(n_)));
    gbuf_[i].resize(size_t(round4(n_ + 2)));
  }
  p_.resize(size_t(round4(n_)));
  x_ = xbuf_[0].get();
  xp_ = xbuf_[1].get();
  xt_ = xbuf_[2].get();
  g_ = gbuf_[0].get();
  gp_ = gbuf_[1].get();
  gt_ = gbuf_[2].get();
  // Speculation depth: iterations enqueued ahead of the host's line-search decision
  // (LBF_SPEC_DEPTH, default 3; 0 = host-driven). Host callbacks synchronise anyway.
  depth_ = obj_->async() ? std::max(0, std::min(16, sw.spec_depth)) : 0;
  // Fused optimizer tail on the speculative path (LBF_FUSED_TAIL=0 disables). It is a latency design
  // (one block per 64 coordinates, a partial row each): past kFusedTailMaxN the classic Gram sweep +
  // folded history step moves fewer bytes.
  fuse_ = sw.fused_tail && depth_ > 0 && obj_->fused_tail() && prm_.m > 0 && prm_.m <= TAIL_MAXM &&
          n_ <= kFusedTailMaxN;
  if (depth_ > 0) {
    abort_.resize(1);
    LBF_HIP(hipMemsetAsync(abort_.get(), 0, sizeof(int), ctx_->stream));
    LBF_HIP(hipHostMalloc(reinterpret_cast<void **>(&spec_rec_), kSpecRing * sizeof(SpecRecord),
                          hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(spec_rec_, 0xff, kSpecRing * sizeof(SpecRecord));
  }
  LBF_HIP(hipMemcpyAsync(x_, d_params, size_t(n_) * sizeof(float), hipMemcpyDeviceToDevice, ctx_->stream));
  l2_on_ = obj_->l2() != 0.0;
  if (l2_on_)
    for (int i = 0; i < 3; ++i) wwbuf_[i].resize(size_t(ww_partials_n(n_)));
  // initial evaluation (lbfgs.hpp:44 / lbfgs.cuh:147); under weight decay the start point has no w.w partials
  // (no combine wrote it) and no loss-only or early twin: its w.w is the evaluation's own sweep
  eval(x_, g_, nullptr);
  read_status();
  loss_ = hs_[SC_LOSS];
  lossf_ = float(loss_);
  gg_ = hs_[SC_TGG];
  t0_ = std::chrono::steady_clock::now();
}

LbfgsSolver::~LbfgsSolver() {
  if (spec_rec_) (void)hipHostFree(spec_rec_);
}

int LbfgsSolver::xslot(const float *x) const {
  for (int i = 0; i < 3; ++i)
    if (x == xbuf_[i].get()) return i;
  throw Error(2, "L-BFGS: not one of the solver's point buffers");
}

double *LbfgsSolver::ww_out(const float *x) {
  if (!l2_on_) return nullptr;
  const int i = xslot(x);
  ww_valid_[i] = true;
  return wwbuf_[i].get();
}

void LbfgsSolver::announce_ww(const float *x) {
  if (!l2_on_) return;
  const int i = xslot(x);
  obj_->point_ww(ww_valid_[i] ? wwbuf_[i].get() : nullptr);
}

void LbfgsSolver::eval(const float *x, float *g, const float *pdir, const TailFuse *tf) {
  LBF_REQUIRE(!tf || fuse_, "L-BFGS: a fused tail for an objective that has none"); // fuse_ implies fused_tail()
  announce_ww(x);
  obj_->eval(x, g, pdir, hist_.scal(), tf);
}

void LbfgsSolver::eval_loss(const float *x) {
  announce_ww(x);
  obj_->eval_loss(x, hist_.scal());
}

void LbfgsSolver::eval_grad_after_loss(const float *x, float *g, const float *pdir, const TailFuse *tf) {
  LBF_REQUIRE(!tf || fuse_, "L-BFGS: a fused tail for an objective that has none");
  announce_ww(x);
  obj_->eval_grad_after_loss(x, g, pdir, hist_.scal(), tf);
}

void LbfgsSolver::writeback() {
  LBF_HIP(hipMemcpyAsync(user_params_, x_, size_t(n_) * sizeof(float), hipMemcpyDeviceToDevice, ctx_->stream));
  LBF_HIP(hipStreamSynchronize(ctx_->stream));
}

bool LbfgsSolver::entry_converged() const {
  if (prm_.line_search == LBF_LS_ARMIJO) return float(std::sqrt(gg_)) < float(prm_.tol); // lbfgs.cuh:143
  return std::sqrt(gg_) < prm_.tol;                                                     // lbfgs.hpp:42
}

int LbfgsSolver::iterate(int iters, lbf_record *rec) {
  ctx_->set_device();
  rw_ = RecordWriter(rec);
  int done;
  if (depth_ > 0)
    done = iterate_spec(iters);
  else
    done = prm_.line_search == LBF_LS_ARMIJO ? iterate_armijo(iters) : iterate_wolfe(iters);
  writeback();
  return done;
}

// x <- trial, xp <- old x, xt <- free (same rotation for g)
void LbfgsSolver::accept_roles() {
  std::swap(xp_, x_);
  std::swap(x_, xt_);
  std::swap(gp_, g_);
  std::swap(g_, gt_);
  pending_pair_ = prm_.m > 0;
  ++iter_;
}

void LbfgsSolver::restore(const Roles &r) {
  x_ = r.x;
  xp_ = r.xp;
  xt_ = r.xt;
  g_ = r.g;
  gp_ = r.gp;
  gt_ = r.gt;
  iter_ = r.iter;
  pending_pair_ = r.pair;
  pending_reset_ = r.reset;
}

LsCtlArgs LbfgsSolver::ls_args(int seq, bool first, bool host_fold) const {
  LsCtlArgs a;
  a.scal = hist_.scal();
  a.abort = abort_.get();
  a.seq = seq;
  a.rec = spec_rec_ + seq % kSpecRing;
  a.armijo = prm_.line_search == LBF_LS_ARMIJO ? 1 : 0;
  a.first = first ? 1 : 0;
  a.host_fold = host_fold ? 1 : 0;
  a.fold = loss_;
  a.foldf = lossf_;
  a.c1 = prm_.c1;
  a.c2 = prm_.c2;
  a.tol = prm_.tol;
  return a;
}

TailFuse LbfgsSolver::tail_request(const LsCtlArgs &ls, float alphaf, bool early) const {
  TailFuse tf;
  tf.h = hist_.view();
  tf.has_pair = prm_.m > 0;
  tf.x_prev = x_;
  tf.g_prev = g_;
  tf.policy = ls.armijo ? POL_CUDA : POL_CPU;
  tf.iter_next = iter_ + 1;
  tf.ls = ls;
  tf.ls.alphaf = alphaf;
  tf.early = early ? 1 : 0;
  return tf;
}

float LbfgsSolver::begin_iteration(const LsCtlArgs *ls) {
  const bool armijo = prm_.line_search == LBF_LS_ARMIJO;
  float alpha = 1.0f;
  if (ls && dir_ready_) { // the previous fused tail computed this direction's coefficients
    hist_.combine(g_, p_.get(), x_, xt_, nullptr, !armijo, armijo ? double(alpha) : 0.0, ww_out(xt_));
  } else {
    GramArgs ga;
    ga.policy = armijo ? POL_CUDA : POL_CPU;
    ga.has_g = 1;
    ga.ga = g_;
    ga.reset = (armijo && pending_reset_) ? 1 : 0;
    if (pending_pair_) {
      ga.has_pair = 1;
      ga.sa = x_;
      ga.sb = xp_;
      ga.ya = g_;
      ga.yb = gp_;
    }
    hist_.update(ga, 1, iter_, -1.0);
    if (armijo) {
      if (iter_ == 0) alpha = std::min(1.0f, 1.0f / float(std::sqrt(gg_))); // lbfgs.cuh:149
      hist_.combine(g_, p_.get(), x_, xt_, nullptr, false, double(alpha), ww_out(xt_));
    } else {
      hist_.combine(g_, p_.get(), x_, xt_, nullptr, true, 0.0, ww_out(xt_)); // xt = x + alpha0 p
    }
  }
  if (ls) {
    // the early test: not on Wolfe iteration 0, which takes its trial without a test
    const TailFuse tf = tail_request(*ls, alpha, early_ && !ls->first);
    eval(xt_, gt_, p_.get(), &tf);
  } else {
    eval(xt_, gt_, p_.get());
  }
  return alpha;
}

// CPU semantics: LBFGS::solve (lbfgs.hpp:38-100) + FullBatchMinimizer::line_search
// (full_batch_minimizer.hpp:126-157). Every f / Gradient call of the reference maps to a cached
// fused evaluation: line_search's f(x), Gradient(x) are the previous accepted trial, the trial's
// Gradient(x+ap) comes with its f, the post-search Gradient(x_new) and the recorder's f(x) are the
// accepted trial's. Only an exhausted search (returns an alpha it never evaluated) costs one more.
// The host-finished search's gradient phase on the speculative route (finish_wolfe / finish_armijo): the backward
// of the loss-only trial just taken, then the fused tail with the host's decision rule at this alpha
// (tail.hip): on acceptance it pushes the pair
// and computes the next direction's coefficients, as a speculative iteration's tail does, so the next
// iteration speculates at once on the fused route. Returns the record's status; anything but SPEC_ACCEPT has
// raised the abort flag, which is cleared here (stream-ordered), and leaves the history untouched.
int LbfgsSolver::grad_fused(double alpha, SpecRecord *r) {
  LsCtlArgs a = ls_args(seq_++, false, true);
  a.alpha = alpha;
  const TailFuse tf = tail_request(a, float(alpha), false); // Armijo: the fp32 trial step itself
  eval_grad_after_loss(xt_, gt_, p_.get(), &tf);
  wait_record(a.seq, r);
  if (r->seq != a.seq) throw Error(2, "speculative line search: record out of sequence");
  if (r->status != SPEC_ACCEPT) LBF_HIP(hipMemsetAsync(abort_.get(), 0, sizeof(int), ctx_->stream));
  return r->status;
}

void LbfgsSolver::finish_wolfe(bool spec) {
  const double inf = std::numeric_limits<double>::infinity();
  double alpha = hs_[SC_ALPHA0];
  int trials = 0;
  bool fused_done = false; // the accepted trial's tail pushed the pair and built the next direction
  SpecRecord fr{};
  if (iter_ > 0) {
    const double f_old = loss_, gfo = hs_[SC_GTP];
    double amin = 0.0, amax = inf;
    alpha = 1.0;
    bool evaluated = true, have_grad = true;
    const bool split = obj_->split_eval();
    for (int i = 0; i < prm_.max_line_iters; ++i) {
      if (!evaluated) {
        {
          ProfScope ps(ctx_, PK_AXPY);
          axpy_to(ctx_->stream, n_, x_, float(alpha), p_.get(), xt_, ww_out(xt_));
        }
        if (split) { // f(x + alpha p) first; the gradient only once Armijo holds (:136-146)
          eval_loss(xt_);
          have_grad = false;
        } else {
          eval(xt_, gt_, p_.get());
        }
        read_status();
        evaluated = true;
      }
      ++trials;
      const double fn = hs_[SC_LOSS];
      if (fn > f_old + prm_.c1 * alpha * gfo) {
        amax = alpha;
        alpha = prm_.rho * (amin + amax);
        evaluated = false;
        continue;
      }
      if (!have_grad) { // backward phase of the forward pass just taken: bitwise the full evaluation
        have_grad = true;
        if (spec && fuse_) {
          if (grad_fused(alpha, &fr) == SPEC_ACCEPT) { // the host's tests below would pass alike
            fused_done = true;
            break;
          }
          read_status(); // rejected on curvature (or converged): the host's search goes on from the status
        } else {
          eval_grad_after_loss(xt_, gt_, p_.get());
          read_status();
        }
      }
      const double gnp = hs_[SC_TGP];
      if (gnp < prm_.c2 * gfo) {
        amin = alpha;
        alpha = (amax == inf) ? alpha * 2 : prm_.rho * (amin + amax);
        evaluated = false;
        continue;
      }
      break;
    }
    if (!evaluated) { // exhausted: the returned alpha was never evaluated (lbfgs.hpp:67-70)
      axpy_to(ctx_->stream, n_, x_, float(alpha), p_.get(), xt_, ww_out(xt_));
      eval(xt_, gt_, p_.get());
      read_status();
    } else if (!have_grad) { // exhausted on an Armijo failure: x_new's gradient is still needed
      eval_grad_after_loss(xt_, gt_, p_.get());
      read_status();
    }
  }
  accept_roles();
  loss_ = fused_done ? fr.loss : hs_[SC_LOSS];
  gg_ = fused_done ? fr.tgg : hs_[SC_TGG];
  dir_ready_ = fused_done;
  record(loss_, std::sqrt(gg_), alpha, trials);
}

int LbfgsSolver::iterate_wolfe(int iters) {
  int k = 0;
  for (; k < iters; ++k) {
    if (entry_converged()) {
      converged_ = true;
      break;
    }
    const bool had_pair = pending_pair_;
    begin_iteration();
    read_status();
    if (had_pair) rw_.patch_prev_accepted(int(hs_[SC_ACCEPT]));
    finish_wolfe();
  }
  return k;
}

// CUDA semantics: CudaLBFGS::solve (lbfgs.cuh:39-194), host scalars in fp32 like the reference.
void LbfgsSolver::finish_armijo(float alpha, bool spec) {
  const float c1 = float(prm_.c1), rho = float(prm_.rho);
  const float gdp = float(hs_[SC_GTP]);
  bool ok = false;
  int trials = 0;
  float lnew = 0.f, a_eval = alpha;
  const bool split = obj_->split_eval();
  bool have_grad = true;
  for (int ls = 0; ls < prm_.max_line_iters; ++ls) {
    if (ls > 0) { // loss only; the accepted (or last) trial's gradient afterwards (lbfgs.cuh:115-140)
      axpy_to(ctx_->stream, n_, x_, alpha, p_.get(), xt_, ww_out(xt_));
      if (split) {
        eval_loss(xt_);
        have_grad = false;
      } else {
        eval(xt_, gt_, p_.get());
      }
      read_status();
    }
    ++trials;
    a_eval = alpha;
    lnew = float(hs_[SC_LOSS]);
    if (lnew <= lossf_ + c1 * alpha * gdp) {
      ok = true;
      break;
    }
    const float den = 2.0f * (lnew - lossf_ - gdp * alpha);
    bool fb = true;
    if (std::fabs(den) > 1e-20f) {
      const float na = -(gdp * alpha * alpha) / den;
      if (na >= 0.1f * alpha && na <= 0.9f * alpha) {
        alpha = na;
        fb = false;
      }
    }
    if (fb) alpha *= rho;
  }
  bool fused_done = false; // the accepted trial's tail pushed the pair and built the next direction
  SpecRecord fr{};
  if (!have_grad) {
    if (spec && fuse_ && ok && grad_fused(double(a_eval), &fr) == SPEC_ACCEPT) {
      fused_done = true;
    } else {
      if (!(spec && fuse_ && ok)) eval_grad_after_loss(xt_, gt_, p_.get());
      read_status(); // (after a fused tail that did not accept: its status block)
    }
  }
  accept_roles();
  pending_reset_ = !ok; // lbfgs.cuh:147
  lossf_ = lnew;
  loss_ = fused_done ? fr.loss : hs_[SC_LOSS];
  gg_ = fused_done ? fr.tgg : hs_[SC_TGG];
  dir_ready_ = fused_done;
  record(double(lnew), double(float(std::sqrt(gg_))), double(a_eval), trials);
}

int LbfgsSolver::iterate_armijo(int iters) {
  int k = 0;
  for (; k < iters; ++k) {
    if (entry_converged()) {
      converged_ = true;
      break;
    }
    const bool had_pair = pending_pair_;
    const float alpha = begin_iteration();
    read_status();
    if (had_pair) rw_.patch_prev_accepted(int(hs_[SC_ACCEPT]));
    finish_armijo(alpha);
  }
  return k;
}

// Spins on the host-mapped record of speculative iteration `seq` (no event: an event record costs
// ~5 us of idle GPU per iteration). Only after 5 ms of spinning is the stream queried, so a failed
// launch or an already-drained queue surfaces instead of spinning forever: hipStreamQuery enqueues a
// marker packet behind the last launch, and a query per iteration put a ~6 us idle gap (the marker's
// release) in front of the first kernel of the iterations enqueued after it (profiles/r03/README.md).
void LbfgsSolver::wait_record(int seq, SpecRecord *out) {
  volatile SpecRecord *r = spec_rec_ + seq % kSpecRing;
  auto t0 = std::chrono::steady_clock::now();
  for (long long spin = 0;; ++spin) {
    if (__atomic_load_n(&spec_rec_[seq % kSpecRing].seq, __ATOMIC_ACQUIRE) == seq) break;
    if ((spin & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) {
      const hipError_t q = hipStreamQuery(ctx_->stream);
      if (q == hipSuccess) { // queue drained: the record must be there now
        if (__atomic_load_n(&spec_rec_[seq % kSpecRing].seq, __ATOMIC_ACQUIRE) == seq) break;
        throw Error(2, "speculative line search: record missing after the stream drained");
      }
      if (q != hipErrorNotReady) LBF_HIP(q);
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120))
        throw Error(2, "speculative line search: timed out waiting for the device");
    }
  }
  out->loss = r->loss;
  out->tgg = r->tgg;
  out->alpha0 = r->alpha0;
  out->accept_prev = r->accept_prev;
  out->status = r->status;
  out->seq = r->seq;
}

// Waits for everything queued, clears the abort flag and forgets the aborted iterations. status: the
// status block is copied to the host behind the aborted launches, in the same wait (read_status's copy).
void LbfgsSolver::drain(std::deque<Flight> &q, size_t prof_end, bool status) {
  if (status) hs_.enqueue(ctx_->stream, hist_.scal());
  LBF_HIP(hipStreamSynchronize(ctx_->stream));
  LBF_HIP(hipMemsetAsync(abort_.get(), 0, sizeof(int), ctx_->stream));
  obj_->discard_evals((long long)q.size());
  if (ctx_->prof.on && ctx_->prof.recs.size() > prof_end) ctx_->prof.recs.resize(prof_end);
  q.clear();
}

// Speculative pipeline. Almost every accepted step is the first trial (alpha = 1), so the host
// enqueues up to depth_ iterations assuming it will be, and a one-thread ls_ctl kernel after each first
// trial decides on the device with the host's own test. A rejected (or converged) trial raises the
// abort flag: every launch queued behind it exits at entry, the host waits, restores the buffer roles
// of that iteration (the history, Gram state and status block are exactly as that trial left them)
// and finishes it host-driven, then speculates again. Results are identical to the host-driven loop.
int LbfgsSolver::iterate_spec(int iters) {
  const bool armijo = prm_.line_search == LBF_LS_ARMIJO;
  std::deque<Flight> q;
  int done = 0, issued = 0;
  bool host_fold = true;
  ctx_->abort = abort_.get();
  struct Clear {
    Ctx *c;
    ~Clear() { c->abort = nullptr; }
  } clear{ctx_};
  // LBF_HOST_TIMING=1: where the host thread spends an iteration (enqueue vs waiting for the device)
  double t_enq = 0.0, t_wait = 0.0;
  long long n_wait = 0, n_ready = 0;
  using clk = std::chrono::steady_clock;
  while (done < iters) {
    if (q.empty() && entry_converged()) {
      converged_ = true;
      break;
    }
    const auto te0 = clk::now();
    while (issued < iters && int(q.size()) < depth_) {
      Flight f;
      f.roles = roles();
      f.seq = seq_++;
      LsCtlArgs a = ls_args(f.seq, iter_ == 0, host_fold);
      if (fuse_) {
        f.alpha = begin_iteration(&a); // decision inside the fused tail
        dir_ready_ = true;
      } else {
        f.alpha = begin_iteration();
        a.alphaf = f.alpha;
        ls_ctl(ctx_->stream, a);
      }
      f.prof_end = ctx_->prof.recs.size();
      q.push_back(f);
      host_fold = false;
      accept_roles(); // assume the first trial is taken
      pending_reset_ = false;
      ++issued;
    }
    const Flight f = q.front();
    q.pop_front();
    SpecRecord r;
    const auto tw0 = clk::now();
    if (host_timing_) {
      t_enq += std::chrono::duration<double>(tw0 - te0).count();
      n_ready += __atomic_load_n(&spec_rec_[f.seq % kSpecRing].seq, __ATOMIC_ACQUIRE) == f.seq ? 1 : 0;
    }
    wait_record(f.seq, &r);
    if (host_timing_) {
      t_wait += std::chrono::duration<double>(clk::now() - tw0).count();
      ++n_wait;
    }
    if (r.seq != f.seq) throw Error(2, "speculative line search: record out of sequence");
    if (f.roles.pair) rw_.patch_prev_accepted(int(r.accept_prev));
    if (r.status == SPEC_REJECT || r.status == SPEC_REJECT_EARLY) {
      if (r.status == SPEC_REJECT_EARLY) obj_->backward_skipped();
      drain(q, f.prof_end, true); // + the status block as the rejected trial left it (one wait)
      dir_ready_ = false;         // the host finishes this iteration; the next one builds its direction
      restore(f.roles);
      if (armijo)
        finish_armijo(f.alpha, true);
      else
        finish_wolfe(true);
      ++done;
      issued = done;
      host_fold = true;
      continue;
    }
    loss_ = r.loss;
    gg_ = r.tgg;
    if (armijo) {
      lossf_ = float(r.loss);
      record(double(lossf_), double(float(std::sqrt(gg_))), double(f.alpha), 1);
    } else {
      record(loss_, std::sqrt(gg_), f.roles.iter == 0 ? r.alpha0 : 1.0, f.roles.iter == 0 ? 0 : 1);
    }
    ++done;
    if (r.status == SPEC_CONVERGED) {
      // the iterations queued behind were aborted: return to the roles right after this step
      if (!q.empty()) restore(q.front().roles);
      drain(q, f.prof_end);
      dir_ready_ = false; // the fused tail does not push the pair of a converged step
      issued = done;
      host_fold = true;
    }
  }
  if (host_timing_ && n_wait)
    std::fprintf(stderr, "[lbf host] spec: %lld records, enqueue %.2f us/iter, wait %.2f us/iter, %lld already there\n",
                 n_wait, 1e6 * t_enq / double(n_wait), 1e6 * t_wait / double(n_wait), n_ready);
  return done;
}

void LbfgsSolver::info(lbf_solve_info *out) const {
  cnt_.fill(out, iter_, loss_, std::sqrt(gg_));
}

} // namespace lbf
