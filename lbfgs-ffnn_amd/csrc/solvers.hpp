// Solver drivers (solve_*.cpp): full-batch L-BFGS (CPU/Wolfe and CUDA/Armijo semantics), S-LBFGS, GD, SGD,
// Hessian-free, OWL-QN and Adam.
#pragma once

#include "../../include/lbfgs_amd.h"
#include "host_sync.hpp"
#include "runtime.hpp"
#include "sampler.hpp"
#include "solver_io.hpp"

#include <atomic>
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <mutex>
#include <random>
#include <thread>

namespace lbf {

// What the minimizer evaluates: the reference's LossGradFun (src/cuda/minimizer_base.cuh:15-16) plus the
// dots the line search needs. eval() writes the gradient into g (n+2 floats) and SC_LOSS / SC_TGG /
// SC_TGP (g.pdir) into the device status block scal, all on ctx()->stream. tf: null, or the fused optimizer tail
// (tail.hip) to run behind the evaluation; only a fused_tail() objective is ever handed one (the solver checks).
struct Objective {
  virtual ~Objective() = default;
  virtual Ctx *ctx() const = 0;
  virtual long long n() const = 0;
  virtual void eval(const float *x, float *g, const float *pdir, double *scal, const TailFuse *tf) = 0;
  virtual long long evals() const = 0;
  virtual long long rows() const { return 0; } // batch rows evaluated (0: not an MLP objective)
  // L2 weight decay inside the objective (loss + 0.5 l2 |x|^2, g + l2 x). When non-zero, the solver announces
  // before each evaluation the w.w partials (kernels.hpp WwPart, ww_partials_n(n) words) that the kernel which
  // wrote the point left, or nullptr for a point no such kernel wrote (the start point).
  virtual double l2() const { return 0.0; }
  virtual void point_ww(const double *) {}
  // Asynchronous objectives can be enqueued ahead of the host's line-search decisions.
  virtual bool async() const { return false; }
  virtual void discard_evals(long long) {}
  virtual void backward_skipped() {} // the last trial's backward was skipped (SPEC_REJECT_EARLY)
  // Two-step evaluation of a line-search trial (split_eval()): the loss alone (SC_LOSS, SC_SSE), then the
  // gradient and dots of that same point; together bitwise equal to eval().
  virtual bool split_eval() const { return false; }
  virtual void eval_loss(const float *, double *) {}
  virtual void eval_grad_after_loss(const float *, float *, const float *, double *, const TailFuse *) {}
  virtual long long loss_only_evals() const { return 0; }
  virtual long long grad_after_loss_evals() const { return 0; }
  virtual bool fused_tail() const { return false; } // eval / eval_grad_after_loss can run the fused tail
};

// The MLP's fused loss+grad over the rank's shard (mean over n_global samples).
struct MlpObjective : Objective {
  Mlp *net;
  const float *X, *Y;
  long long nloc, nglob;
  double lambda; // the network's l2, read once when the solve begins
  WwPart ww;     // the next evaluated point's w.w partials (point_ww)
  MlpObjective(Mlp *m, const float *x, const float *y, long long nl, long long ng)
      : net(m), X(x), Y(y), nloc(nl), nglob(ng), lambda(m->l2()) {}
  double l2() const override { return lambda; }
  void point_ww(const double *part) override {
    ww.part = lambda != 0.0 ? part : nullptr;
    ww.n = ww.part ? ww_partials_n((long long)net->nparams()) : 0;
  }
  Ctx *ctx() const override { return net->ctx(); }
  long long n() const override { return (long long)net->nparams(); }
  void eval(const float *x, float *g, const float *pdir, double *scal, const TailFuse *tf) override {
    net->loss_grad(x, g, X, Y, nullptr, nloc, 1.0 / double(nglob), lambda, pdir, scal, tf, ww);
  }
  long long evals() const override { return net->evals(); }
  long long rows() const override { return net->rows(); }
  bool async() const override { return true; }
  void discard_evals(long long k) override { net->discard_evals(k, nloc); }
  void backward_skipped() override { net->backward_skipped(); }
  bool split_eval() const override { return true; }
  void eval_loss(const float *x, double *scal) override {
    net->loss_only(x, X, Y, nullptr, nloc, 1.0 / double(nglob), scal, lambda, ww);
  }
  void eval_grad_after_loss(const float *x, float *g, const float *pdir, double *scal,
                            const TailFuse *tf) override {
    net->grad_after_loss(x, g, X, nullptr, nloc, 1.0 / double(nglob), lambda, pdir, scal, tf, ww);
  }
  long long loss_only_evals() const override { return net->loss_only_evals(); }
  long long grad_after_loss_evals() const override { return net->grad_after_loss_evals(); }
  bool fused_tail() const override { return true; }
};

// A user callback with the reference's LossGradFun contract: returns the loss, writes the gradient
// (device) for the device parameters it is given. Host-driven, so the stream is synchronised first.
struct CallbackObjective : Objective {
  Ctx *c;
  long long nn;
  double (*fn)(void *, const float *, float *);
  void *user;
  DevBuf<double> part;
  PinnedBuf<double> hl;
  long long count = 0;
  CallbackObjective(Ctx *cx, long long n_, double (*f)(void *, const float *, float *), void *u)
      : c(cx), nn(n_), fn(f), user(u) {
    part.resize(size_t(dots_partials_wg(n_)) * 3);
    hl.ensure(1);
  }
  Ctx *ctx() const override { return c; }
  long long n() const override { return nn; }
  void eval(const float *x, float *g, const float *pdir, double *scal, const TailFuse *) override;
  long long evals() const override { return count; }
};

// Full-batch L-BFGS on the MLP. All vectors, the (s, y) ring and its Gram state stay on the device;
// the host only reads a 16-double status block once per line-search trial.
class LbfgsSolver {
public:
  // sw: speculation depth, fused tail, early Armijo test, host timing; the history's route
  LbfgsSolver(Objective *obj, const lbf_lbfgs_params &prm, float *d_params, const Switches &sw);
  ~LbfgsSolver();
  // Runs up to `iters` iterations. Returns the number run (fewer on convergence).
  int iterate(int iters, lbf_record *rec);
  void info(lbf_solve_info *out) const;
  bool converged() const { return converged_; }

private:
  // The objective's three evaluations of a point buffer x, its w.w partials announced first; status -> scal().
  // tf: the fused tail behind the evaluation (fuse_ only)
  void eval(const float *x, float *g, const float *pdir, const TailFuse *tf = nullptr);
  void eval_loss(const float *x);
  void eval_grad_after_loss(const float *x, float *g, const float *pdir, const TailFuse *tf = nullptr);
  void read_status() { hs_.read(ctx_->stream, hist_.scal()); }
  void writeback();
  int iterate_wolfe(int iters);
  int iterate_armijo(int iters);
  int iterate_spec(int iters);
  bool entry_converged() const;
  // First trial of an iteration (history update, direction, x + alpha p, evaluation), enqueued only.
  // Returns the Armijo trial step (Wolfe takes alpha0 from the device status block). With `ls`, the
  // evaluation carries the fused tail: decision + (on acceptance) the next direction's coefficients.
  float begin_iteration(const LsCtlArgs *ls = nullptr);
  // Rest of the iteration once hs_ holds the first trial's status: further trials, role rotation,
  // record.
  void finish_wolfe(bool spec = false);
  int grad_fused(double alpha, SpecRecord *r); // finish_wolfe's gradient phase through the fused tail
  void finish_armijo(float alpha, bool spec = false);
  void accept_roles();
  // The line-search decision's arguments for sequence number seq, and the fused tail request around them
  // (alphaf: the fp32 trial step; early: the Armijo test in the trial's first backward launch).
  LsCtlArgs ls_args(int seq, bool first, bool host_fold) const;
  TailFuse tail_request(const LsCtlArgs &ls, float alphaf, bool early) const;
  void record(double loss, double gnorm, double alpha, int trials) {
    rw_.put(loss, gnorm, ms_since(t0_), alpha, trials, -1); // accepted: patched by the next iteration
  }

  // speculative pipeline state
  struct Roles {
    float *x, *xp, *xt, *g, *gp, *gt;
    int iter;
    bool pair, reset;
  };
  Roles roles() const { return {x_, xp_, xt_, g_, gp_, gt_, iter_, pending_pair_, pending_reset_}; }
  void restore(const Roles &r);
  struct Flight {
    Roles roles;
    float alpha;
    int seq;
    size_t prof_end;
  };
  void drain(std::deque<Flight> &q, size_t prof_end, bool status = false);
  void wait_record(int seq, SpecRecord *out);
  static constexpr int kSpecRing = 32;
  static constexpr long long kFusedTailMaxN = 1LL << 21;
  int depth_ = 0;
  int seq_ = 0;
  bool fuse_ = false;      // fused optimizer tail on the speculative path
  const bool early_;       // a speculative first trial's Armijo test in its first backward launch (Switches::early)
  const int host_timing_;  // Switches::host_timing
  bool dir_ready_ = false; // the last fused tail left the next direction's coefficients on the device
  DevBuf<int> abort_;
  SpecRecord *spec_rec_ = nullptr;

  Objective *obj_;
  Ctx *ctx_;
  lbf_lbfgs_params prm_;
  float *user_params_;
  long long n_;
  History hist_;
  DevBuf<float> xbuf_[3], gbuf_[3], p_;
  // Weight decay (obj_->l2() != 0): the w.w partials of the point in each x buffer, written by the kernel that
  // wrote the point (the combine or axpy_to of a trial). They travel with the buffer through the role rotation.
  DevBuf<double> wwbuf_[3];
  bool ww_valid_[3] = {false, false, false};
  bool l2_on_ = false;
  int xslot(const float *x) const;
  double *ww_out(const float *x);           // where the producer of x writes (nullptr: no weight decay)
  void announce_ww(const float *x);         // obj_->point_ww for the evaluation of x that follows
  float *x_, *xp_, *xt_, *g_, *gp_, *gt_;
  StatusMirror hs_;
  double loss_ = 0, gg_ = 0;
  float lossf_ = 0;
  int iter_ = 0;
  bool pending_pair_ = false, pending_reset_ = false, converged_ = false;
  RecordWriter rw_; // begun from rec->size by every iterate()
  SolveCounters<Objective> cnt_;
  std::chrono::steady_clock::time_point t0_;
};

class SlbfgsSolver {
public:
  // sw: full-ahead, host timing; the history's route and the switches of the twin workspaces' Mlps
  SlbfgsSolver(Mlp *net, const lbf_slbfgs_params &prm, float *d_params, const float *X, const float *Y,
               long long N, const Switches &sw);
  ~SlbfgsSolver();
  int run(lbf_record *rec);                 // prm.max_epochs epochs (lbf_slbfgs_solve)
  int iterate(int epochs, lbf_record *rec); // up to `epochs` more (lbf_slbfgs_begin / iterate / end)
  void info(lbf_solve_info *out) const;
  // copies the first traced curvature-pair candidate's iterate w_t, average u, s and y (n floats each);
  // false when no candidate was traced yet
  bool pair0(float *wt, float *u, float *s, float *y) const;
  // Diagnostics (lbf_slbfgs_pair_io): at curvature event e (each inner step t > 0 with t % L == 0, the first,
  // which offers no pair, included) record [w_{t+1} | u | g(u + eps s) | g(u - eps s)] into rec + 4 e ld, and
  // force u, g(u + eps s), g(u - eps s) to force + 4 e ld's before use (ld = round4(n); NULL: off)
  void pair_io(int cap, float *rec, const float *force) {
    pio_cap_ = cap;
    pio_rec_ = rec;
    pio_force_ = force;
  }

private:
  const int host_timing_; // Switches::host_timing
  int pio_cap_ = 0, nev_ = 0;
  float *pio_rec_ = nullptr;
  const float *pio_force_ = nullptr;
  struct Slice {
    long long off = 0, cnt = 0, total = 0; // offset / count in this rank's flat list, whole batch size
  };
  // An epoch's index lists: every minibatch, the Hessian batches (only once a u exists), then the anchor
  // pick, in the reference's RNG order (s_lbfgs.hpp:212-266); `flat` holds this rank's slices.
  struct EpochDraw {
    std::vector<int> flat, hflat, batch;
    std::vector<Slice> mb, hb;
    int pick = -1;
    bool u_seen = false; // have_u after the epoch
  };
  void draw_epoch(bool u_seen, EpochDraw &d);
  // The epoch's inner steps (s_lbfgs.hpp:218-262) enqueued on the streams.
  void epoch_steps(const EpochDraw &d);
  int wh_slot(int logical) const { return (wh_head_ + logical) % (prm_.L + 1); }
  int wh_push_slot();
  std::mt19937 rng_;
  std::unique_ptr<MinibatchSampler> sampler_;
  bool started_ = false, have_u_ = false, mu_valid_ = false, next_ready_ = false, converged_ = false;
  EpochDraw cur_, next_;
  int wh_head_ = 0, wh_count_ = 0; // ring of L+1 iterates (w_history)
  RecordWriter rw_;                // begun from rec->size by the first iterate() only
  // Data parallel (a communicator), LBF_SLBFGS_DP_REPLICATED: every rank runs the epoch's whole inner-step
  // chain (identical inputs, identical bits) with no collective; only the full-batch gradient at the
  // anchor (s_lbfgs.hpp:206, 274-284) is sharded, one all-reduce per epoch. LBF_SLBFGS_DP_SLICED: each rank
  // evaluates its 1/p slice of every minibatch and Hessian batch, one all-reduce per inner step.
  bool repl_ = false;
  bool dp_inner() const { return ctx_->dp() && !repl_; }
  // Replicated mode's guard: every epoch, fingerprints of each rank's new anchor w are all-reduced before
  // the sharded full-batch evaluation, and a mismatch (ranks whose inner chains drifted apart, which would
  // make that all-reduce sum gradients taken at different points) fails the solve.
  DevBuf<float> fp_;
  PinnedBuf<float> hfp_;
  void replica_fingerprints();
  void replica_check() const;
  std::chrono::steady_clock::time_point t0_;
  // Two independent batch gradients of one step (the FD pair at u +- eps s) into one [ga | gb] block
  // (gb = gab + ng_): the second on the twin's stream when there is one, joined before the next launch.
  // Data parallel: both evaluations stop before the all-reduce and ONE collective sums the block.
  void eval_pair(const float *wa, const float *wb, float *gab, long long off, long long count,
                 double inv_scale); // rows off .. off+count-1 of this rank's gathered block
  // Data parallel: all-reduce a [ga | gb] block once, then finish both gradients (+ lambda w).
  void reduce_pair(const float *wa, const float *wb, float *gab, double inv_scale);
  void trace_pair(int epoch, int t);
  int npairs_ = 0;
  // diagnostics (pair_trace on): the first traced candidate's w_t, u, s, y (lbf_slbfgs_pair0)
  DevBuf<float> p0_;
  bool p0_set_ = false;
  Mlp *net_;
  Ctx *ctx_;
  lbf_slbfgs_params prm_;
  float *user_params_;
  const float *X_, *Y_;
  long long N_, n_;
  History hist_;
  DevBuf<float> w_, wt_, mu_, v_, r_, u_, up_, s_, wp_, wm_, wh_;
  // [g(w_t) | g(w)] of an inner step, double-buffered (the twin fills the anchor half one step ahead),
  // and [g(u + eps s) | g(u - eps s)] of a Hessian step: one all-reduce per block under data parallelism
  DevBuf<float> gpair_[2], fdpair_;
  long long ng_ = 0; // floats per gradient in a block (n + 2 loss words, rounded to 4)
  DevBuf<int> idx_;
  PinnedBuf<int> idx_host_; // pinned staging of an epoch's index lists
  StatusMirror hs_;
  int iters_ = 0;
  double last_loss_ = 0, last_gnorm_ = 0;
  SolveCounters<Mlp> cnt_; // the side networks below count from zero
  // Twin evaluator: a second workspace of the same network on its own stream, so the two latency-bound
  // minibatch evaluations of a step run concurrently (results unchanged: each is the same launch
  // sequence on its own buffers). Data parallel: the twin's evaluations stop before the all-reduce
  // (it has no communicator) and the context stream's one collective per block sums both.
  std::unique_ptr<Ctx> tctx_;
  std::unique_ptr<Mlp> tnet_;
  // The twin stream's launches enqueued by a helper host thread: the inner step's host enqueue (≈ 100-130 µs, ~40 % of it the twin's evaluation) bounds the epoch on slower
  // hosts. Tasks run in posting order (one FIFO, so the twin stream sees the single-thread launch order);
  // the context thread waits for a task's ticket before it waits on an event that task records, and records
  // an event the twin waits on only after the waiting task has been enqueued (see epoch_steps).
  std::unique_ptr<TaskFifo> tw_; // host_sync.hpp
  long long twin_post(std::function<void()> f);
  void twin_wait(long long ticket); // returns once task `ticket` (1-based) has run; rethrows its error
  // this rank's slices of the epoch's sampled rows, gathered once (all minibatches and Hessian batches)
  DevBuf<float> xg_, yg_;
  hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr;
  // free-running twin (no per-step collective): anchor gradient of step t in ganc_ + t ng_, its event
  // ev_anc_[t]; off for good once its buffer does not fit in free device memory (double-buffered twin)
  bool free_twin_ = true;
  DevBuf<float> ganc_;
  std::vector<hipEvent_t> ev_anc_;
  hipEvent_t ev_g2_[2] = {nullptr, nullptr}, ev_free_[2] = {nullptr, nullptr}; // anchor gradients ahead (twin)
  // The epoch-end full-batch evaluation at the next anchor (s_lbfgs.hpp:265-284: the recorder's loss and
  // gradient, which are the next epoch's mu) started as soon as the picked iterate exists: the pick is drawn
  // with the epoch's index lists, before the epoch runs, and the picked entry of w_history stays in its ring
  // slot to the end. A third workspace of the network on its own stream evaluates it beside the epoch's last
  // inner steps into mu_next_ and its own status block; the context stream joins it where the ordered route
  // evaluated. Same launches on the same inputs: bitwise the ordered route. Single rank only (data parallel
  // keeps the ordered, sharded evaluation and its fingerprint check). Opt-in (LBF_FULL_AHEAD=1): measured
  // slower at cfg 4, 35.27-35.59 against 35.88-36.16 epochs/s interleaved (profiles/r05/n/): the full-batch
  // GEMMs occupy the chip for ~1.2 ms and the latency-bound inner steps beside them slow down by more than
  // the evaluation's ~0.6 ms average window (the pick lands mid-ring) saves.
  std::unique_ptr<Ctx> fctx_;
  std::unique_ptr<Mlp> fnet_;
  DevBuf<float> mu_next_;
  DevBuf<double> fscal_;
  hipEvent_t ev_anchor_ = nullptr, ev_full_ = nullptr;
  bool full_posted_ = false;
  // inner step after whose combine the picked iterate exists (-1: the epoch's start, -2: no pick)
  int full_ahead_step(const EpochDraw &d) const;
  void post_full(const float *anchor);
};

// CudaGD / CudaSGD (src/cuda/gd.cuh:38-106, sgd.cuh:50-153) on the MLP; return the iterations done.
int run_gd(Mlp *net, const lbf_gd_params &prm, float *d_params, const float *X, const float *Y, long long n_local,
           long long n_global, lbf_record *rec, lbf_solve_info *info);
int run_sgd(Mlp *net, const lbf_sgd_params &prm, float *d_params, const float *X, const float *Y, long long N,
            lbf_record *rec, lbf_solve_info *info);

// Adam / AdamW over shuffled minibatches (lbfgs_amd.h lbf_adam_solve states the algorithm). The host
// forms the step's nine coefficients (adam_coefs), draws the epoch's order and enqueues, per batch, the fused
// evaluation and one sweep (adam.hip) that also accumulates the epoch loss: one synchronisation per epoch.
// adam_check: LBF_ERR_INVALID for parameters outside the contract. adam_coefs: p1, p2 = beta1^t, beta2^t, the
// caller's running fp64 products.
void adam_check(const lbf_adam_params &prm);
AdamCoef adam_coefs(const lbf_adam_params &prm, double lr_now, double p1, double p2);
class AdamSolver {
public:
  AdamSolver(Mlp *net, const lbf_adam_params &prm, float *d_params, const float *X, const float *Y, long long N);
  int iterate(int epochs, lbf_record *rec); // up to `epochs` more; returns the epochs run
  void info(lbf_solve_info *out) const;
  int epochs() const { return epoch_; }

private:
  void full_record(bool start);
  Mlp *net_;
  Ctx *ctx_;
  lbf_adam_params prm_;
  float *w_;
  const float *X_, *Y_;
  long long N_, n_, nb_;
  double l2_;
  DevBuf<float> g_, m_, v_;
  DevBuf<double> scal_, acc_; // acc_: [epoch sum | one batch objective per step of the epoch]
  PinnedBuf<double> hacc_;
  DevBuf<int> idx_;
  PinnedBuf<int> hidx_;
  std::vector<int> order_;
  std::mt19937 rng_;
  StatusMirror hs_;
  RecordWriter rw_; // begun from rec->size by the first iterate() only
  SolveCounters<Mlp> cnt_;
  std::chrono::steady_clock::time_point t0_;
  long long t_ = 0;             // steps so far
  double p1_ = 1.0, p2_ = 1.0;  // beta1^t, beta2^t
  double lr_e_ = 0.0, prev_ = 0.0;
  int epoch_ = 0, rows_done_ = 0;
  bool started_ = false, have_prev_ = false, converged_ = false, recorded_ = false;
};

// Hessian-free solver (lbfgs_amd.h lbf_hf_solve): Gauss-Newton CG steps with Levenberg-Marquardt
// damping and a backtracking line search; returns the outer iterations done.
// pc (nullable; null or mode LBF_PRECOND_NONE: plain CG): the CG is preconditioned with
// M = (cinv D + l2 + lambda_k)^exponent, D = Mlp::grad_sq of the curvature rows (lbf_hf_solve_pc).
int run_hf(Mlp *net, const lbf_hf_params &prm, float *d_params, const float *X, const float *Y, long long n_local,
           long long n_global, lbf_record *rec, lbf_solve_info *info, const lbf_hf_precond *pc = nullptr);

// OWL-QN (lbfgs_amd.h lbf_owlqn_solve): L-BFGS on loss + 0.5 l2 |w|^2 + l1 |w|_1 with the pseudo-gradient,
// the sign-constrained direction and the orthant projection of Andrew & Gao 2007; returns the iterations done.
int run_owlqn(Mlp *net, const lbf_owlqn_params &prm, float *d_params, const float *X, const float *Y,
              long long n_local, long long n_global, lbf_record *rec, lbf_solve_info *info, lbf_owlqn_stats *stats);
// Which coordinates of the network's flat parameters carry the L1 penalty: all of them (l1_bias != 0), or all but
// each layer's biases. owl_penalised_count: how many that is.
OwlCoef owl_coef(const Mlp &net, double l1, int l1_bias);
long long owl_penalised_count(const Mlp &net, int l1_bias);

// finite_difference_hvp_batch (s_lbfgs.hpp:88-101) up to the last step: wp/wm = u +- eps s, gp/gm = the
// batch gradients there (1/count scale, + lambda w). y = (gp - gm) / (2 eps) is formed by the caller (the
// S-LBFGS pair sweep, or diff_scale) in fp32 with the factor rounded once.
void fd_hvp_grads(Mlp *net, const float *u, const float *s, const float *X, const float *Y, const int *idx,
                  long long count, double inv_scale, double lambda, double eps, float *wp, float *wm, float *gp,
                  float *gm, double *scal);

} // namespace lbf
