// S-LBFGS driver and the finite-difference Hessian-vector gradients (see solvers.hpp).
#include "solvers.hpp"

#include <algorithm>
#include <cstdio>
#include <cmath>
#include <cstring>

// Host-side acceptance tests must round like ls_ctl_kernel (and the reference's host code).
#pragma clang fp contract(off)

namespace lbf {

void fd_hvp_grads(Mlp *net, const float *u, const float *s, const float *X, const float *Y, const int *idx,
                  long long count, double inv_scale, double lambda, double eps, float *wp, float *wm, float *gp,
                  float *gm, double *scal) {
  hipStream_t st = net->ctx()->stream;
  const long long n = (long long)net->nparams();
  lincomb(st, n, u, eps, s, wp);
  lincomb(st, n, u, -eps, s, wm);
  net->loss_grad(wp, gp, X, Y, idx, count, inv_scale, lambda, nullptr, scal);
  net->loss_grad(wm, gm, X, Y, idx, count, inv_scale, lambda, nullptr, scal);
}

namespace {
// A side stream's context on the parent's device: its own non-blocking stream at the lowest priority (when the
// device has a priority range): what runs there is off the critical path, the context stream's chain is on it
// (the twin confined to 32-128 of the CUs measured the same, profiles/r04/e/).
std::unique_ptr<Ctx> side_ctx(const Ctx &parent) {
  std::unique_ptr<Ctx> c(new Ctx());
  c->device = parent.device;
  c->cus = parent.cus;
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest < least)
    LBF_HIP(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, least));
  else
    LBF_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  c->own_stream = true;
  return c;
}

// The benchmark's section timing covers the side streams' launches too (the settings may change per call).
void copy_prof_settings(const Ctx &parent, Ctx &side) {
  side.prof.on = parent.prof.on;
  side.prof.only = parent.prof.only;
  if (side.prof.every != parent.prof.every) side.prof.seen = 0;
  side.prof.every = parent.prof.every;
}

// A second workspace of the same network (shape and loss) on another context.
std::unique_ptr<Mlp> same_net(const Mlp &net, Ctx *ctx, const Switches &sw) {
  std::vector<int> dims, acts;
  for (const Layer &L : net.layers()) {
    dims.push_back(L.in);
    acts.push_back(L.act);
  }
  dims.push_back(net.layers().back().out);
  std::unique_ptr<Mlp> m(new Mlp(ctx, int(acts.size()), dims.data(), acts.data(), sw));
  m->set_loss(net.loss()); // the side networks evaluate the caller's objective
  return m;
}
} // namespace

SlbfgsSolver::SlbfgsSolver(Mlp *net, const lbf_slbfgs_params &prm, float *d_params, const float *X, const float *Y,
                           long long N, const Switches &sw)
    : host_timing_(sw.host_timing), net_(net), ctx_(net->ctx()), prm_(prm), user_params_(d_params), X_(X), Y_(Y),
      N_(N), n_((long long)net->nparams()), hist_(net->ctx(), prm.M, (long long)net->nparams(), sw.gram_fin),
      cnt_(net) {
  LBF_REQUIRE(d_params && X && Y && N > 0, "null pointer / empty data");
  LBF_REQUIRE(prm.b > 0 && prm.L > 0 && prm.L + 1 <= 64, "b > 0, 1 <= L <= 63");
  const size_t nv = size_t(round4(n_)), ng = size_t(round4(n_ + 2));
  w_.resize(nv);
  wt_.resize(nv);
  v_.resize(nv);
  r_.resize(nv);
  u_.resize(nv);
  up_.resize(nv);
  s_.resize(nv);
  wp_.resize(nv);
  wm_.resize(nv);
  mu_.resize(ng);
  ng_ = (long long)ng;
  // zeroed once: the pads between the two halves of a block are summed by the all-reduce too
  for (auto *b : {&gpair_[0], &gpair_[1], &fdpair_}) {
    b->resize(2 * ng);
    LBF_HIP(hipMemsetAsync(b->get(), 0, 2 * ng * sizeof(float), ctx_->stream));
  }
  wh_.resize(nv * size_t(prm.L + 1));
  rng_.seed(prm.seed);
  sampler_.reset(new MinibatchSampler(size_t(N)));
  repl_ = ctx_->dp() && prm.dp_mode == LBF_SLBFGS_DP_REPLICATED;
  LBF_REQUIRE(prm.dp_mode == LBF_SLBFGS_DP_REPLICATED || prm.dp_mode == LBF_SLBFGS_DP_SLICED, "dp_mode 0 / 1");
  // Twin evaluator (see tnet_). Epoch hipGraphs of both streams were built and measured slower on ROCm
  // 7.2: hipGraphLaunch spends about as much host time per node as an eager launch, and the replay runs
  // every node on one queue, so the twin's anchor gradients stopped overlapping the context stream's chain
  // (profiles/r03b/cfg4_graph*). Precomputing an epoch's anchor gradients in one evaluation measured no
  // faster than the twin (profiles/r03/bench_cfg4_{pre,twin}_*.json).
  {
    tctx_ = side_ctx(*ctx_);
    copy_prof_settings(*ctx_, *tctx_);
    tnet_ = same_net(*net, tctx_.get(), sw);
    LBF_HIP(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming | event_release_flags()));
    LBF_HIP(hipEventCreateWithFlags(&ev_join_, hipEventDisableTiming | event_release_flags()));
    for (int i = 0; i < 2; ++i) {
      LBF_HIP(hipEventCreateWithFlags(&ev_g2_[i], hipEventDisableTiming | event_release_flags()));
      LBF_HIP(hipEventCreateWithFlags(&ev_free_[i], hipEventDisableTiming | event_release_flags()));
    }
    const int dev = ctx_->device;
    tw_.reset(new TaskFifo([dev]() { LBF_HIP(hipSetDevice(dev)); }));
    // the epoch-end full-batch evaluation ahead (see fnet_): single rank, opt-in (LBF_FULL_AHEAD=1)
    if (!ctx_->dp() && sw.full_ahead) {
      fctx_ = side_ctx(*ctx_);
      copy_prof_settings(*ctx_, *fctx_);
      fnet_ = same_net(*net, fctx_.get(), sw);
      mu_next_.resize(ng);
      fscal_.resize(SC_N);
      LBF_HIP(hipMemsetAsync(fscal_.get(), 0, SC_N * sizeof(double), ctx_->stream));
      LBF_HIP(hipEventCreateWithFlags(&ev_anchor_, hipEventDisableTiming | event_release_flags()));
      LBF_HIP(hipEventCreateWithFlags(&ev_full_, hipEventDisableTiming | event_release_flags()));
    }
  }
}

int SlbfgsSolver::full_ahead_step(const EpochDraw &d) const {
  if (!fnet_ || d.pick < 0) return -2;
  // w_history at the epoch's end holds iterates w_{m+1-W} .. w_m (w_0: the anchor copy, w_{t+1}: after step t),
  // W = min(m + 1, L + 1) entries, the same count draw_epoch drew the pick over (s_lbfgs.hpp:265-266)
  const int m_inner = int(std::max(1LL, N_ / prm_.b));
  const int W = std::min(m_inner + 1, prm_.L + 1);
  const int j = m_inner + 1 - W + d.pick;
  return j - 1;
}

void SlbfgsSolver::post_full(const float *anchor) {
  hipStream_t s = ctx_->stream;
  LBF_HIP(hipEventRecord(ev_anchor_, s));
  LBF_HIP(hipStreamWaitEvent(fctx_->stream, ev_anchor_, 0));
  fnet_->loss_grad(anchor, mu_next_.get(), X_, Y_, nullptr, N_, 1.0 / double(N_), prm_.lambda, nullptr, fscal_.get());
  LBF_HIP(hipEventRecord(ev_full_, fctx_->stream));
  full_posted_ = true;
}

long long SlbfgsSolver::twin_post(std::function<void()> f) {
  if (!tw_) {
    f();
    return 0;
  }
  return tw_->post(std::move(f));
}

void SlbfgsSolver::twin_wait(long long ticket) {
  if (tw_) tw_->wait(ticket);
}

SlbfgsSolver::~SlbfgsSolver() {
  tw_.reset(); // runs what is queued, joins the helper thread
  for (auto e : ev_anc_) (void)hipEventDestroy(e);
  if (ev_fork_) (void)hipEventDestroy(ev_fork_);
  if (ev_join_) (void)hipEventDestroy(ev_join_);
  for (int i = 0; i < 2; ++i) {
    if (ev_g2_[i]) (void)hipEventDestroy(ev_g2_[i]);
    if (ev_free_[i]) (void)hipEventDestroy(ev_free_[i]);
  }
  if (fctx_) (void)hipStreamSynchronize(fctx_->stream);
  if (ev_anchor_) (void)hipEventDestroy(ev_anchor_);
  if (ev_full_) (void)hipEventDestroy(ev_full_);
}

void SlbfgsSolver::reduce_pair(const float *wa, const float *wb, float *gab, double inv_scale) {
  {
    ProfScope ps(ctx_, PK_ALLREDUCE);
    ctx_->allreduce(gab, size_t(2 * ng_)); // [ga | hi | lo | pad | gb | hi | lo | pad]
  }
  net_->finish_reduced(wa, gab, inv_scale, prm_.lambda, nullptr, nullptr);
  net_->finish_reduced(wb, gab + ng_, inv_scale, prm_.lambda, nullptr, nullptr);
}

void SlbfgsSolver::eval_pair(const float *wa, const float *wb, float *gab, long long off, long long count,
                             double inv_scale) {
  // the step's rows were gathered for the whole epoch (contiguous slices, same values in the same order
  // as the gathering GEMMs would read), which also lets the dW GEMM of layer 0 take the LDS-DMA path
  const int In = net_->layers().front().in, Out = net_->layers().back().out;
  const float *X = xg_.get() + off * In, *Y = yg_.get() + off * Out;
  float *ga = gab, *gb = gab + ng_;
  const bool dp = dp_inner();
  // gradients only: nobody reads a minibatch evaluation's loss or dots (scal = nullptr skips them)
  auto one = [&](Mlp *m, const float *w, float *g) {
    if (dp) m->loss_grad_local(w, g, X, Y, nullptr, count, inv_scale);
    else m->loss_grad(w, g, X, Y, nullptr, count, inv_scale, prm_.lambda, nullptr, nullptr);
  };
  if (!tnet_) {
    one(net_, wa, ga);
    one(net_, wb, gb);
  } else {
    LBF_HIP(hipEventRecord(ev_fork_, ctx_->stream)); // wa, wb, the gathered rows and gb's last reader are done
    const long long tk = twin_post([=]() {
      LBF_HIP(hipStreamWaitEvent(tctx_->stream, ev_fork_, 0));
      one(tnet_.get(), wb, gb);
      LBF_HIP(hipEventRecord(ev_join_, tctx_->stream));
    });
    try {
      one(net_, wa, ga);
    } catch (...) { // the task refers to this frame: let it finish first
      try {
        twin_wait(tk);
      } catch (...) {
      }
      throw;
    }
    twin_wait(tk); // ev_join_ recorded (and ev_fork_ waited for: it may be re-recorded after this)
    LBF_HIP(hipStreamWaitEvent(ctx_->stream, ev_join_, 0));
  }
  if (dp) reduce_pair(wa, wb, gab, inv_scale);
}

// SLBFGS::stochastic_solve (s_lbfgs.hpp:165-290) with the UnifiedSLBFGS_CPU closures
// (unified_optimization.hpp:343-400). The host RNG stream is consumed in exactly the reference's
// order; because no sample depends on device values, each epoch's index lists are drawn up front
// and uploaded once, and the epoch then runs without a host synchronisation.
int SlbfgsSolver::run(lbf_record *rec) {
  iterate(prm_.max_epochs, rec);
  return iters_;
}

// An epoch's index lists in the reference's RNG order (s_lbfgs.hpp:212-266). Every rank draws the same
// lists; with sliced data parallelism it keeps only its slice [b*rk/nr, b*(rk+1)/nr) of each batch (a
// replicated rank keeps every index). The minibatch slices come first
// in `flat` (minibatch t's rows right after minibatch t-1's, as Mlp::batch_grads reads them), the
// Hessian-batch slices after them; the draws stay in RNG order.
void SlbfgsSolver::draw_epoch(bool u_seen, EpochDraw &d) {
  const int nr = dp_inner() ? ctx_->nranks : 1, rk = dp_inner() ? ctx_->rank : 0;
  const int m_inner = int(std::max(1LL, N_ / prm_.b));
  const int L = prm_.L;
  d.flat.clear();
  d.hflat.clear();
  d.mb.assign(size_t(m_inner), Slice{});
  d.hb.assign(size_t(m_inner), Slice{-1, 0, 0});
  auto take = [&](size_t bsz, std::vector<int> &dst) {
    d.batch.clear();
    const long long tot = (long long)sampler_->draw(bsz, rng_, d.batch);
    long long a0, a1;
    rank_slice(tot, rk, nr, &a0, &a1);
    Slice sl{(long long)dst.size(), a1 - a0, tot};
    dst.insert(dst.end(), d.batch.begin() + a0, d.batch.begin() + a1);
    return sl;
  };
  int whist_size = 1;
  for (int t = 0; t < m_inner; ++t) {
    d.mb[t] = take(size_t(prm_.b), d.flat);
    whist_size = std::min(whist_size + 1, L + 1);
    if (t > 0 && t % L == 0) {
      if (u_seen) d.hb[t] = take(size_t(prm_.b_H), d.hflat);
      u_seen = true;
    }
  }
  const long long nmb_rows = (long long)d.flat.size();
  for (Slice &h : d.hb)
    if (h.off >= 0) h.off += nmb_rows;
  d.flat.insert(d.flat.end(), d.hflat.begin(), d.hflat.end());
  d.pick = -1;
  if (whist_size >= 2) {
    std::uniform_int_distribution<size_t> pk(0, size_t(whist_size) - 2); // s_lbfgs.hpp:266
    d.pick = int(pk(rng_));
  }
  d.u_seen = u_seen;
}

int SlbfgsSolver::wh_push_slot() {
  const int L = prm_.L;
  int slot;
  if (wh_count_ < L + 1) {
    slot = (wh_head_ + wh_count_) % (L + 1);
    ++wh_count_;
  } else {
    slot = wh_head_;
    wh_head_ = (wh_head_ + 1) % (L + 1);
  }
  return slot;
}

// The inner steps of one epoch (s_lbfgs.hpp:218-262), from the anchor copy to the last step; the epoch's
// rows are gathered (xg_, yg_) and the context stream is idle when this is called.
void SlbfgsSolver::epoch_steps(const EpochDraw &d) {
  hipStream_t s = ctx_->stream;
  const long long In = net_->layers().front().in, Out = net_->layers().back().out;
  const long long ld = round4(n_);
  const int m_inner = int(std::max(1LL, N_ / prm_.b));
  const int L = prm_.L;
  const bool dp = dp_inner();
  const auto &mb = d.mb, &hb = d.hb;
  LBF_HIP(hipMemcpyAsync(wt_.get(), w_.get(), size_t(n_) * sizeof(float), hipMemcpyDeviceToDevice, s));
  wh_head_ = 0;
  wh_count_ = 0;
  const int full_at = full_ahead_step(d);
  {
    const int slot = wh_push_slot();
    LBF_HIP(hipMemcpyAsync(wh_.get() + slot * ld, wt_.get(), size_t(n_) * sizeof(float), hipMemcpyDeviceToDevice,
                           s));
    if (full_at == -1) post_full(wh_.get() + slot * ld);
  }
  // The minibatch gradients at the anchor w (fixed for the epoch, and independent of the iterates) run one
  // step ahead on the twin stream: step t's evaluation at w_t and its direction on the context stream then
  // overlap the twin's gradient of minibatch t + 1 at w, instead of joining the two evaluations of each
  // step. Same evaluations on the same inputs: bitwise the same.
  // Free-running (no per-step collective): the anchor half of step t goes to its own buffer ganc_ + t ng_
  // (the epoch's 234 anchor gradients, 501 MB at cfg 4), so the twin never waits for the context stream to
  // release a block: no ev_free_ record on the context stream (≈ 5 µs of its time per step,
  // profiles/r03/launch_floor.txt) and no wait on the twin. When that buffer does not fit in free device
  // memory (keeping a quarter of it free), or its allocation fails, the twin falls back for good to two
  // blocks, double-buffered in the second half of gpair_[t & 1]. Sliced data parallelism keeps that packed
  // [g(w_t) | g(w)] block: both halves are this rank's partial sums until the step's one all-reduce.
  bool twin_free = !dp && free_twin_;
  if (twin_free) {
    const size_t need = size_t(m_inner) * size_t(ng_);
    if (ganc_.size() < need) {
      size_t fr = 0, tot = 0;
      const bool fits = hipMemGetInfo(&fr, &tot) == hipSuccess &&
                        double(need - ganc_.size()) * sizeof(float) <= 0.75 * double(fr);
      try {
        if (fits) ganc_.resize(need);
      } catch (const Error &) {
        (void)hipGetLastError();
      }
      if (ganc_.size() < need) {
        ganc_.resize(0);
        free_twin_ = twin_free = false;
      }
    }
  }
  if (twin_free) {
    while (ev_anc_.size() < size_t(m_inner)) {
      hipEvent_t e;
      LBF_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming | event_release_flags()));
      ev_anc_.push_back(e);
    }
  }
  auto g1 = [&](int t) { return gpair_[t & 1].get(); };
  auto g2 = [&](int t) { return twin_free ? ganc_.get() + (long long)t * ng_ : gpair_[t & 1].get() + ng_; };
  auto rows_x = [&](const Slice &sl) { return xg_.get() + sl.off * In; };
  auto rows_y = [&](const Slice &sl) { return yg_.get() + sl.off * Out; };
  // Tickets of the twin tasks (0: ran inline). Event order across the two host threads: task t + 2 (which
  // waits on ev_free_[t & 1]) is posted at step t + 1, after step t recorded that event; step t + 2
  // re-records it only after twin_wait(task t + 2), i.e. after that wait was enqueued. Task t records
  // ev_g2_[t & 1] and the context thread waits on it after twin_wait(task t); task t + 2 re-records it
  // only after being posted at step t + 1, after that wait.
  std::vector<long long> tk(size_t(std::max(m_inner, 1)), 0);
  auto anchor_ahead = [&](int t) { // twin stream: the anchor half of step t's block
    const Slice sl = mb[t];
    float *gdst = g2(t);
    const float *xr = rows_x(sl), *yr = rows_y(sl);
    hipEvent_t efree = twin_free ? nullptr : ev_free_[t & 1], eg2 = twin_free ? ev_anc_[size_t(t)] : ev_g2_[t & 1];
    tk[size_t(t)] = twin_post([=]() {
      if (efree) LBF_HIP(hipStreamWaitEvent(tctx_->stream, efree, 0)); // step t - 2's direction read it
      if (dp)
        tnet_->loss_grad_local(w_.get(), gdst, xr, yr, nullptr, sl.cnt, 1.0 / double(sl.total));
      else
        tnet_->loss_grad(w_.get(), gdst, xr, yr, nullptr, sl.cnt, 1.0 / double(sl.total), prm_.lambda, nullptr,
                         nullptr);
      LBF_HIP(hipEventRecord(eg2, tctx_->stream));
    });
  };
  // LBF_HOST_TIMING=2: host time of each part of the inner step's enqueue (where the epoch's host-bound
  // ~130 us per step go)
  using hclk = std::chrono::steady_clock;
  double ht[6] = {0, 0, 0, 0, 0, 0}; // twin, main eval, events, direction, combine, Hessian step
  auto tick = [&]() { return host_timing_ >= 2 ? hclk::now() : hclk::time_point(); };
  auto tock = [&](int i, hclk::time_point a) {
    if (host_timing_ >= 2) ht[i] += std::chrono::duration<double, std::micro>(hclk::now() - a).count();
  };
  if (!twin_free) {
    // the twin may reuse block t & 1 once the direction of step t - 2 has read it: nothing of this epoch
    // has yet
    LBF_HIP(hipEventRecord(ev_free_[0], s));
    LBF_HIP(hipEventRecord(ev_free_[1], s));
  } else {
    // the twin's first launch must follow this epoch's gather and w (same role as ev_free_ above)
    LBF_HIP(hipEventRecord(ev_fork_, s));
    LBF_HIP(hipStreamWaitEvent(tctx_->stream, ev_fork_, 0));
  }
  anchor_ahead(0);
  RedAllArgs gred; // the main evaluation's split-K slabs, finished by the direction sweep
  for (int t = 0; t < m_inner; ++t) {
    const Slice &sl = mb[t];
    const double inv_b = 1.0 / double(sl.total);
    const float *gb = g2(t);
    {
      auto h0 = tick();
      if (t + 1 < m_inner) anchor_ahead(t + 1);
      tock(0, h0);
      h0 = tick();
      if (dp)
        net_->loss_grad_local(wt_.get(), g1(t), rows_x(sl), rows_y(sl), nullptr, sl.cnt, inv_b);
      else // the gradient's last reduction runs inside the direction sweep (one launch fewer per step)
        net_->loss_grad_deferred(wt_.get(), g1(t), rows_x(sl), rows_y(sl), nullptr, sl.cnt, inv_b, prm_.lambda,
                                 &gred);
      tock(1, h0);
      h0 = tick();
      twin_wait(tk[size_t(t)]); // task t recorded ev_g2_[t & 1] / ev_anc_[t]
      LBF_HIP(hipStreamWaitEvent(ctx_->stream, twin_free ? ev_anc_[size_t(t)] : ev_g2_[t & 1], 0));
      tock(2, h0);
      if (dp) reduce_pair(wt_.get(), w_.get(), g1(t), inv_b);
    }
    GramArgs ga;
    ga.policy = POL_SLBFGS;
    ga.has_g = 1;
    ga.ga = g1(t);
    ga.gb = gb;
    ga.gc = mu_.get();
    ga.g_out = v_.get();
    auto h0 = tick();
    const int slot = wh_push_slot();
    // r = H v (two-loop), then wt = wt - step * r ; w_history.push_back(wt)
    hist_.update_combine(ga, 1, +1.0, wt_.get(), wt_.get(), wh_.get() + slot * ld, -prm_.step, dp ? nullptr : &gred);
    tock(3, h0);
    h0 = tick();
    if (!twin_free) LBF_HIP(hipEventRecord(ev_free_[t & 1], ctx_->stream)); // block t & 1 read (v formed)
    tock(2, h0);
    if (t == full_at) post_full(wh_.get() + slot * ld); // the picked iterate w_{t+1} now exists
    h0 = tick();
    if (t > 0 && t % L == 0) {
      int slots[64];
      for (int i = 0; i < wh_count_; ++i) slots[i] = wh_slot(i);
      average_slots(s, n_, wh_.get(), ld, slots, wh_count_, u_.get());
      // diagnostics (lbf_slbfgs_pair_io): this event's record [w_{t+1} | u | g+ | g-] and forced inputs
      const int ev = nev_++;
      float *pr = pio_rec_ && ev < pio_cap_ ? pio_rec_ + size_t(ev) * 4 * size_t(ld) : nullptr;
      const float *pf = pio_force_ && ev < pio_cap_ ? pio_force_ + size_t(ev) * 4 * size_t(ld) : nullptr;
      const size_t nb = size_t(n_) * sizeof(float);
      if (pr) {
        LBF_HIP(hipMemcpyAsync(pr, wt_.get(), nb, hipMemcpyDeviceToDevice, s));
        LBF_HIP(hipMemcpyAsync(pr + ld, u_.get(), nb, hipMemcpyDeviceToDevice, s));
        LBF_HIP(hipMemsetAsync(pr + 2 * ld, 0, 2 * nb + 2 * (size_t(ld) - size_t(n_)) * sizeof(float), s));
      }
      if (pf) LBF_HIP(hipMemcpyAsync(u_.get(), pf + ld, nb, hipMemcpyDeviceToDevice, s));
      if (have_u_) {
        const Slice &hs = hb[t];
        const double eps = prm_.fd_eps;
        lincomb(s, n_, u_.get(), -1.0, up_.get(), s_.get()); // s = u - u_prev
        GramArgs pa;
        pa.policy = POL_SLBFGS;
        pa.has_pair = 1;
        pa.sa = u_.get();
        pa.sb = up_.get();
        float *gp = fdpair_.get(), *gm = fdpair_.get() + ng_;
        if (prm_.hvp_exact) { // y = H(u) s on the b_H batch, R-operator, or the Gauss-Newton G(u) s (hvp.hip)
          if (prm_.hvp_exact == LBF_HVP_GAUSS_NEWTON)
            net_->gnvp(u_.get(), s_.get(), X_, Y_, idx_.get() + hs.off, hs.cnt, 1.0 / double(hs.total), prm_.lambda,
                       gp);
          else
            net_->hvp(u_.get(), s_.get(), X_, Y_, idx_.get() + hs.off, hs.cnt, 1.0 / double(hs.total), prm_.lambda,
                      gp);
          LBF_HIP(hipMemsetAsync(gm, 0, size_t(n_) * sizeof(float), s));
          pa.yscale = 1.0;
        } else { // s_lbfgs.hpp:88-101: central difference of two batch gradients
          lincomb(s, n_, u_.get(), eps, s_.get(), wp_.get()); // fd_hvp_grads, the two evaluations paired
          lincomb(s, n_, u_.get(), -eps, s_.get(), wm_.get());
          eval_pair(wp_.get(), wm_.get(), fdpair_.get(), hs.off, hs.cnt, 1.0 / double(hs.total));
          pa.yscale = 1.0 / (2.0 * eps);
        }
        if (pr) {
          LBF_HIP(hipMemcpyAsync(pr + 2 * ld, gp, nb, hipMemcpyDeviceToDevice, s));
          LBF_HIP(hipMemcpyAsync(pr + 3 * ld, gm, nb, hipMemcpyDeviceToDevice, s));
        }
        if (pf) {
          LBF_HIP(hipMemcpyAsync(gp, pf + 2 * ld, nb, hipMemcpyDeviceToDevice, s));
          LBF_HIP(hipMemcpyAsync(gm, pf + 3 * ld, nb, hipMemcpyDeviceToDevice, s));
        }
        pa.ya = gp;
        pa.yb = gm;
        hist_.update(pa, 0, 1, +1.0);
        if (prm_.pair_trace && npairs_ < prm_.pair_trace_cap) trace_pair(iters_, t);
      }
      LBF_HIP(hipMemcpyAsync(up_.get(), u_.get(), size_t(n_) * sizeof(float), hipMemcpyDeviceToDevice, s));
      have_u_ = true;
    }
    tock(5, h0);
  }
  if (tw_) tw_->wait_all(); // every twin task of the epoch enqueued
  if (host_timing_ >= 2)
    std::fprintf(stderr, "[lbf host] per inner step (us): twin %.1f, main eval %.1f, events %.1f, direction %.1f, "
                 "combine %.1f, Hessian step %.1f\n", ht[0] / m_inner, ht[1] / m_inner, ht[2] / m_inner,
                 ht[3] / m_inner, ht[4] / m_inner, ht[5] / m_inner);
}

int SlbfgsSolver::iterate(int epochs, lbf_record *rec) {
  ctx_->set_device();
  hipStream_t s = ctx_->stream;
  const long long In = net_->layers().front().in, Out = net_->layers().back().out;
  const long long ld = round4(n_);
  const int nr = ctx_->nranks, rk = ctx_->rank;
  const int m_inner = int(std::max(1LL, N_ / prm_.b));
  for (Ctx *c : {tctx_.get(), fctx_.get()})
    if (c) copy_prof_settings(*ctx_, *c);
  if (!started_) {
    LBF_HIP(hipMemcpyAsync(w_.get(), user_params_, size_t(n_) * sizeof(float), hipMemcpyDeviceToDevice, s));
    t0_ = std::chrono::steady_clock::now();
    rw_ = RecordWriter(rec);
    started_ = true;
  }
  rw_.retarget(rec); // the row index is the first call's, the record each call's own
  // full-batch shard of this rank
  const long long lo = N_ * rk / nr, hi = N_ * (rk + 1) / nr;
  const float *Xs = X_ + lo * In, *Ys = Y_ + lo * Out;
  const double inv_full = 1.0 / double(N_);
  auto eval_full = [&](const float *w, float *g) {
    net_->loss_grad(w, g, Xs, Ys, nullptr, hi - lo, inv_full, prm_.lambda, nullptr, hist_.scal());
  };
  auto read = [&]() { hs_.read(s, hist_.scal()); };
  const int target = iters_ + std::max(0, epochs);
  const int done0 = iters_;
  while (iters_ < target && !converged_) {
    if (!mu_valid_) {
      if (repl_ && nr > 1) replica_fingerprints(); // the caller's parameters must agree too
      eval_full(w_.get(), mu_.get());
      read();
      if (repl_ && nr > 1) replica_check();
    }
    if (std::sqrt(hs_[SC_TGG]) < prm_.tol) { // s_lbfgs.hpp:208
      converged_ = true;
      break;
    }
    // --- this epoch's samples in reference order (drawn during the previous epoch when it ran) -------
    if (next_ready_) std::swap(cur_, next_);
    else draw_epoch(have_u_, cur_);
    next_ready_ = false;
    const std::vector<int> &flat = cur_.flat;
    const int pick = cur_.pick;
    idx_.ensure(std::max<size_t>(1, flat.size()));
    if (!flat.empty()) { // through pinned staging: an asynchronous copy (the stream was synchronised by read())
      idx_host_.ensure(flat.size());
      std::memcpy(idx_host_.get(), flat.data(), flat.size() * sizeof(int));
      LBF_HIP(hipMemcpyAsync(idx_.get(), idx_host_.get(), flat.size() * sizeof(int), hipMemcpyHostToDevice, s));
    }
    // this rank's sampled rows of the epoch gathered once, in sampling order: step t's minibatch slice (and
    // its Hessian batch slice) is then contiguous (batch_g's column gather, unified_optimization.hpp:361-364)
    xg_.ensure(std::max<size_t>(1, flat.size()) * size_t(In));
    yg_.ensure(std::max<size_t>(1, flat.size()) * size_t(Out));
    gather_rows(s, X_, In, idx_.get(), (long long)flat.size(), int(In), xg_.get());
    gather_rows(s, Y_, Out, idx_.get(), (long long)flat.size(), int(Out), yg_.get());
    // No host synchronisation here: the upload reads pinned staging (rewritten only after the next read()),
    // and every consumer of the gathered rows is ordered after the gathers (the context stream, and the
    // twin through the event it waits on at the epoch's start), so the host enqueues the first inner step
    // while the gathers run.
    // --- epoch -----------------------------------------------------------------------------------
    const auto th0 = std::chrono::steady_clock::now();
    {
      // replicated data parallelism: the inner steps evaluate without the communicator
      LocalOnly lo_guard(ctx_, repl_);
      epoch_steps(cur_);
    }
    if (host_timing_) { // host time to enqueue the epoch's inner steps vs the epoch on the device
      const auto th1 = std::chrono::steady_clock::now();
      LBF_HIP(hipStreamSynchronize(s));
      const auto th2 = std::chrono::steady_clock::now();
      std::fprintf(stderr, "[lbf host] epoch %d: %d inner steps enqueued in %.3f ms, device done %.3f ms later\n",
                   iters_, m_inner, std::chrono::duration<double, std::milli>(th1 - th0).count(),
                   std::chrono::duration<double, std::milli>(th2 - th1).count());
    }
    // the next epoch's lists, drawn while the GPU runs this epoch's queued steps
    if (iters_ + 1 < target || iters_ + 1 < prm_.max_epochs) {
      draw_epoch(cur_.u_seen, next_);
      next_ready_ = true;
    }
    // anchor reset (s_lbfgs.hpp:265-270)
    const float *anchor = pick >= 0 ? wh_.get() + wh_slot(pick) * ld : wt_.get();
    LBF_HIP(hipMemcpyAsync(w_.get(), anchor, size_t(n_) * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (repl_ && nr > 1) replica_fingerprints(); // compared after read(): no extra host wait
    // recorder (s_lbfgs.hpp:274-284): full loss and gradient at the new anchor == next epoch's mu
    if (full_posted_) { // evaluated ahead on the third stream (fnet_): join, take its gradient and status words
      LBF_HIP(hipStreamWaitEvent(s, ev_full_, 0));
      std::swap(mu_, mu_next_);
      double *hsc = hist_.scal();
      LBF_HIP(hipMemcpyAsync(hsc + SC_LOSS, fscal_.get() + SC_LOSS, 2 * sizeof(double), hipMemcpyDeviceToDevice, s));
      LBF_HIP(hipMemcpyAsync(hsc + SC_WW, fscal_.get() + SC_WW, 2 * sizeof(double), hipMemcpyDeviceToDevice, s));
      full_posted_ = false;
    } else {
      eval_full(w_.get(), mu_.get());
    }
    read();
    if (repl_ && nr > 1) replica_check();
    if (hs_[SC_KERR] != 0.0) // dir_combine_kernel's check of the coefficient map against the ring's live count
      throw Error(LBF_ERR_STATE, "S-LBFGS: a direction step found the coefficient map K out of step with the "
                                 "history ring's live count (epoch " + std::to_string(iters_) + ")");
    mu_valid_ = true;
    last_loss_ = hs_[SC_LOSS];
    last_gnorm_ = std::sqrt(hs_[SC_TGG]);
    rw_.put(last_loss_, last_gnorm_, ms_since(t0_), prm_.step, 0, int(hs_[SC_COUNT])); // accepted: the live pairs
    ++iters_;
  }
  LBF_HIP(hipMemcpyAsync(user_params_, w_.get(), size_t(n_) * sizeof(float), hipMemcpyDeviceToDevice, s));
  LBF_HIP(hipStreamSynchronize(s));
  if (tctx_) {
    LBF_HIP(hipStreamSynchronize(tctx_->stream));
    tctx_->prof.merge_into(ctx_->prof);
  }
  if (fctx_) {
    LBF_HIP(hipStreamSynchronize(fctx_->stream));
    fctx_->prof.merge_into(ctx_->prof);
  }
  return iters_ - done0;
}

void SlbfgsSolver::replica_fingerprints() {
  hipStream_t s = ctx_->stream;
  const size_t cnt = 4 * size_t(ctx_->nranks);
  fp_.ensure(cnt);
  hfp_.ensure(cnt);
  LBF_HIP(hipMemsetAsync(fp_.get(), 0, cnt * sizeof(float), s));
  fingerprint(s, n_, w_.get(), ctx_->rank, fp_.get());
  ctx_->allreduce(fp_.get(), cnt);
  LBF_HIP(hipMemcpyAsync(hfp_.get(), fp_.get(), cnt * sizeof(float), hipMemcpyDeviceToHost, s));
}

void SlbfgsSolver::replica_check() const {
  const float *f = hfp_.get();
  for (int r = 1; r < ctx_->nranks; ++r)
    for (int i = 0; i < 4; ++i)
      if (f[4 * r + i] != f[i])
        throw Error(LBF_ERR_STATE, "S-LBFGS replicated data parallelism: rank " + std::to_string(r) +
                                       "'s anchor differs from rank 0's at the full-batch evaluation of epoch " +
                                       std::to_string(iters_) + " (the replicated ranks' parameters drifted apart)");
}

// Diagnostics row of the pair just offered to the ring (lbf_slbfgs_params.pair_trace): synchronous.
void SlbfgsSolver::trace_pair(int epoch, int t) {
  hipStream_t s = ctx_->stream;
  const HistView v = hist_.view();
  hs_.enqueue(s, v.scal);
  int wslot = 0;
  LBF_HIP(hipMemcpyAsync(&wslot, v.ist + IST_WSLOT, sizeof(int), hipMemcpyDeviceToHost, s));
  LBF_HIP(hipStreamSynchronize(s));
  double ss = 0.0, yy = 0.0;
  const size_t d = size_t(wslot) * size_t(v.slots) + size_t(wslot);
  LBF_HIP(hipMemcpyAsync(&ss, v.SS + d, sizeof(double), hipMemcpyDeviceToHost, s));
  LBF_HIP(hipMemcpyAsync(&yy, v.YY + d, sizeof(double), hipMemcpyDeviceToHost, s));
  LBF_HIP(hipStreamSynchronize(s));
  if (npairs_ == 0) { // the iterate after step t, u, s = u - u_prev and the y just stored in the ring
    const size_t nb = size_t(n_) * sizeof(float), ld = size_t(round4(n_));
    p0_.resize(4 * ld);
    const float *src[4] = {wt_.get(), u_.get(), s_.get(), v.Y + size_t(wslot) * size_t(v.ld)};
    for (int i = 0; i < 4; ++i)
      LBF_HIP(hipMemcpyAsync(p0_.get() + i * ld, src[i], nb, hipMemcpyDeviceToDevice, s));
    LBF_HIP(hipStreamSynchronize(s));
    p0_set_ = true;
  }
  double *row = prm_.pair_trace + size_t(npairs_++) * LBF_PAIR_TRACE_COLS;
  const double vals[LBF_PAIR_TRACE_COLS] = {double(epoch), double(t), hs_[SC_YS], ss, yy, hs_[SC_ACCEPT],
                                            hs_[SC_COUNT], 0.0};
  for (int i = 0; i < LBF_PAIR_TRACE_COLS; ++i) row[i] = vals[i];
}

bool SlbfgsSolver::pair0(float *wt, float *u, float *s, float *y) const {
  if (!p0_set_) return false;
  const size_t nb = size_t(n_) * sizeof(float), ld = size_t(round4(n_));
  float *dst[4] = {wt, u, s, y};
  for (int i = 0; i < 4; ++i)
    if (dst[i]) LBF_HIP(hipMemcpyAsync(dst[i], p0_.get() + i * ld, nb, hipMemcpyDeviceToDevice, ctx_->stream));
  LBF_HIP(hipStreamSynchronize(ctx_->stream));
  return true;
}

void SlbfgsSolver::info(lbf_solve_info *out) const {
  if (!out) return;
  cnt_.fill(out, iters_, last_loss_, last_gnorm_);
  for (const Mlp *side : {tnet_.get(), fnet_.get()}) { // the side networks' totals on top
    if (!side) continue;
    out->n_evals += side->evals();
    out->n_rows += side->rows();
  }
}

} // namespace lbf
