// Adam / AdamW driver (see solvers.hpp; the algorithm is stated at lbf_adam_solve in lbfgs_amd.h).
#include "solvers.hpp"

#include <algorithm>
#include <cmath>

// The coefficients are fp64 expressions rounded once: no fused multiply-add (a Python restatement gives the bits).
#pragma clang fp contract(off)

namespace lbf {

static_assert(sizeof(AdamCoef) == sizeof(lbf_adam_coef) && sizeof(AdamCoef) == 9 * sizeof(float), "coefficient layout");

void adam_check(const lbf_adam_params &p) {
  LBF_REQUIRE(p.batch >= 1, "batch must be >= 1");
  LBF_REQUIRE(std::isfinite(p.lr) && p.lr > 0.0, "lr must be finite and > 0");
  LBF_REQUIRE(std::isfinite(p.eps) && p.eps > 0.0, "eps must be finite and > 0");
  LBF_REQUIRE(p.beta1 >= 0.0 && p.beta1 < 1.0, "beta1 must lie in [0, 1)");
  LBF_REQUIRE(p.beta2 >= 0.0 && p.beta2 < 1.0, "beta2 must lie in [0, 1)");
  LBF_REQUIRE(std::isfinite(p.weight_decay) && p.weight_decay >= 0.0, "weight_decay must be finite and >= 0");
  LBF_REQUIRE(std::isfinite(p.clip_norm) && p.clip_norm >= 0.0, "clip_norm must be finite and >= 0");
  LBF_REQUIRE(std::isfinite(p.decay_rate) && p.decay_step >= 0, "decay_rate must be finite, decay_step >= 0");
  LBF_REQUIRE(p.max_epochs >= 0 && p.trace_cap >= 0, "max_epochs and trace_cap must be >= 0");
}

AdamCoef adam_coefs(const lbf_adam_params &p, double lr_now, double p1, double p2) {
  AdamCoef k;
  k.b1 = float(p.beta1);
  k.a1 = float(1.0 - p.beta1);
  k.b2 = float(p.beta2);
  k.a2 = float(1.0 - p.beta2);
  k.step = float(lr_now / (1.0 - p1));
  k.rbc2 = float(1.0 / std::sqrt(1.0 - p2));
  k.eps = float(p.eps);
  k.decay = float(1.0 - lr_now * p.weight_decay);
  k.clip = float(p.clip_norm);
  return k;
}

AdamSolver::AdamSolver(Mlp *net, const lbf_adam_params &prm, float *d_params, const float *X, const float *Y,
                       long long N)
    : net_(net), ctx_(net->ctx()), prm_(prm), w_(d_params), X_(X), Y_(Y), N_(N), n_((long long)net->nparams()),
      nb_(0), l2_(net->l2()), cnt_(net) {
  LBF_REQUIRE(d_params && X && Y, "null pointer");
  nb_ = cdiv(N_, prm_.batch);
  ctx_->set_device();
  hipStream_t s = ctx_->stream;
  g_.resize(size_t(round4(n_ + 2)));
  m_.resize(size_t(std::max(1LL, n_)));
  v_.resize(size_t(std::max(1LL, n_)));
  LBF_HIP(hipMemsetAsync(m_.get(), 0, size_t(n_) * sizeof(float), s));
  LBF_HIP(hipMemsetAsync(v_.get(), 0, size_t(n_) * sizeof(float), s));
  scal_.resize(SC_N);
  acc_.resize(size_t(1 + nb_));
  hacc_.ensure(size_t(1 + nb_));
  if (prm_.shuffle) {
    order_.resize(size_t(N_));
    idx_.resize(size_t(N_));
    hidx_.ensure(size_t(N_));
    rng_.seed(prm_.seed);
  }
  lr_e_ = prm_.lr;
}

// the recorder's full-batch loss and norm through float, like run_sgd's; each rank its share of the rows
void AdamSolver::full_record(bool start) {
  const int nr = ctx_->dp() ? ctx_->nranks : 1, rk = ctx_->dp() ? ctx_->rank : 0;
  const int In = net_->layers().front().in, Out = net_->layers().back().out;
  long long a0, a1;
  rank_slice(N_, rk, nr, &a0, &a1);
  net_->loss_grad(w_, g_.get(), X_ + a0 * In, Y_ + a0 * Out, nullptr, a1 - a0, 1.0 / double(N_), l2_, nullptr,
                  scal_.get());
  hs_.read(ctx_->stream, scal_.get());
  rw_.put(double(float(hs_[SC_LOSS])), double(float(std::sqrt(hs_[SC_TGG]))), start ? 0.0 : ms_since(t0_), lr_e_, 0,
          -1);
  recorded_ = true;
}

int AdamSolver::iterate(int epochs, lbf_record *rec) {
  ctx_->set_device();
  hipStream_t s = ctx_->stream;
  const int nr = ctx_->dp() ? ctx_->nranks : 1, rk = ctx_->dp() ? ctx_->rank : 0;
  const int In = net_->layers().front().in, Out = net_->layers().back().out;
  if (!started_) {
    rw_ = RecordWriter(rec);
    t0_ = std::chrono::steady_clock::now();
    started_ = true;
    if (rec) {
      full_record(true);
      ++rows_done_;
    }
  }
  rw_.retarget(rec);
  int ran = 0;
  while (ran < epochs && !converged_) {
    if (prm_.decay_step > 0 && epoch_ > 0 && epoch_ % prm_.decay_step == 0) lr_e_ *= prm_.decay_rate;
    if (prm_.shuffle) { // this rank's slice of every batch, batch after batch; one upload per epoch
      epoch_order(rng_, N_, order_.data());
      long long off = 0;
      for (long long b = 0; b < nb_; ++b) {
        const long long r0 = b * prm_.batch, bs = std::min<long long>(prm_.batch, N_ - r0);
        long long a0, a1;
        rank_slice(bs, rk, nr, &a0, &a1);
        std::copy(order_.begin() + (r0 + a0), order_.begin() + (r0 + a1), hidx_.get() + off);
        off += a1 - a0;
      }
      if (off > 0)
        LBF_HIP(hipMemcpyAsync(idx_.get(), hidx_.get(), size_t(off) * sizeof(int), hipMemcpyHostToDevice, s));
    }
    LBF_HIP(hipMemsetAsync(acc_.get(), 0, sizeof(double), s));
    const long long t_epoch = t_;
    long long off = 0;
    for (long long b = 0; b < nb_; ++b) {
      const long long r0 = b * prm_.batch, bs = std::min<long long>(prm_.batch, N_ - r0);
      long long a0, a1;
      rank_slice(bs, rk, nr, &a0, &a1);
      if (prm_.shuffle)
        net_->loss_grad(w_, g_.get(), X_, Y_, idx_.get() + off, a1 - a0, 1.0 / double(bs), l2_, nullptr, scal_.get());
      else // the identity order: the batch's rows by pointer offset, no gather
        net_->loss_grad(w_, g_.get(), X_ + (r0 + a0) * In, Y_ + (r0 + a0) * Out, nullptr, a1 - a0, 1.0 / double(bs),
                        l2_, nullptr, scal_.get());
      off += a1 - a0;
      ++t_;
      p1_ *= prm_.beta1;
      p2_ *= prm_.beta2;
      AdamLoss ls;
      ls.scal = scal_.get();
      ls.rows = double(bs);
      ls.esum = acc_.get();
      ls.trace = acc_.get() + 1 + b;
      adam_step(s, n_, adam_coefs(prm_, lr_e_, p1_, p2_), g_.get(), m_.get(), v_.get(), w_,
                prm_.clip_norm > 0.0 ? scal_.get() + SC_TGG : nullptr, ls);
    }
    LBF_HIP(hipMemcpyAsync(hacc_.get(), acc_.get(), size_t(1 + nb_) * sizeof(double), hipMemcpyDeviceToHost, s));
    LBF_HIP(hipStreamSynchronize(s));
    if (prm_.loss_trace)
      for (long long b = 0; b < nb_ && t_epoch + b < prm_.trace_cap; ++b) prm_.loss_trace[t_epoch + b] = hacc_[1 + b];
    const double avg = hacc_[0] / double(N_);
    ++epoch_;
    ++ran;
    if (prm_.tol > 0.0 && have_prev_ && std::isfinite(prev_)) { // run_sgd's test, on the fp64 epoch mean
      const double rel = std::fabs(prev_ - avg) / std::max(1.0, std::fabs(prev_));
      if (rel < prm_.tol) {
        converged_ = true;
        break;
      }
    }
    prev_ = avg;
    have_prev_ = true;
    if (rec) full_record(false);
    ++rows_done_;
  }
  return ran;
}

void AdamSolver::info(lbf_solve_info *out) const {
  cnt_.fill(out, rows_done_, recorded_ ? hs_[SC_LOSS] : prev_, recorded_ ? std::sqrt(hs_[SC_TGG]) : 0.0);
}

} // namespace lbf
