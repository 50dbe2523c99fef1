// GD and SGD (with momentum) drivers (see solvers.hpp).
#include "solvers.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

// Host-side acceptance tests must round like ls_ctl_kernel (and the reference's host code).
#pragma clang fp contract(off)

namespace lbf {

// CudaGD::solve (gd.cuh:38-106): the loss/grad callback is one fused evaluation; the reference's
// blocking cublasSnrm2 becomes the evaluation's g.g, read with the loss once per iteration.
int run_gd(Mlp *net, const lbf_gd_params &prm, float *d_params, const float *X, const float *Y, long long n_local,
           long long n_global, lbf_record *rec, lbf_solve_info *info) {
  LBF_REQUIRE(d_params && n_local >= 0 && n_global > 0 && (n_local == 0 || (X && Y)), "bad argument");
  Ctx *c = net->ctx();
  c->set_device();
  hipStream_t s = c->stream;
  const long long n = (long long)net->nparams();
  DevBuf<float> g(size_t(round4(n + 2))), v(size_t(std::max(1LL, n)));
  DevBuf<double> scal(SC_N);
  StatusMirror hs;
  LBF_HIP(hipMemsetAsync(v.get(), 0, size_t(n) * sizeof(float), s));
  const SolveCounters<Mlp> cnt(net);
  const double l2 = net->l2(); // weight decay: loss + 0.5 l2 |w|^2, g + l2 w (the evaluation's finalize path)
  auto eval = [&]() {
    net->loss_grad(d_params, g.get(), X, Y, nullptr, n_local, 1.0 / double(n_global), l2, nullptr, scal.get());
    hs.read(s, scal.get());
  };
  const float lr = float(prm.lr), mom = float(prm.momentum), tol = float(prm.tol);
  eval();
  const auto t0 = std::chrono::steady_clock::now();
  RecordWriter rw(rec);
  int done = 0;
  for (int it = 0; it < prm.max_iters; ++it) {
    if (float(std::sqrt(hs[SC_TGG])) < tol) break; // gd.cuh:73
    momentum_step(s, n, mom, lr, nullptr, g.get(), v.get(), d_params);
    eval();
    // loss and norm through float, like the reference's recorder
    rw.put(double(float(hs[SC_LOSS])), double(float(std::sqrt(hs[SC_TGG]))), ms_since(t0), double(lr), 0, -1);
    ++done;
  }
  cnt.fill(info, done, hs[SC_LOSS], std::sqrt(hs[SC_TGG]));
  return done;
}

// CudaSGD::solve (sgd.cuh:50-153). Batch losses accumulate on the device (epoch_loss_acc, fp32 like
// the reference's host sum), so an epoch synchronises once, not once per batch. Under weight decay (the
// network's l2) every batch objective is batch loss + 0.5 l2 |w|^2 at the batch's own w, so the epoch loss is the
// row-weighted mean of the batch objectives, penalty included.
int run_sgd(Mlp *net, const lbf_sgd_params &prm, float *d_params, const float *X, const float *Y, long long N,
            lbf_record *rec, lbf_solve_info *info) {
  LBF_REQUIRE(d_params && X && Y && N > 0 && prm.batch > 0, "bad argument");
  Ctx *c = net->ctx();
  LBF_REQUIRE(!c->dp(), "SGD runs on one rank (the reference's contiguous batches have no shard split)");
  c->set_device();
  hipStream_t s = c->stream;
  const long long n = (long long)net->nparams();
  const int In = net->layers().front().in, Out = net->layers().back().out;
  DevBuf<float> g(size_t(round4(n + 2))), v(size_t(std::max(1LL, n))), esum(1);
  DevBuf<double> scal(SC_N);
  StatusMirror hs;
  PinnedBuf<float> he;
  he.ensure(1);
  LBF_HIP(hipMemsetAsync(v.get(), 0, size_t(n) * sizeof(float), s));
  const SolveCounters<Mlp> cnt(net);
  const double l2 = net->l2();
  const float mom = float(prm.momentum), tol = float(prm.tol);
  float cur_lr = float(prm.lr);
  const long long nb = cdiv(N, prm.batch);
  float prev = std::numeric_limits<float>::infinity();
  const auto t0 = std::chrono::steady_clock::now();
  RecordWriter rw(rec);
  int done = 0;
  // the recorder's full-batch loss and norm, through float like the reference's; the start point's row at time 0
  auto full_record = [&](bool start) {
    net->loss_grad(d_params, g.get(), X, Y, nullptr, N, 1.0 / double(N), l2, nullptr, scal.get());
    hs.read(s, scal.get());
    rw.put(double(float(hs[SC_LOSS])), double(float(std::sqrt(hs[SC_TGG]))), start ? 0.0 : ms_since(t0),
           double(cur_lr), 0, -1);
  };
  if (rec) { // sgd.cuh:93-98
    full_record(true);
    ++done;
  }
  for (int it = 0; it < prm.max_epochs; ++it) {
    if (prm.decay_step > 0 && it > 0 && it % prm.decay_step == 0) cur_lr *= float(prm.decay_rate); // :101-103
    LBF_HIP(hipMemsetAsync(esum.get(), 0, sizeof(float), s));
    for (long long b = 0; b < nb; ++b) { // :107-127
      const long long r0 = b * prm.batch, bs = std::min<long long>(prm.batch, N - r0);
      net->loss_grad(d_params, g.get(), X + r0 * In, Y + r0 * Out, nullptr, bs, 1.0 / double(bs), l2, nullptr,
                     scal.get());
      epoch_loss_acc(s, scal.get(), bs, esum.get());
      momentum_step(s, n, mom, cur_lr, nullptr, g.get(), v.get(), d_params);
    }
    LBF_HIP(hipMemcpyAsync(he.get(), esum.get(), sizeof(float), hipMemcpyDeviceToHost, s));
    LBF_HIP(hipStreamSynchronize(s));
    const float avg = he[0] / float(N);
    if (tol > 0.0f && std::isfinite(prev)) { // :129-135
      const float rel = std::fabs(prev - avg) / std::max(1.0f, std::fabs(prev));
      if (rel < tol) break;
    }
    prev = avg;
    if (rec) full_record(false); // :138-148
    ++done;
  }
  cnt.fill(info, done, rec ? hs[SC_LOSS] : double(prev), rec ? std::sqrt(hs[SC_TGG]) : 0.0);
  return done;
}

} // namespace lbf
