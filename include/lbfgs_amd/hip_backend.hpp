// include/lbfgs_amd/hip_backend.hpp — header-only C++ mirror of the reference's unified API for a
// HipBackend, written purely against the C ABI (include/lbfgs_amd.h; link -llbfgs_amd). Plain C++17:
// no HIP, Eigen or torch headers are needed to compile it.
//
// Reference interfaces mirrored (paths relative to SignorB/lbfgs-FFNN):
//   hip_mlp::HipMinimizerBase / HipLBFGS     <- cuda_mlp::CudaMinimizerBase / CudaLBFGS
//                                               (src/cuda/minimizer_base.cuh:12-67, src/cuda/lbfgs.cuh:25-266)
//   hip_mlp::HipNetwork                      <- cuda_mlp::CudaNetwork (src/cuda/network.cuh:21-158)
//   hip_mlp::DeviceBuffer<T>                 <- cuda_mlp::DeviceBuffer (src/cuda/device_buffer.cuh:7-96)
//   hip_mlp::HipHandle                       <- cuda_mlp::CublasHandle (src/cuda/cublas_handle.cuh:22-39)
//   IterationRecorder<HipBackend>            <- IterationRecorder<CudaBackend> (src/iteration_recorder.hpp:98-146)
//   NetworkWrapper<HipBackend>               <- NetworkWrapper<CudaBackend> (src/network_wrapper.hpp:92-110)
//   UnifiedOptimizer<HipBackend>, UnifiedLBFGS_HIP, UnifiedSLBFGS_HIP
//                                            <- UnifiedOptimizer<CudaBackend>, UnifiedLBFGS_CUDA
//                                               (src/unified_optimization.hpp:420-592; S-LBFGS is CPU-only there)
//   UnifiedLauncher<HipBackend>              <- UnifiedLauncher<CudaBackend> (src/unified_launcher.hpp:83-205)
// Standalone, the header also defines UnifiedConfig / UnifiedDataset (same fields as
// src/unified_optimization.hpp:26-59) with a column-major HostMatrix in place of Eigen::MatrixXd.
// Dropped in next to the reference headers, define LBF_USE_REFERENCE_UNIFIED_TYPES first so the
// reference's own UnifiedConfig / UnifiedDataset (Eigen) are used.
#pragma once

#include "../lbfgs_amd.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

/// @brief Backend tag for the MI355X (HIP) implementation.
struct HipBackend {};

template <typename Backend> class IterationRecorder;
template <typename Backend> class NetworkWrapper;
template <typename Backend> class UnifiedOptimizer;
template <typename Backend> class UnifiedLauncher;

namespace hip_mlp {

using HipScalar = float; // fp32 like CudaScalar (src/cuda/common.cuh:11)

/// Abort with a message on any engine error, like cuda_check (src/cuda/common.cuh:18-23).
inline void hip_check(int rc, const char *msg) {
  if (rc != LBF_OK) {
    std::cerr << "HIP engine error: " << msg << " -> " << lbf_last_error() << std::endl;
    std::abort();
  }
}

/// Activation tags (the reference uses cpu_mlp::{Linear,ReLU,Sigmoid,Tanh}, src/layer.hpp:16-47).
struct Linear { static constexpr int id = LBF_ACT_LINEAR; };
struct Tanh { static constexpr int id = LBF_ACT_TANH; };
struct ReLU { static constexpr int id = LBF_ACT_RELU; };
struct Sigmoid { static constexpr int id = LBF_ACT_SIGMOID; };
/// Rectifiers with curvature (an extension; formulas and fixed constants: lbf_mlp_create in lbfgs_amd.h).
struct LeakyReLU { static constexpr int id = LBF_ACT_LEAKY_RELU; };
struct ELU { static constexpr int id = LBF_ACT_ELU; };
struct Softplus { static constexpr int id = LBF_ACT_SOFTPLUS; };

/// The loss the network's evaluations and every solver on it minimise (lbf_mlp_set_loss; an extension: the
/// reference has the squared error only). SoftmaxCrossEntropy takes the outputs of a Linear last layer as logits.
enum class Loss : int { MeanSquaredError = LBF_LOSS_MSE, SoftmaxCrossEntropy = LBF_LOSS_SOFTMAX_XENT };

/// Maps an activation tag type to the engine's id; specialise for other tag types.
template <typename T> struct ActivationId { static constexpr int value = T::id; };

/// Owns the device context (stream, optional RCCL communicator): CublasHandle analogue.
class HipHandle {
public:
  explicit HipHandle(int device = 0) { hip_check(lbf_ctx_create(device, nullptr, &h_), "lbf_ctx_create"); }
  ~HipHandle() { lbf_ctx_destroy(h_); }
  HipHandle(const HipHandle &) = delete;
  HipHandle &operator=(const HipHandle &) = delete;
  lbf_ctx *get() const { return h_; }
  void sync() const { hip_check(lbf_ctx_sync(h_), "lbf_ctx_sync"); }
  /// Data parallelism: call on every rank with the id from rank 0's unique_id().
  static std::vector<char> unique_id() {
    std::vector<char> id(128);
    hip_check(lbf_comm_unique_id(id.data()), "lbf_comm_unique_id");
    return id;
  }
  void comm_init(int nranks, int rank, const std::vector<char> &id) {
    hip_check(lbf_comm_init(h_, nranks, rank, id.data()), "lbf_comm_init");
  }

private:
  lbf_ctx *h_ = nullptr;
};

/// RAII device buffer (src/cuda/device_buffer.cuh:7-96).
template <typename T> class DeviceBuffer {
public:
  explicit DeviceBuffer(HipHandle &h, size_t n = 0) : h_(&h) { resize(n); }
  ~DeviceBuffer() { release(); }
  DeviceBuffer(const DeviceBuffer &) = delete;
  DeviceBuffer &operator=(const DeviceBuffer &) = delete;
  void resize(size_t n) {
    if (n == n_) return;
    release();
    if (n) {
      void *p = nullptr;
      hip_check(lbf_device_alloc(h_->get(), n * sizeof(T), &p), "lbf_device_alloc");
      p_ = static_cast<T *>(p);
    }
    n_ = n;
  }
  T *data() { return p_; }
  const T *data() const { return p_; }
  size_t size() const { return n_; }
  void copy_from_host(const T *src, size_t n) {
    hip_check(lbf_memcpy(h_->get(), p_, src, n * sizeof(T), 0), "copy_from_host");
  }
  void copy_to_host(T *dst, size_t n) const {
    hip_check(lbf_memcpy(h_->get(), dst, p_, n * sizeof(T), 1), "copy_to_host");
  }

private:
  void release() {
    if (p_) lbf_device_free(h_->get(), p_);
    p_ = nullptr;
    n_ = 0;
  }
  HipHandle *h_;
  T *p_ = nullptr;
  size_t n_ = 0;
};

/// What HipNetwork::evaluate returns (lbf_eval_result): the data loss with inv_scale = 1 / rows, and the counts.
struct EvalResult {
  double loss = 0.0;
  long long rows = 0, correct = 0, topk = 0;
  int k = 1;
  double accuracy() const { return rows > 0 ? double(correct) / double(rows) : 0.0; } ///< in [0, 1]
  double topk_accuracy() const { return rows > 0 ? double(topk) / double(rows) : 0.0; }
};

/// Dense MLP on the device (CudaNetwork, src/cuda/network.cuh:21-158).
class HipNetwork {
public:
  explicit HipNetwork(HipHandle &h) : h_(h), params_(h), grads_(h) {}
  ~HipNetwork() {
    if (net_) lbf_mlp_destroy(net_);
  }
  void addLayer(int in, int out, int act) {
    if (dims_.empty()) dims_.push_back(in);
    dims_.push_back(out);
    acts_.push_back(act);
  }
  /// init_mode LBF_INIT_CUDA reproduces network.cuh:36-59; LBF_INIT_CPU reproduces network.hpp:45-71.
  void bindParams(unsigned seed = 123, int init_mode = LBF_INIT_CUDA) {
    if (!net_) {
      hip_check(lbf_mlp_create(h_.get(), int(acts_.size()), dims_.data(), acts_.data(), &net_), "lbf_mlp_create");
      params_.resize(size_t(lbf_mlp_param_count(net_)));
      grads_.resize(params_.size());
      if (loss_ != Loss::MeanSquaredError) hip_check(lbf_mlp_set_loss(net_, int(loss_)), "lbf_mlp_set_loss");
      if (l2_ != 0.0) hip_check(lbf_mlp_set_l2(net_, l2_), "lbf_mlp_set_l2");
    }
    hip_check(lbf_mlp_init_params(net_, seed, init_mode, params_.data()), "lbf_mlp_init_params");
  }
  /// Before or after bindParams(); not between a stateful solver's begin and end. An invalid choice (a
  /// non-linear last layer, fewer than two outputs) aborts like any engine error.
  void setLoss(Loss loss) {
    if (net_) hip_check(lbf_mlp_set_loss(net_, int(loss)), "lbf_mlp_set_loss");
    loss_ = loss;
  }
  Loss loss() const { return loss_; }
  /// L2 weight decay of the full-batch L-BFGS, GD and SGD solvers on this network (lbf_mlp_set_l2): they minimise
  /// data loss + 0.5 l2 |w|^2 and report it. Before or after bindParams(); not between a stateful solver's begin
  /// and end. compute_loss_and_grad, forward_only and the launcher's evaluate() keep the data term only. A
  /// negative or non-finite value aborts like any engine error.
  void setL2(double l2) {
    if (net_) hip_check(lbf_mlp_set_l2(net_, l2), "lbf_mlp_set_l2");
    else if (!(l2 >= 0.0) || l2 > 1.7976931348623157e308) hip_check(LBF_ERR_INVALID, "lbf_mlp_set_l2");
    l2_ = l2;
  }
  double l2() const { return l2_; }
  size_t params_size() const { return params_.size(); }
  int output_size() const { return dims_.empty() ? 0 : dims_.back(); }
  HipScalar *params_data() { return params_.data(); }
  HipScalar *grads_data() { return grads_.data(); }
  void forward_only(const HipScalar *input, int batch, HipScalar *out) {
    hip_check(lbf_mlp_forward(net_, params_.data(), input, batch, out), "lbf_mlp_forward");
  }
  /// Mean loss (MSE, or the cross-entropy after setLoss) and gradient into grads_data() (network.cuh:97-119).
  HipScalar compute_loss_and_grad(const HipScalar *input, const HipScalar *target, int batch) {
    double loss = 0.0;
    hip_check(lbf_mlp_loss_grad(net_, params_.data(), grads_.data(), input, target, nullptr, batch, 1.0 / batch, 0.0,
                                &loss),
              "lbf_mlp_loss_grad");
    return HipScalar(loss);
  }
  /// Device-side evaluation (lbf_mlp_evaluate; replaces the host scan of unified_launcher.hpp:154-199): loss,
  /// correct and top-k counts of `batch` rows; d_y null: predictions only. confusion (nullable): resized to
  /// Out x Out, [target * Out + predicted]. d_pred (nullable): batch ints on the device. The argmax and top-k
  /// rules are stated in lbfgs_amd.h. With a communicator `batch` is this rank's share and the result the total.
  EvalResult evaluate(const HipScalar *d_x, const HipScalar *d_y, long long batch, int k = 1,
                      std::vector<long long> *confusion = nullptr, int *d_pred = nullptr) {
    lbf_eval_result r{};
    const size_t out = size_t(output_size());
    if (confusion) confusion->assign(out * out, 0);
    hip_check(lbf_mlp_evaluate(net_, params_.data(), d_x, d_y, nullptr, batch, 1.0, k, 0, &r,
                               confusion ? confusion->data() : nullptr, d_pred, nullptr),
              "lbf_mlp_evaluate");
    EvalResult e;
    e.rows = r.rows;
    e.correct = r.correct;
    e.topk = r.topk;
    e.k = r.k;
    e.loss = r.rows > 0 ? r.loss * (1.0 / double(r.rows)) : 0.0; // linear in inv_scale: 1 / total rows
    return e;
  }
  /// d_out[i] = scale * sum_b (d l_b / d w_i)^2 over `batch` rows (lbf_mlp_grad_sq): the sum of the squared
  /// per-example gradients of the data loss, the diagonal of the empirical Fisher matrix, in the flat parameter
  /// layout (parameter count floats on the device). No l2 term. Overwrites the activation workspace.
  void gradSq(const HipScalar *d_x, const HipScalar *d_y, long long batch, double scale, HipScalar *d_out) {
    hip_check(lbf_mlp_grad_sq(net_, params_.data(), d_x, d_y, nullptr, batch, scale, d_out), "lbf_mlp_grad_sq");
  }
  lbf_mlp *raw() const { return net_; }
  HipHandle &handle() { return h_; }
  const std::vector<int> &dims() const { return dims_; }

private:
  HipHandle &h_;
  lbf_mlp *net_ = nullptr;
  std::vector<int> dims_, acts_;
  Loss loss_ = Loss::MeanSquaredError;
  double l2_ = 0.0;
  DeviceBuffer<HipScalar> params_, grads_;
};

} // namespace hip_mlp

/// Host-side history of (loss, ||g||, cumulative ms) per iteration (iteration_recorder.hpp:13-146;
/// the device records in bulk instead of three H2D copies per iteration).
template <> class IterationRecorder<HipBackend> {
public:
  void init(int capacity) {
    if (capacity <= 0) return;
    capacity_ = capacity;
    loss_.assign(size_t(capacity), 0.0);
    grad_norm_.assign(size_t(capacity), 0.0);
    time_ms_.assign(size_t(capacity), 0.0);
    size_ = 0;
  }
  void reset() { size_ = 0; }
  void record(int idx, double loss, double grad_norm, double time_ms = 0.0) {
    if (idx < 0 || idx >= capacity_) return;
    loss_[size_t(idx)] = loss;
    grad_norm_[size_t(idx)] = grad_norm;
    time_ms_[size_t(idx)] = time_ms;
    size_ = std::max(size_, idx + 1);
  }
  void copy_to_host(std::vector<double> &l, std::vector<double> &g) const {
    l.assign(loss_.begin(), loss_.begin() + size_);
    g.assign(grad_norm_.begin(), grad_norm_.begin() + size_);
  }
  void copy_to_host(std::vector<double> &l, std::vector<double> &g, std::vector<double> &t) const {
    copy_to_host(l, g);
    t.assign(time_ms_.begin(), time_ms_.begin() + size_);
  }
  int size() const { return size_; }
  // the engine writes its record here (lbf_record views the recorder's arrays)
  lbf_record view() {
    lbf_record r{};
    r.loss = loss_.data();
    r.grad_norm = grad_norm_.data();
    r.time_ms = time_ms_.data();
    r.cap = capacity_;
    r.size = 0;
    return r;
  }
  void set_size(int s) { size_ = s; }

private:
  std::vector<double> loss_, grad_norm_, time_ms_;
  int capacity_ = 0, size_ = 0;
};

namespace hip_mlp {

/// Abstract minimizer (CudaMinimizerBase, src/cuda/minimizer_base.cuh:12-67).
class HipMinimizerBase {
public:
  using LossGradFun = std::function<HipScalar(const HipScalar *params, HipScalar *grad, const HipScalar *input,
                                              const HipScalar *target, int batch)>;
  using IterHook = std::function<void(int)>;
  explicit HipMinimizerBase(HipHandle &handle) : handle_(handle) {}
  virtual ~HipMinimizerBase() = default;
  int iterations() const noexcept { return last_iterations_; }
  void setRecorder(::IterationRecorder<HipBackend> *recorder) { recorder_ = recorder; }
  void setMaxIterations(int iters) { max_iters_ = iters; }
  void setTolerance(HipScalar tol) { tol_ = tol; }
  void setLineSearchParams(int max_iters, HipScalar c1, HipScalar rho) {
    max_line_iters_ = (max_iters < 1) ? 1 : max_iters;
    c1_ = c1;
    rho_ = rho;
  }
  virtual void solve(int n, HipScalar *params, const HipScalar *input, const HipScalar *target, int batch,
                     const LossGradFun &loss_grad) = 0;

protected:
  /// What every solve() shares. Nothing to solve (lbfgs.cuh:45-48): zero iterations and no engine call. Otherwise
  /// call(rec, info) runs the entry point, rec being the recorder's arrays (null without a recorder).
  template <class Call> void run(int n, const HipScalar *params, const char *what, Call &&call) {
    last_iterations_ = 0;
    if (n <= 0 || params == nullptr) return;
    lbf_record rec{};
    if (recorder_) {
      recorder_->reset();
      rec = recorder_->view();
    }
    lbf_solve_info info{};
    hip_check(call(recorder_ ? &rec : nullptr, &info), what);
    if (recorder_) recorder_->set_size(rec.size);
    last_iterations_ = info.iterations;
  }

  HipHandle &handle_;
  int max_iters_ = 200, max_line_iters_ = 20;
  HipScalar tol_ = 1e-6f, c1_ = 1e-4f, rho_ = 0.5f;
  int last_iterations_ = 0;
  ::IterationRecorder<HipBackend> *recorder_ = nullptr;
};

/// L-BFGS with the reference's CUDA semantics by default (Armijo + interpolation, lbfgs.cuh:39-194);
/// setLineSearch(LBF_LS_WOLFE) selects the CPU semantics (lbfgs.hpp:38-100). Any LossGradFun works:
/// the engine keeps the (s, y) history, two-loop and line search on the device.
class HipLBFGS : public HipMinimizerBase {
public:
  explicit HipLBFGS(HipHandle &handle) : HipMinimizerBase(handle) {}
  void setMemory(size_t m) { m_ = m; }
  void setLineSearch(int ls) { ls_ = ls; }

  void solve(int n, HipScalar *params, const HipScalar *input, const HipScalar *target, int batch,
             const LossGradFun &loss_grad) override {
    struct Closure {
      const LossGradFun *f;
      const HipScalar *in, *tg;
      int batch;
    } cl{&loss_grad, input, target, batch};
    auto tramp = [](void *u, const float *p, float *g) -> double {
      auto *c = static_cast<Closure *>(u);
      return double((*c->f)(p, g, c->in, c->tg, c->batch));
    };
    lbf_lbfgs_params prm;
    lbf_lbfgs_default_params(&prm, ls_);
    prm.m = int(m_);
    prm.max_iters = max_iters_;
    prm.tol = tol_;
    if (ls_ == LBF_LS_ARMIJO) {
      prm.max_line_iters = max_line_iters_;
      prm.c1 = c1_;
      prm.rho = rho_;
    }
    run(n, params, "lbf_lbfgs_solve_fn", [&](lbf_record *rec, lbf_solve_info *info) {
      return lbf_lbfgs_solve_fn(handle_.get(), &prm, n, params, tramp, &cl, rec, info);
    });
  }

private:
  size_t m_ = 16; // lbfgs.cuh:264
  int ls_ = LBF_LS_ARMIJO;
};

/// What HipHF and HipHFPreconditioned share: the network, the setters and the lbf_hf_params they give.
class HipHFBase : public HipMinimizerBase {
public:
  void setCG(int iters, double rtol) {
    cg_iters_ = iters;
    cg_rtol_ = rtol;
  }
  void setDamping(double damping0) { damping0_ = damping0; }
  void setCurvatureRows(long long rows) { curv_rows_ = rows; }

protected:
  HipHFBase(HipHandle &handle, HipNetwork &net) : HipMinimizerBase(handle), net_(net) {}
  lbf_hf_params hfParams() const {
    lbf_hf_params prm;
    lbf_hf_default_params(&prm);
    prm.max_iters = max_iters_;
    prm.tol = tol_;
    prm.cg_iters = cg_iters_;
    prm.cg_rtol = cg_rtol_;
    prm.damping0 = damping0_;
    prm.curv_rows = curv_rows_;
    prm.max_line_iters = max_line_iters_;
    prm.c1 = c1_;
    prm.rho = rho_;
    return prm;
  }
  HipNetwork &net_;

private:
  int cg_iters_ = 50;
  double cg_rtol_ = 0.1, damping0_ = 1.0;
  long long curv_rows_ = 0;
};

/// Hessian-free (truncated Newton) minimizer on a HipNetwork (HIP extension, no reference counterpart:
/// lbf_hf_solve, Gauss-Newton CG steps with Levenberg-Marquardt damping). The curvature needs the network, not
/// only its loss and gradient, so solve() minimises the network's own loss (+ its l2) on input / target and does
/// not call loss_grad; n must be the network's parameter count.
class HipHF : public HipHFBase {
public:
  HipHF(HipHandle &handle, HipNetwork &net) : HipHFBase(handle, net) {}
  void solve(int n, HipScalar *params, const HipScalar *input, const HipScalar *target, int batch,
             const LossGradFun &) override {
    const lbf_hf_params prm = hfParams();
    run(n, params, "lbf_hf_solve", [&](lbf_record *rec, lbf_solve_info *info) {
      return lbf_hf_solve(net_.raw(), &prm, params, input, target, batch, batch, rec, info);
    });
  }
};

/// HipHF with the CG preconditioned by the squared-gradient diagonal (lbf_hf_solve_pc, LBF_PRECOND_GRAD_SQ):
/// M = (D / rows + l2 + damping)^exponent, D = HipNetwork::gradSq of the curvature rows. A class of its own, so that
/// a program using HipHF alone links against a library that predates lbf_hf_solve_pc.
class HipHFPreconditioned : public HipHFBase {
public:
  HipHFPreconditioned(HipHandle &handle, HipNetwork &net) : HipHFBase(handle, net) {}
  /// exponent in [0, 1] (0: no preconditioning, the bits of HipHF); refresh: outer iterations between two
  /// evaluations of D
  void setPreconditioner(double exponent, int refresh = 1) { pc_ = gradSqPreconditioner(exponent, refresh); }
  /// the lbf_hf_precond of this class and of UnifiedHFPreconditioned_HIP
  static lbf_hf_precond gradSqPreconditioner(double exponent, int refresh) {
    lbf_hf_precond pc;
    lbf_hf_precond_default(&pc);
    pc.mode = LBF_PRECOND_GRAD_SQ;
    pc.exponent = exponent;
    pc.refresh = refresh;
    return pc;
  }

  void solve(int n, HipScalar *params, const HipScalar *input, const HipScalar *target, int batch,
             const LossGradFun &) override {
    const lbf_hf_params prm = hfParams();
    run(n, params, "lbf_hf_solve_pc", [&](lbf_record *rec, lbf_solve_info *info) {
      return lbf_hf_solve_pc(net_.raw(), &prm, &pc_, params, input, target, batch, batch, rec, info);
    });
  }

private:
  lbf_hf_precond pc_ = gradSqPreconditioner(0.75, 1);
};

/// OWL-QN minimizer on a HipNetwork (HIP extension, no reference counterpart: lbf_owlqn_solve, L-BFGS on the
/// network's loss + its l2 + l1 |w|_1 with the orthant-wise pseudo-gradient, direction and projection). Like HipHF,
/// solve() minimises the network's own objective on input / target and does not call loss_grad; n must be the
/// network's parameter count.
class HipOWLQN : public HipMinimizerBase {
public:
  HipOWLQN(HipHandle &handle, HipNetwork &net) : HipMinimizerBase(handle), net_(net) {}
  void setL1(double l1, bool on_biases = false) {
    l1_ = l1;
    l1_bias_ = on_biases ? 1 : 0;
  }
  void setHistorySize(int m) { m_ = m; }
  /// of the last solve's final point: zero and penalised coordinates, l1 |w|_1, the pseudo-gradient norm
  const lbf_owlqn_stats &stats() const { return stats_; }

  void solve(int n, HipScalar *params, const HipScalar *input, const HipScalar *target, int batch,
             const LossGradFun &) override {
    lbf_owlqn_params prm;
    lbf_owlqn_default_params(&prm);
    prm.m = m_;
    prm.max_iters = max_iters_;
    prm.tol = tol_;
    prm.l1 = l1_;
    prm.l1_bias = l1_bias_;
    prm.max_line_iters = max_line_iters_;
    prm.c1 = c1_;
    prm.rho = rho_;
    run(n, params, "lbf_owlqn_solve", [&](lbf_record *rec, lbf_solve_info *info) {
      return lbf_owlqn_solve(net_.raw(), &prm, params, input, target, batch, batch, rec, info, &stats_);
    });
  }

private:
  HipNetwork &net_;
  double l1_ = 0.0;
  int l1_bias_ = 0, m_ = 10;
  lbf_owlqn_stats stats_{};
};

/// Adam's loss trace, for HipAdam and UnifiedAdam_HIP: one entry per step, ceil(rows / batch) steps in each of
/// prm.max_epochs epochs, NaN until the step has run. Sizes `trace` and points prm at it (no steps: a null pointer).
inline void adam_trace_attach(std::vector<double> &trace, lbf_adam_params &prm, long long rows) {
  const long long per_epoch = prm.batch > 0 ? (rows + prm.batch - 1) / prm.batch : 0;
  trace.assign(size_t(std::max(0LL, per_epoch * std::max(0, prm.max_epochs))), std::nan(""));
  prm.loss_trace = trace.empty() ? nullptr : trace.data();
  prm.trace_cap = int(trace.size());
}
/// After the solve: drops the steps that did not run.
inline void adam_trace_trim(std::vector<double> &trace) {
  while (!trace.empty() && std::isnan(trace.back())) trace.pop_back();
}

/// Adam / AdamW minimizer on a HipNetwork (HIP extension, no reference counterpart: lbf_adam_solve, shuffled
/// minibatches, one fused evaluation and one device-side sweep per step). Like HipHF, solve() minimises the
/// network's own loss (+ its l2) and does not call loss_grad; n must be the network's parameter count, `batch` is the
/// number of rows N of input / target, setMaxIterations counts epochs and setTolerance is the relative epoch-loss
/// test of CudaSGD. With a recorder: the start point's full-batch row and one per epoch.
class HipAdam : public HipMinimizerBase {
public:
  HipAdam(HipHandle &handle, HipNetwork &net) : HipMinimizerBase(handle), net_(net) { lbf_adam_default_params(&prm_); }
  void setLearningRate(double lr) { prm_.lr = lr; }
  void setBetas(double beta1, double beta2) {
    prm_.beta1 = beta1;
    prm_.beta2 = beta2;
  }
  void setEpsilon(double eps) { prm_.eps = eps; }
  void setWeightDecay(double wd) { prm_.weight_decay = wd; } ///< AdamW's decoupled decay
  void setClipNorm(double c) { prm_.clip_norm = c; }
  void setBatchSize(int b) { prm_.batch = b; }
  void setShuffle(bool on, unsigned seed = 123u) {
    prm_.shuffle = on ? 1 : 0;
    prm_.seed = seed;
  }
  void setLearningRateDecay(double rate, int step) {
    prm_.decay_rate = rate;
    prm_.decay_step = step;
  }
  /// the batch objective of every step of the last solve, evaluated before the step
  const std::vector<double> &lossTrace() const { return trace_; }

  void solve(int n, HipScalar *params, const HipScalar *input, const HipScalar *target, int batch,
             const LossGradFun &) override {
    run(n, params, "lbf_adam_solve", [&](lbf_record *rec, lbf_solve_info *info) {
      lbf_adam_params prm = prm_;
      prm.max_epochs = max_iters_;
      prm.tol = tol_;
      adam_trace_attach(trace_, prm, batch);
      return lbf_adam_solve(net_.raw(), &prm, params, input, target, batch, rec, info);
    });
    adam_trace_trim(trace_);
  }

private:
  HipNetwork &net_;
  lbf_adam_params prm_{};
  std::vector<double> trace_;
};

/// The curvature spectrum of a HipNetwork at its current parameters (HIP extension, no reference counterpart:
/// lbf_mlp_lanczos and lbf_tridiag_eig): k steps of device-side Lanczos on the Gauss-Newton matrix or the exact Hessian
/// of the mean loss over `batch` rows, plus l2 I. A class of its own, so that a program using the other classes alone
/// links against a library that predates these entry points.
class HipSpectrum {
public:
  HipSpectrum(HipHandle &, HipNetwork &net) : net_(net) { lbf_lanczos_default_params(&prm_); }
  void setSteps(int steps) { prm_.steps = steps; }
  /// LBF_HVP_GAUSS_NEWTON (default) or LBF_HVP_EXACT
  void setMatrix(int matrix) { prm_.matrix = matrix; }
  /// full re-orthogonalisation (default) or the three-vector recurrence
  void setReorthogonalize(bool on) { prm_.reorth = on ? 1 : 0; }
  void setL2(double l2) { prm_.l2 = l2; }
  void setCheck(int check) { prm_.check = check; }
  void setBreakdownTolerance(double rtol) { prm_.breakdown_rtol = rtol; }
  /// Runs from the start vector d_v0 (parameter count floats on the device). d_basis (nullable): steps + 1 rows at
  /// stride ld floats receive the Lanczos vectors. Returns the status: 0 all steps ran, 1 the Krylov space was
  /// exhausted after steps() steps, 2 a non-finite product or start vector.
  int lanczos(const HipScalar *d_v0, const HipScalar *input, const HipScalar *target, long long batch,
              HipScalar *d_basis = nullptr, long long ld = 0) {
    alpha_.assign(size_t(prm_.steps > 0 ? prm_.steps : 1), 0.0);
    beta_.assign(alpha_.size(), 0.0);
    hip_check(lbf_mlp_lanczos(net_.raw(), net_.params_data(), d_v0, input, target, nullptr, batch,
                              1.0 / double(batch > 0 ? batch : 1), &prm_, alpha_.data(), beta_.data(), d_basis, ld,
                              &info_),
              "lbf_mlp_lanczos");
    return info_.status;
  }
  int steps() const { return info_.steps; }
  int status() const { return info_.status; }
  const std::vector<double> &alpha() const { return alpha_; } ///< steps() entries count, zeros behind them
  const std::vector<double> &beta() const { return beta_; }
  /// The Ritz values of the last run, ascending; weights (nullable): the squared first components of the
  /// tridiagonal's eigenvectors, the quadrature weights of the start vector's spectral measure.
  std::vector<double> ritz(std::vector<double> *weights = nullptr) const {
    std::vector<double> theta(size_t(info_.steps));
    if (weights) weights->assign(theta.size(), 0.0);
    if (!theta.empty())
      hip_check(lbf_tridiag_eig(info_.steps, alpha_.data(), beta_.data(), theta.data(),
                                weights ? weights->data() : nullptr, nullptr),
                "lbf_tridiag_eig");
    return theta;
  }

private:
  HipNetwork &net_;
  lbf_lanczos_params prm_{};
  lbf_lanczos_info info_{};
  std::vector<double> alpha_, beta_;
};

/// Column-major host matrix with the subset of Eigen::MatrixXd's interface the launcher uses.
class HostMatrix {
public:
  HostMatrix() = default;
  HostMatrix(long rows, long cols) : r_(rows), c_(cols), d_(size_t(rows * cols), 0.0) {}
  long rows() const { return r_; }
  long cols() const { return c_; }
  long size() const { return r_ * c_; }
  double *data() { return d_.data(); }
  const double *data() const { return d_.data(); }
  double &operator()(long i, long j) { return d_[size_t(i + j * r_)]; }
  double operator()(long i, long j) const { return d_[size_t(i + j * r_)]; }

private:
  long r_ = 0, c_ = 0;
  std::vector<double> d_;
};

/// The reference's MNISTLoader (tests/mnist/mnist_loader.hpp:8-100) over lbf_idx_read_*: images as a
/// (rows*cols) x N matrix scaled to [0, 1], labels one-hot 10 x N, column-major like the Eigen version.
struct MNISTLoader {
  static HostMatrix loadImages(const std::string &path, int max_images = 0) {
    long long n = 0;
    int r = 0, c = 0;
    hip_check(lbf_idx_read_images(path.c_str(), max_images, nullptr, &n, &r, &c), "lbf_idx_read_images");
    std::vector<float> buf(size_t(n) * size_t(r) * size_t(c));
    hip_check(lbf_idx_read_images(path.c_str(), max_images, buf.data(), &n, &r, &c), "lbf_idx_read_images");
    HostMatrix m(long(r) * c, long(n));
    for (size_t i = 0; i < buf.size(); ++i) m.data()[i] = double(buf[i]);
    return m;
  }
  static HostMatrix loadLabels(const std::string &path, int max_images = 0) {
    long long n = 0;
    hip_check(lbf_idx_read_labels(path.c_str(), max_images, 10, nullptr, &n), "lbf_idx_read_labels");
    std::vector<float> buf(size_t(n) * 10);
    hip_check(lbf_idx_read_labels(path.c_str(), max_images, 10, buf.data(), &n), "lbf_idx_read_labels");
    HostMatrix m(10, long(n));
    for (size_t i = 0; i < buf.size(); ++i) m.data()[i] = double(buf[i]);
    return m;
  }
};

} // namespace hip_mlp

#ifndef LBF_USE_REFERENCE_UNIFIED_TYPES
/// src/unified_optimization.hpp:26-48
struct UnifiedConfig {
  std::string name = "Experiment";
  int max_iters = 100;
  double tolerance = 1e-4;
  double learning_rate = 0.01;
  double momentum = 0.0;
  double lr_decay = 0.0;
  int lr_decay_rate = 1;
  int batch_size = 128;
  int m_param = 10;
  int L_param = 10;
  int b_H_param = 0;
  int log_interval = 10;
  bool reset_params = true;
  unsigned int seed = 123u;
  double l2 = 0.0; ///< HIP extension: train() applies a non-zero value like UnifiedLauncher::setL2
  /// HIP extension: UnifiedSLBFGS_HIP's curvature pairs, LBF_HVP_FD (the reference's finite difference),
  /// LBF_HVP_EXACT or LBF_HVP_GAUSS_NEWTON (lbf_slbfgs_params.hvp_exact)
  int curvature = LBF_HVP_FD;
  /// HIP extension: UnifiedHF_HIP's CG iterations and relative residual per step and its initial damping
  int cg_iters = 50;
  double cg_rtol = 0.1;
  double damping = 1.0;
  double l1 = 0.0; ///< HIP extension: UnifiedOWLQN_HIP's L1 penalty on the weights; the other optimisers do not read it
  /// HIP extension: UnifiedAdam_HIP (it also reads learning_rate, batch_size, max_iters as epochs, seed, and
  /// lr_decay / lr_decay_rate when lr_decay > 0). weight_decay is AdamW's decoupled decay, clip_norm the global norm
  /// each batch gradient is clipped to (0: off)
  double beta1 = 0.9, beta2 = 0.999, adam_eps = 1e-8, weight_decay = 0.0, clip_norm = 0.0;
  bool shuffle = true;
};
/// src/unified_optimization.hpp:54-59 (HostMatrix instead of Eigen::MatrixXd)
struct UnifiedDataset {
  hip_mlp::HostMatrix train_x, train_y, test_x, test_y;
};
#endif

/// NetworkWrapper<HipBackend> (src/network_wrapper.hpp:92-110).
template <> class NetworkWrapper<HipBackend> {
public:
  using InternalNetwork = hip_mlp::HipNetwork;
  explicit NetworkWrapper(hip_mlp::HipHandle &handle) : network_(handle) {}
  template <int In, int Out, typename Activation> void addLayer() {
    network_.addLayer(In, Out, hip_mlp::ActivationId<Activation>::value);
  }
  void bindParams() { network_.bindParams(); }
  void bindParams(unsigned int seed, int init_mode = LBF_INIT_CUDA) { network_.bindParams(seed, init_mode); }
  InternalNetwork &getInternal() { return network_; }
  const InternalNetwork &getInternal() const { return network_; }
  size_t getParamsSize() const { return network_.params_size(); }

private:
  InternalNetwork network_;
};

inline std::string hip_log_filename(const UnifiedConfig &config) {
  return (config.name.empty() ? std::string("run") : config.name) + "_history.csv";
}

/// CSV schema Iteration,Loss,GradNorm,TimeMs (unified_optimization.hpp:446-465).
inline void write_hip_history_csv(const std::string &filename, const IterationRecorder<HipBackend> &recorder,
                                  int log_interval) {
  if (log_interval <= 0) return;
  std::vector<double> l, g, t;
  recorder.copy_to_host(l, g, t);
  if (l.empty()) return;
  std::ofstream f(filename);
  if (!f.is_open()) return;
  f << "Iteration,Loss,GradNorm,TimeMs\n";
  for (size_t i = 0; i < l.size(); i += size_t(std::max(1, log_interval)))
    f << i << "," << l[i] << "," << g[i] << "," << t[i] << "\n";
}

/// UnifiedOptimizer<HipBackend> (unified_optimization.hpp:420-439): the reference strategy's parameter list,
/// (handle, net, host_data, d_train_x, d_train_y, config), so a strategy written against
/// UnifiedOptimizer<CudaBackend>::optimize overrides this one with its backend types renamed. host_data is the
/// host dataset (for dimensions: n_train = host_data.train_x.cols()); the device data are fp32 rows of In / Out
/// floats per sample (== the reference's column-major matrices).
template <> class UnifiedOptimizer<HipBackend> {
public:
  virtual ~UnifiedOptimizer() = default;
  virtual void optimize(hip_mlp::HipHandle &handle, NetworkWrapper<HipBackend> &net, const UnifiedDataset &host_data,
                        hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &d_train_x,
                        hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &d_train_y, const UnifiedConfig &config) = 0;
  IterationRecorder<HipBackend> recorder;
  int line_search = LBF_LS_ARMIJO; // UnifiedLBFGS_CUDA's semantics unless set to LBF_LS_WOLFE

protected:
  /// What every optimize() shares: a record of `cap` rows, call(network, n_train, rec, info) runs the entry point,
  /// then the recorder's size and the history CSV.
  template <class Call>
  void run(NetworkWrapper<HipBackend> &net, const UnifiedDataset &host_data, const UnifiedConfig &c, int cap,
           const char *what, Call &&call) {
    recorder.init(cap);
    lbf_record rec = recorder.view();
    lbf_solve_info info{};
    hip_mlp::hip_check(call(net.getInternal(), long(host_data.train_x.cols()), &rec, &info), what);
    recorder.set_size(rec.size);
    write_hip_history_csv(hip_log_filename(c), recorder, c.log_interval);
  }
};

/// lbf_hf_params of UnifiedHF_HIP and UnifiedHFPreconditioned_HIP: the config's max_iters and tolerance and, where
/// the config is this header's own, its cg_iters, cg_rtol and damping.
inline lbf_hf_params hip_hf_params(const UnifiedConfig &c) {
  lbf_hf_params prm;
  lbf_hf_default_params(&prm);
  prm.max_iters = c.max_iters;
  prm.tol = c.tolerance;
#ifndef LBF_USE_REFERENCE_UNIFIED_TYPES // the reference's own UnifiedConfig has no such members
  prm.cg_iters = c.cg_iters;
  prm.cg_rtol = c.cg_rtol;
  prm.damping0 = c.damping;
#endif
  return prm;
}

/// UnifiedLBFGS_CUDA counterpart (unified_optimization.hpp:560-592): full-batch L-BFGS of the MLP,
/// all on the device (no per-evaluation callback or D2D gradient copy, cf. :483-491).
class UnifiedLBFGS_HIP : public UnifiedOptimizer<HipBackend> {
public:
  void optimize(hip_mlp::HipHandle &, NetworkWrapper<HipBackend> &net, const UnifiedDataset &host_data,
                hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dx, hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dy,
                const UnifiedConfig &c) override {
    lbf_lbfgs_params prm;
    lbf_lbfgs_default_params(&prm, line_search);
    prm.m = c.m_param > 0 ? c.m_param : 10;
    prm.max_iters = c.max_iters;
    prm.tol = c.tolerance;
    run(net, host_data, c, c.max_iters, "lbf_lbfgs_solve",
        [&](hip_mlp::HipNetwork &nw, long n, lbf_record *rec, lbf_solve_info *info) {
          return lbf_lbfgs_solve(nw.raw(), &prm, nw.params_data(), dx.data(), dy.data(), n, n, rec, info);
        });
  }
};

/// S-LBFGS on the device (the reference's is CPU-only: unified_optimization.hpp:306-408, 688-696).
class UnifiedSLBFGS_HIP : public UnifiedOptimizer<HipBackend> {
public:
  void optimize(hip_mlp::HipHandle &, NetworkWrapper<HipBackend> &net, const UnifiedDataset &host_data,
                hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dx, hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dy,
                const UnifiedConfig &c) override {
    lbf_slbfgs_params prm;
    lbf_slbfgs_default_params(&prm);
    prm.max_epochs = c.max_iters;
    prm.tol = c.tolerance;
    prm.M = c.m_param;
    prm.L = c.L_param;
    prm.b = c.batch_size;
    prm.b_H = c.b_H_param > 0 ? c.b_H_param : c.batch_size / 2;
    prm.step = c.learning_rate;
#ifndef LBF_USE_REFERENCE_UNIFIED_TYPES // the reference's own UnifiedConfig has no such member
    prm.hvp_exact = c.curvature;
#endif
    run(net, host_data, c, c.max_iters, "lbf_slbfgs_solve",
        [&](hip_mlp::HipNetwork &nw, long n, lbf_record *rec, lbf_solve_info *info) {
          return lbf_slbfgs_solve(nw.raw(), &prm, nw.params_data(), dx.data(), dy.data(), n, rec, info);
        });
  }
};

/// UnifiedGD_CUDA counterpart (unified_optimization.hpp:518-554): CudaGD with lr, momentum,
/// max_iters, tolerance from the config (gd.cuh:38-106), on the device.
class UnifiedGD_HIP : public UnifiedOptimizer<HipBackend> {
public:
  void optimize(hip_mlp::HipHandle &, NetworkWrapper<HipBackend> &net, const UnifiedDataset &host_data,
                hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dx, hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dy,
                const UnifiedConfig &c) override {
    lbf_gd_params prm;
    lbf_gd_default_params(&prm);
    prm.lr = c.learning_rate;
    prm.momentum = c.momentum;
    prm.max_iters = c.max_iters;
    prm.tol = c.tolerance;
    run(net, host_data, c, c.max_iters, "lbf_gd_solve",
        [&](hip_mlp::HipNetwork &nw, long n, lbf_record *rec, lbf_solve_info *info) {
          return lbf_gd_solve(nw.raw(), &prm, nw.params_data(), dx.data(), dy.data(), n, n, rec, info);
        });
  }
};

/// Hessian-free training (HIP extension, no reference counterpart): lbf_hf_solve with hip_hf_params(config).
class UnifiedHF_HIP : public UnifiedOptimizer<HipBackend> {
public:
  void optimize(hip_mlp::HipHandle &, NetworkWrapper<HipBackend> &net, const UnifiedDataset &host_data,
                hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dx, hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dy,
                const UnifiedConfig &c) override {
    const lbf_hf_params prm = hip_hf_params(c);
    run(net, host_data, c, c.max_iters, "lbf_hf_solve",
        [&](hip_mlp::HipNetwork &nw, long n, lbf_record *rec, lbf_solve_info *info) {
          return lbf_hf_solve(nw.raw(), &prm, nw.params_data(), dx.data(), dy.data(), n, n, rec, info);
        });
  }
};

/// UnifiedHF_HIP with the CG preconditioned by the squared-gradient diagonal (lbf_hf_solve_pc); the exponent and the
/// refresh interval are the optimizer's own (setPreconditioner), since the reference's UnifiedConfig has no place
/// for them. A class of its own for the reason given at HipHFPreconditioned.
class UnifiedHFPreconditioned_HIP : public UnifiedOptimizer<HipBackend> {
public:
  void setPreconditioner(double exponent, int refresh = 1) {
    pc_ = hip_mlp::HipHFPreconditioned::gradSqPreconditioner(exponent, refresh);
  }
  void optimize(hip_mlp::HipHandle &, NetworkWrapper<HipBackend> &net, const UnifiedDataset &host_data,
                hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dx, hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dy,
                const UnifiedConfig &c) override {
    const lbf_hf_params prm = hip_hf_params(c);
    run(net, host_data, c, c.max_iters, "lbf_hf_solve_pc",
        [&](hip_mlp::HipNetwork &nw, long n, lbf_record *rec, lbf_solve_info *info) {
          return lbf_hf_solve_pc(nw.raw(), &prm, &pc_, nw.params_data(), dx.data(), dy.data(), n, n, rec, info);
        });
  }

private:
  lbf_hf_precond pc_ = hip_mlp::HipHFPreconditioned::gradSqPreconditioner(0.75, 1);
};

/// L1-regularised L-BFGS (HIP extension, no reference counterpart): lbf_owlqn_solve with the config's m_param,
/// max_iters and tolerance and, where the config is this header's own, its l1.
class UnifiedOWLQN_HIP : public UnifiedOptimizer<HipBackend> {
public:
  lbf_owlqn_stats stats{};
  void optimize(hip_mlp::HipHandle &, NetworkWrapper<HipBackend> &net, const UnifiedDataset &host_data,
                hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dx, hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dy,
                const UnifiedConfig &c) override {
    lbf_owlqn_params prm;
    lbf_owlqn_default_params(&prm);
    prm.m = c.m_param;
    prm.max_iters = c.max_iters;
    prm.tol = c.tolerance;
#ifndef LBF_USE_REFERENCE_UNIFIED_TYPES // the reference's own UnifiedConfig has no such member
    prm.l1 = c.l1;
#endif
    run(net, host_data, c, c.max_iters, "lbf_owlqn_solve",
        [&](hip_mlp::HipNetwork &nw, long n, lbf_record *rec, lbf_solve_info *info) {
          return lbf_owlqn_solve(nw.raw(), &prm, nw.params_data(), dx.data(), dy.data(), n, n, rec, info, &stats);
        });
  }
};

/// Adam / AdamW (HIP extension, no reference counterpart): lbf_adam_solve with the config's learning_rate,
/// batch_size, max_iters (epochs), seed and lr_decay / lr_decay_rate (only when lr_decay > 0) and, where the config is
/// this header's own, its beta1, beta2, adam_eps, weight_decay, clip_norm and shuffle. The tolerance is not passed,
/// as for UnifiedSGD_HIP. trace: the batch objective of every step.
class UnifiedAdam_HIP : public UnifiedOptimizer<HipBackend> {
public:
  std::vector<double> trace;
  void optimize(hip_mlp::HipHandle &, NetworkWrapper<HipBackend> &net, const UnifiedDataset &host_data,
                hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dx, hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dy,
                const UnifiedConfig &c) override {
    lbf_adam_params prm;
    lbf_adam_default_params(&prm);
    prm.lr = c.learning_rate;
    prm.batch = c.batch_size;
    prm.max_epochs = c.max_iters;
    prm.seed = c.seed;
    if (c.lr_decay > 0.0) {
      prm.decay_rate = c.lr_decay;
      prm.decay_step = c.lr_decay_rate;
    }
#ifndef LBF_USE_REFERENCE_UNIFIED_TYPES // the reference's own UnifiedConfig has no such members
    prm.beta1 = c.beta1;
    prm.beta2 = c.beta2;
    prm.eps = c.adam_eps;
    prm.weight_decay = c.weight_decay;
    prm.clip_norm = c.clip_norm;
    prm.shuffle = c.shuffle ? 1 : 0;
#endif
    run(net, host_data, c, c.max_iters + 1, "lbf_adam_solve",
        [&](hip_mlp::HipNetwork &nw, long n, lbf_record *rec, lbf_solve_info *info) {
          hip_mlp::adam_trace_attach(trace, prm, n);
          return lbf_adam_solve(nw.raw(), &prm, nw.params_data(), dx.data(), dy.data(), n, rec, info);
        });
    hip_mlp::adam_trace_trim(trace);
  }
};

/// UnifiedSGD_CUDA counterpart (unified_optimization.hpp:595-632): CudaSGD with the config's lr,
/// momentum, batch size, max_iters (epochs) and setLearningRateDecay(lr_decay, lr_decay_rate)
/// (sgd.cuh:50-153; the reference does not pass the tolerance, so CudaSGD keeps its 1e-6).
class UnifiedSGD_HIP : public UnifiedOptimizer<HipBackend> {
public:
  void optimize(hip_mlp::HipHandle &, NetworkWrapper<HipBackend> &net, const UnifiedDataset &host_data,
                hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dx, hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &dy,
                const UnifiedConfig &c) override {
    lbf_sgd_params prm;
    lbf_sgd_default_params(&prm);
    prm.lr = c.learning_rate;
    prm.momentum = c.momentum;
    prm.batch = c.batch_size;
    prm.max_epochs = c.max_iters;
    prm.decay_rate = c.lr_decay;
    prm.decay_step = c.lr_decay_rate;
    run(net, host_data, c, c.max_iters + 1, "lbf_sgd_solve",
        [&](hip_mlp::HipNetwork &nw, long n, lbf_record *rec, lbf_solve_info *info) {
          return lbf_sgd_solve(nw.raw(), &prm, nw.params_data(), dx.data(), dy.data(), n, rec, info);
        });
  }
};

/// UnifiedLauncher<HipBackend> (src/unified_launcher.hpp:83-205).
template <> class UnifiedLauncher<HipBackend> {
public:
  explicit UnifiedLauncher(int device = 0)
      : handle_(device), net_wrapper_(handle_), d_train_x_(handle_), d_train_y_(handle_), d_test_x_(handle_),
        d_test_y_(handle_) {}
  template <int In, int Out, typename Activation> void addLayer() { net_wrapper_.addLayer<In, Out, Activation>(); }
  void buildNetwork() { net_wrapper_.bindParams(); }
  /// The loss train() minimises and evaluate() reports (default: the reference's MSE). It lives on the network,
  /// not in UnifiedConfig, which in reference mode is the reference's own struct.
  void setLoss(hip_mlp::Loss loss) { net_wrapper_.getInternal().setLoss(loss); }
  /// L2 weight decay of UnifiedLBFGS / UnifiedGD / UnifiedSGD (HipNetwork::setL2); evaluate() reports the data term.
  void setL2(double l2) { net_wrapper_.getInternal().setL2(l2); }

  /// Host -> device upload with the fp64 -> fp32 conversion of unified_launcher.hpp:105-128; like the reference
  /// it keeps a copy of the dataset, which train() hands to the strategy as host_data.
  /// Works with the reference's Eigen-based UnifiedDataset and with the standalone HostMatrix one.
  void setData(const UnifiedDataset &data) {
    dataset_ = data;
    upload(dataset_.train_x, d_train_x_, train_x_);
    upload(dataset_.train_y, d_train_y_, train_y_);
    upload(dataset_.test_x, d_test_x_, test_x_);
    upload(dataset_.test_y, d_test_y_, test_y_);
    n_train_ = long(dataset_.train_x.cols());
    n_test_ = long(dataset_.test_x.cols());
    std::cout << "Data Uploaded to GPU. Train: " << n_train_ << " samples." << std::endl;
  }

  void train(UnifiedOptimizer<HipBackend> &optimizer, const UnifiedConfig &config) {
    std::cout << ">>> Running HIP Experiment: " << config.name << std::endl;
#ifndef LBF_USE_REFERENCE_UNIFIED_TYPES
    if (config.l2 != 0.0) setL2(config.l2);
#endif
    if (config.reset_params) net_wrapper_.bindParams(config.seed);
    optimizer.optimize(handle_, net_wrapper_, dataset_, d_train_x_, d_train_y_, config);
    last_train_ = evaluate(train_y_, d_train_x_, n_train_, "Training Results");
  }
  void test() { last_test_ = evaluate(test_y_, d_test_x_, n_test_, "Test Results"); }
  /// Device-side metrics of the training or the test split (HipNetwork::evaluate) against the fp32 targets that
  /// setData() uploaded once; prints nothing. evaluate() / train() / test() keep the reference's host scan.
  hip_mlp::EvalResult metrics(bool test_split, int k = 1, std::vector<long long> *confusion = nullptr) {
    auto &net = net_wrapper_.getInternal();
    const long n = test_split ? n_test_ : n_train_;
    if (n <= 0) return hip_mlp::EvalResult{};
    return net.evaluate((test_split ? d_test_x_ : d_train_x_).data(), (test_split ? d_test_y_ : d_train_y_).data(), n,
                        k, confusion);
  }
  NetworkWrapper<HipBackend> &getWrapper() { return net_wrapper_; }
  std::pair<double, double> lastTrain() const { return last_train_; }
  std::pair<double, double> lastTest() const { return last_test_; }

private:
  template <typename M>
  void upload(const M &mat, hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &buf, std::vector<double> &host) {
    const size_t n = size_t(mat.rows() * mat.cols());
    host.assign(mat.data(), mat.data() + n);
    std::vector<hip_mlp::HipScalar> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = hip_mlp::HipScalar(host[i]);
    buf.resize(n);
    if (n) buf.copy_from_host(tmp.data(), n);
    rows_.push_back(long(mat.rows()));
  }
  /// Accuracy + mean MSE (unified_launcher.hpp:154-199).
  std::pair<double, double> evaluate(const std::vector<double> &y, hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &d_x,
                                     long batch, const char *label) {
    auto &net = net_wrapper_.getInternal();
    const int out_dim = net.output_size();
    if (batch <= 0) return {0.0, 0.0};
    hip_mlp::DeviceBuffer<hip_mlp::HipScalar> d_out(handle_, size_t(batch) * out_dim);
    net.forward_only(d_x.data(), int(batch), d_out.data());
    std::vector<hip_mlp::HipScalar> out(size_t(batch) * out_dim);
    d_out.copy_to_host(out.data(), out.size());
    const bool xent = net.loss() == hip_mlp::Loss::SoftmaxCrossEntropy;
    double mse = 0.0; // with the cross-entropy loss: the mean cross-entropy per sample, under the same label
    long correct = 0;
    for (long i = 0; i < batch; ++i) {
      int pi = 0, ti = 0;
      double pm = -1e20, tm = -1e20;
      for (int r = 0; r < out_dim; ++r) {
        const size_t idx = size_t(r + i * out_dim);
        const double v = out[idx], t = y[idx];
        if (!xent) mse += (v - t) * (v - t);
        if (v > pm) { pm = v; pi = r; }
        if (t > tm) { tm = t; ti = r; }
      }
      if (xent) { // sum_o y (lse - z), lse from the row maximum pm
        double se = 0.0;
        for (int r = 0; r < out_dim; ++r) se += std::exp(double(out[size_t(r + i * out_dim)]) - pm);
        const double lse = pm + std::log(se);
        for (int r = 0; r < out_dim; ++r) mse += y[size_t(r + i * out_dim)] * (lse - out[size_t(r + i * out_dim)]);
      }
      if (pi == ti) ++correct;
    }
    mse /= xent ? double(batch) : double(batch * out_dim);
    const double acc = double(correct) / double(batch) * 100.0;
    std::cout << label << ": MSE=" << mse << ", Accuracy=" << acc << "%" << std::endl;
    return {mse, acc};
  }

  hip_mlp::HipHandle handle_;
  NetworkWrapper<HipBackend> net_wrapper_;
  UnifiedDataset dataset_;
  hip_mlp::DeviceBuffer<hip_mlp::HipScalar> d_train_x_, d_train_y_, d_test_x_, d_test_y_;
  std::vector<double> train_x_, train_y_, test_x_, test_y_;
  std::vector<long> rows_;
  long n_train_ = 0, n_test_ = 0;
  std::pair<double, double> last_train_{0, 0}, last_test_{0, 0};
};
