// Parity driver: every solver class of include/lbfgs_amd/hip_backend.hpp on two small problems, each result dumped
// as raw arrays so that tests/test_gpu_dropin_parity.py can repeat the case through the ctypes wrappers and compare
// bit for bit. It is also the worked example of the C++ calls main_hip.cpp does not make: the cross-entropy loss,
// l2, UnifiedHF_HIP / HipHF, UnifiedOWLQN_HIP / HipOWLQN and their stats, metrics() / HipNetwork::evaluate, and a
// LossGradFun that evaluates a HipNetwork at the trial point it is handed. Plain C++17, links liblbfgs_amd_abi3.so.
//   usage: parity_hip <dir>
// <dir> holds fp32 row-major p{1,2}_{X,Y}_{train,test}.f32 (one sample per row):
//   P1  [20, 16, 3]  tanh / linear, MSE,                   37 train / 19 test rows (387 parameters: n % 4 != 0)
//   P2  [64, 32, 10] relu / linear, softmax cross-entropy, 257 train / 63 test rows, one-hot targets
// Per case it writes <dir>/<case>.params.f32, .loss.f64, .gnorm.f64, .time.f64 (the recorder) and <case>.txt, one
// "key value" per line, floating values as %a. The values of every case are restated in the test.
#include "lbfgs_amd/hip_backend.hpp"

#include <cstdio>
#include <string>
#include <vector>

using Backend = HipBackend;
using hip_mlp::HipScalar;
using hip_mlp::HostMatrix;

namespace {

std::string g_dir;

struct P1 {
  static constexpr int In = 20, Hid = 16, Out = 3, NTrain = 37, NTest = 19;
  static constexpr const char *tag = "p1";
  using HidAct = hip_mlp::Tanh;
};
struct P2 {
  static constexpr int In = 64, Hid = 32, Out = 10, NTrain = 257, NTest = 63;
  static constexpr const char *tag = "p2";
  using HidAct = hip_mlp::ReLU;
};

std::vector<float> read_f32(const std::string &name, size_t count) {
  std::vector<float> v(count);
  const std::string path = g_dir + "/" + name;
  std::FILE *f = std::fopen(path.c_str(), "rb");
  if (!f || std::fread(v.data(), sizeof(float), count, f) != count) {
    std::cerr << "cannot read " << count << " floats from " << path << std::endl;
    std::exit(2);
  }
  std::fclose(f);
  return v;
}

void write_raw(const std::string &name, const void *p, size_t bytes) {
  const std::string path = g_dir + "/" + name;
  std::FILE *f = std::fopen(path.c_str(), "wb");
  if (!f || (bytes && std::fwrite(p, 1, bytes, f) != bytes)) {
    std::cerr << "cannot write " << path << std::endl;
    std::exit(2);
  }
  std::fclose(f);
}

// <case>.txt
class Txt {
public:
  explicit Txt(const std::string &name) : f_(std::fopen((g_dir + "/" + name + ".txt").c_str(), "w")) {
    if (!f_) {
      std::cerr << "cannot write " << name << ".txt" << std::endl;
      std::exit(2);
    }
  }
  ~Txt() { std::fclose(f_); }
  void i(const char *key, long long v) { std::fprintf(f_, "%s %lld\n", key, v); }
  void d(const char *key, double v) { std::fprintf(f_, "%s %a\n", key, v); }
  void pair(const char *key, const std::pair<double, double> &p) {
    d((std::string(key) + "_loss").c_str(), p.first);
    d((std::string(key) + "_acc").c_str(), p.second);
  }
  void eval(const char *key, const hip_mlp::EvalResult &e) {
    const std::string k(key);
    d((k + "_loss").c_str(), e.loss);
    i((k + "_rows").c_str(), e.rows);
    i((k + "_correct").c_str(), e.correct);
    i((k + "_topk").c_str(), e.topk);
    i((k + "_k").c_str(), e.k);
  }
  void stats(const lbf_owlqn_stats &s) {
    i("zeros", s.zeros);
    i("penalised", s.penalised);
    d("l1_term", s.l1_term);
    d("pg_norm", s.pg_norm);
  }

private:
  std::FILE *f_;
};

void dump_recorder(const std::string &name, const IterationRecorder<Backend> &rec) {
  std::vector<double> l, g, t;
  rec.copy_to_host(l, g, t);
  write_raw(name + ".loss.f64", l.data(), l.size() * sizeof(double));
  write_raw(name + ".gnorm.f64", g.data(), g.size() * sizeof(double));
  write_raw(name + ".time.f64", t.data(), t.size() * sizeof(double));
}

void dump_device(const std::string &file, hip_mlp::HipHandle &h, const void *d_ptr, size_t bytes) {
  std::vector<char> host(bytes);
  hip_mlp::hip_check(lbf_memcpy(h.get(), host.data(), d_ptr, bytes, 1), "lbf_memcpy");
  write_raw(file, host.data(), bytes);
}

void dump_params(const std::string &name, hip_mlp::HipNetwork &net) {
  dump_device(name + ".params.f32", net.handle(), net.params_data(), net.params_size() * sizeof(HipScalar));
}

// The column-major In x N matrix of the launcher is the row-major [N][In] file, element for element.
HostMatrix to_matrix(const std::vector<float> &v, long rows, long cols) {
  HostMatrix m(rows, cols);
  for (size_t i = 0; i < v.size(); ++i) m.data()[i] = double(v[i]);
  return m;
}

template <class P> struct Data {
  std::vector<float> xtr, ytr, xte, yte;
  Data()
      : xtr(read_f32(std::string(P::tag) + "_X_train.f32", size_t(P::NTrain) * P::In)),
        ytr(read_f32(std::string(P::tag) + "_Y_train.f32", size_t(P::NTrain) * P::Out)),
        xte(read_f32(std::string(P::tag) + "_X_test.f32", size_t(P::NTest) * P::In)),
        yte(read_f32(std::string(P::tag) + "_Y_test.f32", size_t(P::NTest) * P::Out)) {}
  UnifiedDataset dataset() const {
    UnifiedDataset d;
    d.train_x = to_matrix(xtr, P::In, P::NTrain);
    d.train_y = to_matrix(ytr, P::Out, P::NTrain);
    d.test_x = to_matrix(xte, P::In, P::NTest);
    d.test_y = to_matrix(yte, P::Out, P::NTest);
    return d;
  }
};

template <class P> void build(UnifiedLauncher<Backend> &l, const Data<P> &data) {
  l.template addLayer<P::In, P::Hid, typename P::HidAct>();
  l.template addLayer<P::Hid, P::Out, hip_mlp::Linear>();
  l.buildNetwork();
  l.setData(data.dataset());
}

template <class P> void build(hip_mlp::HipNetwork &net) {
  net.addLayer(P::In, P::Hid, P::HidAct::id);
  net.addLayer(P::Hid, P::Out, hip_mlp::Linear::id);
}

// train() + test(), then the dumps every launcher case shares
void run_case(const std::string &name, UnifiedLauncher<Backend> &l, UnifiedOptimizer<Backend> &opt,
              const UnifiedConfig &cfg, const lbf_owlqn_stats *stats = nullptr) {
  l.train(opt, cfg);
  l.test();
  Txt t(name);
  t.i("rows", opt.recorder.size());
  t.pair("train", l.lastTrain());
  t.pair("test", l.lastTest());
  if (stats) t.stats(*stats);
  dump_recorder(name, opt.recorder);
  dump_params(name, l.getWrapper().getInternal());
}

// The direct minimizer classes: a device copy of one split
struct DeviceSplit {
  hip_mlp::DeviceBuffer<HipScalar> x, y;
  DeviceSplit(hip_mlp::HipHandle &h, const std::vector<float> &xv, const std::vector<float> &yv)
      : x(h, xv.size()), y(h, yv.size()) {
    x.copy_from_host(xv.data(), xv.size());
    y.copy_from_host(yv.data(), yv.size());
  }
};

void finish_direct(const std::string &name, hip_mlp::HipMinimizerBase &s, const IterationRecorder<Backend> &rec,
                   hip_mlp::HipNetwork &net, const lbf_owlqn_stats *stats = nullptr) {
  Txt t(name);
  t.i("iterations", s.iterations());
  t.i("rows", rec.size());
  if (stats) t.stats(*stats);
  dump_recorder(name, rec);
  dump_params(name, net);
}

UnifiedConfig config(const char *name, int max_iters, double tolerance, unsigned seed) {
  UnifiedConfig c;
  c.name = g_dir + "/" + name; // the history CSV goes next to the dumps
  c.max_iters = max_iters;
  c.tolerance = tolerance;
  c.seed = seed;
  c.log_interval = 2;
  return c;
}

} // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::cerr << "usage: parity_hip <dir>" << std::endl;
    return 2;
  }
  g_dir = argv[1];
  const Data<P1> d1;
  const Data<P2> d2;

  { // 1a. full-batch L-BFGS, Armijo (the CUDA semantics), MSE
    UnifiedLauncher<Backend> l;
    build(l, d1);
    UnifiedConfig c = config("lbfgs_armijo", 8, 1e-9, 99u);
    c.m_param = 4;
    UnifiedLBFGS_HIP opt;
    run_case("lbfgs_armijo", l, opt, c);
  }
  { // 1b. Wolfe (the CPU semantics) on the cross-entropy loss with l2; the tolerance ends the run
    UnifiedLauncher<Backend> l;
    l.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy); // before buildNetwork(): replayed at creation
    build(l, d2);
    UnifiedConfig c = config("lbfgs_wolfe", 60, 0.05, 99u);
    c.m_param = 4;
    c.l2 = 2e-3;
    UnifiedLBFGS_HIP opt;
    opt.line_search = LBF_LS_WOLFE;
    run_case("lbfgs_wolfe", l, opt, c);

    // 7. a second train() on the same launcher continues from the first run's parameters; l2 stays set
    UnifiedConfig c2 = config("lbfgs_continue", 3, 1e-9, 5u);
    c2.m_param = 4;
    c2.reset_params = false;
    UnifiedLBFGS_HIP again;
    again.line_search = LBF_LS_WOLFE;
    run_case("lbfgs_continue", l, again, c2);

    // 8. evaluation of the trained network
    Txt t("eval");
    auto &net = l.getWrapper().getInternal();
    std::vector<long long> conf;
    t.eval("metrics_train", l.metrics(false, 3, &conf));
    write_raw("eval.confusion_train.i64", conf.data(), conf.size() * sizeof(long long));
    t.eval("metrics_test", l.metrics(true, 1));
    DeviceSplit train(net.handle(), d2.xtr, d2.ytr), test(net.handle(), d2.xte, d2.yte);
    hip_mlp::DeviceBuffer<int> d_pred(net.handle(), P2::NTest);
    std::vector<long long> conf_test;
    t.eval("evaluate_test", net.evaluate(test.x.data(), test.y.data(), P2::NTest, 2, &conf_test, d_pred.data()));
    write_raw("eval.confusion_test.i64", conf_test.data(), conf_test.size() * sizeof(long long));
    dump_device("eval.pred_test.i32", net.handle(), d_pred.data(), P2::NTest * sizeof(int));
    t.d("loss_and_grad", double(net.compute_loss_and_grad(train.x.data(), train.y.data(), P2::NTrain)));
    dump_device("eval.grad.f32", net.handle(), net.grads_data(), net.params_size() * sizeof(HipScalar));
    hip_mlp::DeviceBuffer<HipScalar> d_out(net.handle(), size_t(P2::NTest) * P2::Out);
    net.forward_only(test.x.data(), P2::NTest, d_out.data());
    dump_device("eval.forward_test.f32", net.handle(), d_out.data(), d_out.size() * sizeof(HipScalar));
    t.pair("train", l.lastTrain());
    t.pair("test", l.lastTest());
    dump_params("eval", net);
  }
  for (int curvature : {LBF_HVP_FD, LBF_HVP_GAUSS_NEWTON}) { // 2. S-LBFGS, both kinds of curvature pair
    UnifiedLauncher<Backend> l;
    l.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
    build(l, d2);
    const char *name = curvature == LBF_HVP_FD ? "slbfgs_fd" : "slbfgs_gn";
    UnifiedConfig c = config(name, 6, 1e-9, 7u);
    c.m_param = 3;
    c.L_param = 2;
    c.batch_size = 32;
    c.b_H_param = 20;
    c.learning_rate = 0.03;
    c.curvature = curvature;
    UnifiedSLBFGS_HIP opt;
    run_case(name, l, opt, c);
  }
  { // 3a. gradient descent with momentum and l2
    UnifiedLauncher<Backend> l;
    build(l, d1);
    UnifiedConfig c = config("gd", 7, 1e-9, 11u);
    c.learning_rate = 0.05;
    c.momentum = 0.6;
    c.l2 = 1e-3;
    UnifiedGD_HIP opt;
    run_case("gd", l, opt, c);
  }
  for (int batch : {64, 48}) { // 3b. minibatch SGD with step decay; 257 rows leave a ragged last batch of 1 / 17
    UnifiedLauncher<Backend> l;
    l.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
    build(l, d2);
    const char *name = batch == 64 ? "sgd" : "sgd_b48";
    UnifiedConfig c = config(name, 6, 1e-9, 12u); // the tolerance is not passed on: SGD keeps its own
    c.learning_rate = 0.02;
    c.momentum = 0.5;
    c.batch_size = batch;
    c.lr_decay = 0.7;
    c.lr_decay_rate = 2;
    UnifiedSGD_HIP opt;
    run_case(name, l, opt, c);
  }
  { // 4a. Hessian-free through the launcher
    UnifiedLauncher<Backend> l;
    l.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
    build(l, d2);
    UnifiedConfig c = config("hf", 6, 1e-9, 13u);
    c.cg_iters = 4;
    c.cg_rtol = 0.3;
    c.damping = 0.05;
    UnifiedHF_HIP opt;
    run_case("hf", l, opt, c);
  }
  { // 4b. HipHF on a network of one's own, curvature on a window of 16 rows
    hip_mlp::HipHandle h;
    hip_mlp::HipNetwork net(h);
    build<P1>(net);
    net.bindParams(17u);
    DeviceSplit train(h, d1.xtr, d1.ytr);
    hip_mlp::HipHF s(h, net);
    IterationRecorder<Backend> rec;
    rec.init(12);
    s.setRecorder(&rec);
    s.setMaxIterations(12);
    s.setTolerance(0.1f);
    s.setCG(5, 0.2);
    s.setDamping(0.3);
    s.setCurvatureRows(16);
    s.setLineSearchParams(6, 0.6f, 0.4f);
    s.solve(int(net.params_size()), net.params_data(), train.x.data(), train.y.data(), P1::NTrain, {});
    finish_direct("hiphf", s, rec, net);
  }
  { // 5a. OWL-QN through the launcher, l1 and l2
    UnifiedLauncher<Backend> l;
    l.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
    build(l, d2);
    UnifiedConfig c = config("owlqn", 8, 1e-9, 14u);
    c.m_param = 2;
    c.l1 = 2e-3;
    c.l2 = 1e-3;
    UnifiedOWLQN_HIP opt;
    run_case("owlqn", l, opt, c, &opt.stats);
  }
  { // 5b. HipOWLQN, the biases penalised too
    hip_mlp::HipHandle h;
    hip_mlp::HipNetwork net(h);
    build<P1>(net);
    net.bindParams(18u);
    DeviceSplit train(h, d1.xtr, d1.ytr);
    hip_mlp::HipOWLQN s(h, net);
    IterationRecorder<Backend> rec;
    rec.init(9);
    s.setRecorder(&rec);
    s.setMaxIterations(9);
    s.setTolerance(1e-9f);
    s.setL1(0.01, true);
    s.setHistorySize(3);
    s.solve(int(net.params_size()), net.params_data(), train.x.data(), train.y.data(), P1::NTrain, {});
    finish_direct("hipowlqn", s, rec, net, &s.stats());
  }
  for (int ls : {LBF_LS_ARMIJO, LBF_LS_WOLFE}) { // 6. HipLBFGS on a callback that evaluates the network at `p`
    hip_mlp::HipHandle h;
    hip_mlp::HipNetwork net(h);
    build<P1>(net);
    net.bindParams(19u);
    DeviceSplit train(h, d1.xtr, d1.ytr);
    // The engine hands the callback a trial point that is not net.params_data(): evaluate there, not at the
    // network's own buffer (compute_loss_and_grad would ignore p).
    hip_mlp::HipMinimizerBase::LossGradFun fn = [&net](const HipScalar *p, HipScalar *grad, const HipScalar *input,
                                                       const HipScalar *target, int batch) -> HipScalar {
      double loss = 0.0;
      hip_mlp::hip_check(lbf_mlp_loss_grad(net.raw(), p, grad, input, target, nullptr, batch, 1.0 / batch, 0.0, &loss),
                         "lbf_mlp_loss_grad");
      return HipScalar(loss);
    };
    hip_mlp::HipLBFGS s(h);
    IterationRecorder<Backend> rec;
    rec.init(8);
    s.setRecorder(&rec);
    s.setMemory(5);
    s.setLineSearch(ls);
    s.setMaxIterations(8);
    s.setTolerance(1e-9f);
    s.setLineSearchParams(7, 0.5f, 0.4f); // read under Armijo only
    s.solve(int(net.params_size()), net.params_data(), train.x.data(), train.y.data(), P1::NTrain, fn);
    finish_direct(ls == LBF_LS_ARMIJO ? "hiplbfgs_armijo" : "hiplbfgs_wolfe", s, rec, net);
  }
  std::cout << "[RESULT] ok" << std::endl;
  return 0;
}
