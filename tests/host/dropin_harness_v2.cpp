// tests/host/dropin_harness_v2.cpp — dropin_harness.cpp's checks for the classes of include/lbfgs_amd/hip_backend.hpp
// that call entry points outside the earlier ABI: HipNetwork::gradSq, HipHFPreconditioned, HipAdam,
// UnifiedHFPreconditioned_HIP and UnifiedAdam_HIP, against fake_lbf_abi.cpp plus fake_lbf_abi_v2.cpp. Every field of
// lbf_hf_params, lbf_hf_precond and lbf_adam_params, the pointers and row counts, the recorder, iterations(), and
// Adam's trace capacity and trim. tests/test_dropin_host.py builds it plain and with AddressSanitizer +
// UndefinedBehaviorSanitizer and runs it as its own process.
//   usage: dropin_harness_v2 <work dir>          prints "dropin harness v2 ok"
#include "fake_lbf_abi_v2.hpp"
#include "lbfgs_amd/hip_backend.hpp"

#include <cstdio>
#include <fstream>
#include <unistd.h>

#define CHECK(cond)                                                                                       \
  do {                                                                                                    \
    if (!(cond)) {                                                                                        \
      std::fprintf(stderr, "CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond);                     \
      std::exit(1);                                                                                       \
    }                                                                                                     \
  } while (0)

using hip_mlp::HipScalar;
using hip_mlp::HostMatrix;

namespace {

// N = 5 rows in batches of 2 over 2 epochs: ceil(5 / 2) * 2 = 6 steps. Rounding down gives 4, forgetting the
// epochs 3, so a wrong capacity shows; the fake writes 4 entries, so the trim shows too.
constexpr int In = 6, Hid = 5, Out = 3, NTrain = 5, NTest = 4, Batch = 2, Epochs = 2, TraceCap = 6, TraceRun = 4;
constexpr long long NParams = (In + 1) * Hid + (Hid + 1) * Out;

// Every field non-default and distinct from every other, so a swap shows.
UnifiedConfig distinct_config() {
  UnifiedConfig c;
  c.name = "v2name";
  c.max_iters = Epochs;
  c.tolerance = 0.0625;
  c.learning_rate = 0.03125;
  c.momentum = 0.71;
  c.lr_decay = 0.37;
  c.lr_decay_rate = 3;
  c.batch_size = Batch;
  c.m_param = 7;
  c.L_param = 5;
  c.b_H_param = 9;
  c.log_interval = 1;
  c.reset_params = true;
  c.seed = 777u;
  c.l2 = 0.0123;
  c.curvature = LBF_HVP_GAUSS_NEWTON;
  c.cg_iters = 13;
  c.cg_rtol = 0.19;
  c.damping = 2.5;
  c.l1 = 0.0047;
  c.beta1 = 0.81;
  c.beta2 = 0.93;
  c.adam_eps = 3e-7;
  c.weight_decay = 0.011;
  c.clip_norm = 1.75;
  c.shuffle = false;
  return c;
}

UnifiedDataset dataset() {
  UnifiedDataset d;
  d.train_x = HostMatrix(In, NTrain);
  d.train_y = HostMatrix(Out, NTrain);
  d.test_x = HostMatrix(In, NTest);
  d.test_y = HostMatrix(Out, NTest);
  for (long i = 0; i < d.train_x.size(); ++i) d.train_x.data()[i] = 0.25 * double(i % 9);
  for (long i = 0; i < d.train_y.size(); ++i) d.train_y.data()[i] = 0.125 * double(i % 7);
  return d;
}

void build_net(hip_mlp::HipNetwork &net) {
  net.addLayer(In, Hid, hip_mlp::Tanh::id);
  net.addLayer(Hid, Out, hip_mlp::Linear::id);
}

// the fields of lbf_hf_params that no class of the header sets: the library's defaults, no traces
void check_hf_untouched(const lbf_hf_params &p) {
  CHECK(p.cg_check == 10 && p.damp_up == 1.5 && p.damp_down == 2.0 / 3.0 && p.ratio_lo == 0.25 && p.ratio_hi == 0.75);
  CHECK(p.damping_trace == nullptr && p.ratio_trace == nullptr && p.cg_trace == nullptr && p.trace_cap == 0);
}

void check_trace(const std::vector<double> &t) {
  CHECK(t.size() == size_t(TraceRun));
  for (int i = 0; i < TraceRun; ++i) CHECK(t[size_t(i)] == 400.0 + i);
}

void test_grad_sq() {
  hip_mlp::HipHandle h;
  hip_mlp::HipNetwork net(h);
  build_net(net);
  net.bindParams(31);
  hip_mlp::DeviceBuffer<float> x(h, 8 * In), y(h, 8 * Out), out(h, size_t(NParams));
  fake2::state().log.clear();
  net.gradSq(x.data(), y.data(), 8, 0.125, out.data());
  CHECK(fake2::state().log.size() == 1);
  const fake2::Call *c = fake2::last("mlp_grad_sq");
  CHECK(c && c->net == net.raw() && c->params == net.params_data() && c->X == x.data() && c->Y == y.data());
  CHECK(c->idx == nullptr && c->batch == 8 && c->scale == 0.125 && c->out == out.data());
  std::vector<float> back(static_cast<size_t>(NParams));
  out.copy_to_host(back.data(), back.size());
  CHECK(back[0] == 0.0f && back[size_t(NParams) - 1] == float(NParams - 1) * 0.25f);
}

void test_hip_hf_preconditioned() {
  auto &st = fake::state();
  hip_mlp::HipHandle h;
  hip_mlp::HipNetwork net(h);
  build_net(net);
  net.bindParams(31);
  hip_mlp::DeviceBuffer<float> in(h, 8 * In), tg(h, 8 * Out), other(h, size_t(NParams));
  hip_mlp::HipMinimizerBase::LossGradFun unused;
  st.rows_to_write = 4;
  st.iterations = 3;
  IterationRecorder<HipBackend> rec;
  rec.init(6);
  hip_mlp::HipHFPreconditioned s(h, net);
  fake2::state().log.clear();
  st.log.clear();
  s.solve(int(NParams), net.params_data(), in.data(), tg.data(), 8, unused); // untouched: the class's defaults
  const fake2::Call *d = fake2::last("hf_solve_pc");
  CHECK(d && d->hf.max_iters == 200 && d->hf.tol == double(1e-6f) && d->hf.cg_iters == 50 && d->hf.cg_rtol == 0.1);
  CHECK(d->hf.damping0 == 1.0 && d->hf.curv_rows == 0 && d->hf.max_line_iters == 20);
  CHECK(d->hf.c1 == double(1e-4f) && d->hf.rho == 0.5 && d->rec == nullptr && d->info != nullptr);
  check_hf_untouched(d->hf);
  CHECK(d->has_precond && d->precond.mode == LBF_PRECOND_GRAD_SQ && d->precond.exponent == 0.75);
  CHECK(d->precond.refresh == 1 && s.iterations() == 3);
  s.setRecorder(&rec);
  s.setMaxIterations(23);
  s.setTolerance(0.017f);
  s.setCG(13, 0.19);
  s.setDamping(2.5);
  s.setCurvatureRows(16);
  s.setLineSearchParams(9, 0.003f, 0.4f);
  s.setPreconditioner(0.4, 5);
  fake2::state().log.clear();
  s.solve(int(NParams), other.data(), in.data(), tg.data(), 8, unused);
  CHECK(fake2::count("hf_solve_pc") == 1 && st.log.empty()); // and not lbf_hf_solve
  const fake2::Call *c = fake2::last("hf_solve_pc");
  CHECK(c->net == net.raw() && c->params == other.data() && c->X == in.data() && c->Y == tg.data());
  CHECK(c->n_local == 8 && c->n_global == 8);
  CHECK(c->hf.max_iters == 23 && c->hf.tol == double(0.017f) && c->hf.cg_iters == 13 && c->hf.cg_rtol == 0.19);
  CHECK(c->hf.damping0 == 2.5 && c->hf.curv_rows == 16);
  CHECK(c->hf.c1 == double(0.003f) && c->hf.rho == double(0.4f) && c->hf.max_line_iters == 9);
  check_hf_untouched(c->hf);
  CHECK(c->has_precond && c->precond.mode == LBF_PRECOND_GRAD_SQ && c->precond.exponent == 0.4);
  CHECK(c->precond.refresh == 5);
  lbf_record v = rec.view();
  CHECK(c->rec_loss == v.loss && c->rec_grad_norm == v.grad_norm && c->rec_time_ms == v.time_ms);
  CHECK(c->rec_cap == 6 && c->rec_size_in == 0 && c->rec_alpha == nullptr);
  CHECK(rec.size() == 4 && s.iterations() == 3);
  s.setPreconditioner(0.6); // refresh defaults to 1
  s.solve(int(NParams), other.data(), in.data(), tg.data(), 8, unused);
  CHECK(fake2::last("hf_solve_pc")->precond.exponent == 0.6 && fake2::last("hf_solve_pc")->precond.refresh == 1);
  st.rows_to_write = 1000; // a solver that fills the record
  s.solve(int(NParams), other.data(), in.data(), tg.data(), 8, unused);
  CHECK(rec.size() == 6);
  st.rows_to_write = 4;
  fake2::state().log.clear(); // nothing to solve: no engine call, zero iterations
  s.solve(0, other.data(), in.data(), tg.data(), 8, unused);
  CHECK(s.iterations() == 0 && fake2::state().log.empty());
  s.solve(int(NParams), other.data(), in.data(), tg.data(), 8, unused);
  CHECK(s.iterations() == 3);
  s.solve(int(NParams), nullptr, in.data(), tg.data(), 8, unused);
  CHECK(s.iterations() == 0 && fake2::count("hf_solve_pc") == 1);
}

void test_hip_adam() {
  auto &st = fake::state();
  hip_mlp::HipHandle h;
  hip_mlp::HipNetwork net(h);
  build_net(net);
  net.bindParams(31);
  hip_mlp::DeviceBuffer<float> in(h, NTrain * In), tg(h, NTrain * Out), other(h, size_t(NParams));
  hip_mlp::HipMinimizerBase::LossGradFun unused;
  st.rows_to_write = 3;
  st.iterations = 3;
  fake2::state().trace_to_write = TraceRun;
  hip_mlp::HipAdam s(h, net);
  CHECK(s.lossTrace().empty());
  fake2::state().log.clear();
  s.solve(int(NParams), net.params_data(), in.data(), tg.data(), NTrain, unused); // untouched: the defaults
  const fake2::Call *d = fake2::last("adam_solve");
  CHECK(d && d->adam.lr == 1e-3 && d->adam.beta1 == 0.9 && d->adam.beta2 == 0.999 && d->adam.eps == 1e-8);
  CHECK(d->adam.weight_decay == 0.0 && d->adam.clip_norm == 0.0 && d->adam.batch == 128 && d->adam.shuffle == 1);
  CHECK(d->adam.seed == 123u && d->adam.decay_rate == 1.0 && d->adam.decay_step == 0);
  CHECK(d->adam.max_epochs == 200 && d->adam.tol == double(1e-6f)); // the base class's iterations and tolerance
  CHECK(d->adam.trace_cap == 200 && d->adam.loss_trace != nullptr && d->trace_nan_on_entry); // one step per epoch
  CHECK(d->rec == nullptr && d->info != nullptr && s.iterations() == 3);
  check_trace(s.lossTrace());

  IterationRecorder<HipBackend> rec;
  rec.init(Epochs + 1);
  s.setRecorder(&rec);
  s.setMaxIterations(Epochs);
  s.setTolerance(0.017f);
  s.setLearningRate(0.03125);
  s.setBetas(0.81, 0.93);
  s.setEpsilon(3e-7);
  s.setWeightDecay(0.011);
  s.setClipNorm(1.75);
  s.setBatchSize(Batch);
  s.setShuffle(false, 777u);
  s.setLearningRateDecay(0.37, 3);
  fake2::state().log.clear();
  s.solve(int(NParams), other.data(), in.data(), tg.data(), NTrain, unused);
  CHECK(fake2::count("adam_solve") == 1);
  const fake2::Call *c = fake2::last("adam_solve");
  CHECK(c->net == net.raw() && c->params == other.data() && c->X == in.data() && c->Y == tg.data());
  CHECK(c->n_local == NTrain);
  CHECK(c->adam.lr == 0.03125 && c->adam.beta1 == 0.81 && c->adam.beta2 == 0.93 && c->adam.eps == 3e-7);
  CHECK(c->adam.weight_decay == 0.011 && c->adam.clip_norm == 1.75 && c->adam.batch == Batch);
  CHECK(c->adam.shuffle == 0 && c->adam.seed == 777u && c->adam.decay_rate == 0.37 && c->adam.decay_step == 3);
  CHECK(c->adam.max_epochs == Epochs && c->adam.tol == double(0.017f));
  CHECK(c->adam.trace_cap == TraceCap && c->adam.loss_trace != nullptr && c->trace_nan_on_entry);
  CHECK(c->adam.loss_trace == s.lossTrace().data()); // the engine wrote into the vector that lossTrace() returns
  check_trace(s.lossTrace());
  lbf_record v = rec.view();
  CHECK(c->rec_loss == v.loss && c->rec_grad_norm == v.grad_norm && c->rec_time_ms == v.time_ms);
  CHECK(c->rec_cap == Epochs + 1 && c->rec_size_in == 0 && c->rec_alpha == nullptr);
  CHECK(rec.size() == 3 && s.iterations() == 3);
  s.setShuffle(true); // the seed defaults to 123
  s.solve(int(NParams), other.data(), in.data(), tg.data(), NTrain, unused);
  CHECK(fake2::last("adam_solve")->adam.shuffle == 1 && fake2::last("adam_solve")->adam.seed == 123u);
  { // a solve that runs every step keeps the whole trace; one that runs none, nothing
    fake2::state().trace_to_write = 1000;
    s.solve(int(NParams), other.data(), in.data(), tg.data(), NTrain, unused);
    CHECK(s.lossTrace().size() == size_t(TraceCap) && s.lossTrace()[TraceCap - 1] == 400.0 + TraceCap - 1);
    fake2::state().trace_to_write = 0;
    s.solve(int(NParams), other.data(), in.data(), tg.data(), NTrain, unused);
    CHECK(s.lossTrace().empty() && fake2::last("adam_solve")->adam.trace_cap == TraceCap);
    fake2::state().trace_to_write = TraceRun;
  }
  { // batch 0 (the engine rejects it; the header must not divide by it): no trace, a null pointer
    s.setBatchSize(0);
    s.solve(int(NParams), other.data(), in.data(), tg.data(), NTrain, unused);
    const fake2::Call *z = fake2::last("adam_solve");
    CHECK(z->adam.batch == 0 && z->adam.trace_cap == 0 && z->adam.loss_trace == nullptr && s.lossTrace().empty());
    s.setBatchSize(Batch);
    s.setMaxIterations(0); // no epochs: the same
    s.solve(int(NParams), other.data(), in.data(), tg.data(), NTrain, unused);
    z = fake2::last("adam_solve");
    CHECK(z->adam.max_epochs == 0 && z->adam.trace_cap == 0 && z->adam.loss_trace == nullptr);
    s.setMaxIterations(Epochs);
  }
  fake2::state().log.clear(); // nothing to solve: no engine call, zero iterations
  s.solve(0, other.data(), in.data(), tg.data(), NTrain, unused);
  CHECK(s.iterations() == 0 && fake2::state().log.empty());
  s.solve(int(NParams), other.data(), in.data(), tg.data(), NTrain, unused);
  CHECK(s.iterations() == 3);
  s.solve(int(NParams), nullptr, in.data(), tg.data(), NTrain, unused);
  CHECK(s.iterations() == 0 && fake2::count("adam_solve") == 1);
}

template <class L> void add_layers(L &l) {
  l.template addLayer<In, Hid, hip_mlp::Tanh>();
  l.template addLayer<Hid, Out, hip_mlp::Linear>();
}

// what every Unified* strategy must hand its solver besides the parameter struct
void check_unified_call(const fake2::Call *c, UnifiedLauncher<HipBackend> &l, UnifiedOptimizer<HipBackend> &opt,
                        int cap, int rows) {
  auto &net = l.getWrapper().getInternal();
  CHECK(c && c->net == net.raw() && c->params == net.params_data());
  CHECK(c->X != nullptr && c->Y != nullptr && c->X != c->Y);
  CHECK(c->n_local == NTrain && c->n_global == NTrain); // train_x.cols()
  lbf_record v = opt.recorder.view();
  CHECK(c->rec_loss == v.loss && c->rec_grad_norm == v.grad_norm && c->rec_time_ms == v.time_ms);
  CHECK(c->rec_cap == cap && c->rec_size_in == 0 && c->info != nullptr);
  CHECK(opt.recorder.size() == rows);
}

void test_unified_strategies() {
  auto &st = fake::state();
  st.forward_tables[NTrain] = std::vector<float>(NTrain * Out, 0.25f);
  UnifiedLauncher<HipBackend> l;
  add_layers(l);
  l.buildNetwork();
  l.setData(dataset());
  const UnifiedConfig cfg = distinct_config();
  st.rows_to_write = 1000; // fill the record: its capacity is the row count
  st.iterations = 2;
  fake2::state().trace_to_write = TraceRun;
  {
    UnifiedHFPreconditioned_HIP o;
    fake2::state().log.clear();
    st.log.clear();
    l.train(o, cfg); // setPreconditioner untouched: exponent 0.75, refresh 1
    CHECK(fake2::count("hf_solve_pc") == 1 && fake::count("hf_solve") == 0);
    const fake2::Call *c = fake2::last("hf_solve_pc");
    check_unified_call(c, l, o, cfg.max_iters, cfg.max_iters);
    CHECK(c->hf.max_iters == Epochs && c->hf.tol == 0.0625 && c->hf.cg_iters == 13 && c->hf.cg_rtol == 0.19);
    CHECK(c->hf.damping0 == 2.5 && c->hf.curv_rows == 0);
    CHECK(c->hf.c1 == 1e-4 && c->hf.rho == 0.5 && c->hf.max_line_iters == 20);
    check_hf_untouched(c->hf);
    CHECK(c->has_precond && c->precond.mode == LBF_PRECOND_GRAD_SQ && c->precond.exponent == 0.75);
    CHECK(c->precond.refresh == 1);
    o.setPreconditioner(0.4, 5);
    l.train(o, cfg);
    c = fake2::last("hf_solve_pc");
    CHECK(c->precond.mode == LBF_PRECOND_GRAD_SQ && c->precond.exponent == 0.4 && c->precond.refresh == 5);
    o.setPreconditioner(0.6);
    l.train(o, cfg);
    CHECK(fake2::last("hf_solve_pc")->precond.exponent == 0.6 && fake2::last("hf_solve_pc")->precond.refresh == 1);
  }
  {
    UnifiedAdam_HIP o;
    fake2::state().log.clear();
    l.train(o, cfg); // lr_decay > 0: the decay fields are the config's
    CHECK(fake2::count("adam_solve") == 1);
    const fake2::Call *c = fake2::last("adam_solve");
    check_unified_call(c, l, o, cfg.max_iters + 1, cfg.max_iters + 1);
    CHECK(c->adam.lr == 0.03125 && c->adam.beta1 == 0.81 && c->adam.beta2 == 0.93 && c->adam.eps == 3e-7);
    CHECK(c->adam.weight_decay == 0.011 && c->adam.clip_norm == 1.75 && c->adam.batch == Batch);
    CHECK(c->adam.shuffle == 0 && c->adam.seed == 777u && c->adam.decay_rate == 0.37 && c->adam.decay_step == 3);
    CHECK(c->adam.max_epochs == Epochs && c->adam.tol == 1e-6); // Adam keeps its own tolerance, like SGD
    CHECK(c->adam.trace_cap == TraceCap && c->adam.loss_trace != nullptr && c->trace_nan_on_entry);
    CHECK(c->adam.loss_trace == o.trace.data());
    check_trace(o.trace);
    std::vector<double> lo, g, t;
    o.recorder.copy_to_host(lo, g, t);
    CHECK(lo.size() == size_t(Epochs + 1) && lo[Epochs] == 100.0 + Epochs && t[Epochs] == 300.0 + Epochs);
    std::ifstream f("v2name_history.csv"); // the header and every row, at log_interval 1
    int n = 0;
    for (std::string s; std::getline(f, s);) ++n;
    CHECK(n == Epochs + 2);

    UnifiedConfig c0 = cfg; // lr_decay = 0: the library's defaults stay, not the config's step
    c0.lr_decay = 0.0;
    c0.shuffle = true;
    l.train(o, c0);
    c = fake2::last("adam_solve");
    CHECK(c->adam.decay_rate == 1.0 && c->adam.decay_step == 0 && c->adam.shuffle == 1 && c->adam.lr == 0.03125);
    c0.lr_decay = -0.5;
    l.train(o, c0);
    CHECK(fake2::last("adam_solve")->adam.decay_rate == 1.0 && fake2::last("adam_solve")->adam.decay_step == 0);

    fake2::state().trace_to_write = 1000; // every step ran: nothing to trim
    l.train(o, cfg);
    CHECK(o.trace.size() == size_t(TraceCap));
    fake2::state().trace_to_write = TraceRun;
    c0 = cfg; // batch 0: no trace, a null pointer
    c0.batch_size = 0;
    l.train(o, c0);
    c = fake2::last("adam_solve");
    CHECK(c->adam.batch == 0 && c->adam.trace_cap == 0 && c->adam.loss_trace == nullptr && o.trace.empty());
  }
}

} // namespace

int main(int argc, char **argv) {
  if (argc < 2 || chdir(argv[1]) != 0) {
    std::fprintf(stderr, "usage: dropin_harness_v2 <work dir>\n");
    return 2;
  }
  test_grad_sq();
  test_hip_hf_preconditioned();
  test_hip_adam();
  test_unified_strategies();
  CHECK(fake::state().live_allocs == 0 && fake::state().live_nets == 0 && fake::state().live_ctxs == 0);
  std::printf("dropin harness v2 ok\n");
  return 0;
}
