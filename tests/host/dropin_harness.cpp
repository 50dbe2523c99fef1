// tests/host/dropin_harness.cpp — runs every class of include/lbfgs_amd/hip_backend.hpp on a CPU, against the
// recording fake of the C ABI (fake_lbf_abi.cpp), and checks what the header hands the engine: every field of
// every parameter struct, the pointers and sizes, the launcher's call order, the host scan of evaluate(), the
// metrics rescaling, the recorder, the history CSV and the small host classes. tests/test_dropin_host.py builds it
// plain and with AddressSanitizer + UndefinedBehaviorSanitizer and runs it as its own process.
//   usage: dropin_harness <work dir>            prints "dropin harness ok"
//          dropin_harness <work dir> abort_l2   HipNetwork::setL2(-1) before bindParams(): dies with SIGABRT
#include "fake_lbf_abi.hpp"
#include "lbfgs_amd/hip_backend.hpp"

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <limits>
#include <sstream>
#include <unistd.h>

#define CHECK(cond)                                                                                       \
  do {                                                                                                    \
    if (!(cond)) {                                                                                        \
      std::fprintf(stderr, "CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond);                     \
      std::exit(1);                                                                                       \
    }                                                                                                     \
  } while (0)

using hip_mlp::HostMatrix;
using hip_mlp::HipScalar;

namespace {

constexpr int In = 6, Hid = 5, Out = 3, NTrain = 7, NTest = 4;
constexpr long long NParams = (In + 1) * Hid + (Hid + 1) * Out;

// Every field non-default and distinct from every other, so a swap shows.
UnifiedConfig distinct_config() {
  UnifiedConfig c;
  c.name = "cfgname";
  c.max_iters = 11;
  c.tolerance = 0.0625;
  c.learning_rate = 0.03125;
  c.momentum = 0.71;
  c.lr_decay = 0.37;
  c.lr_decay_rate = 3;
  c.batch_size = 14;
  c.m_param = 7;
  c.L_param = 5;
  c.b_H_param = 9;
  c.log_interval = 4;
  c.reset_params = true;
  c.seed = 777u;
  c.l2 = 0.0123;
  c.curvature = LBF_HVP_GAUSS_NEWTON;
  c.cg_iters = 13;
  c.cg_rtol = 0.19;
  c.damping = 2.5;
  c.l1 = 0.0047;
  return c;
}

UnifiedDataset dataset(long n_train = NTrain, long n_test = NTest) {
  UnifiedDataset d;
  d.train_x = HostMatrix(In, n_train);
  d.train_y = HostMatrix(Out, n_train);
  d.test_x = HostMatrix(In, n_test);
  d.test_y = HostMatrix(Out, n_test);
  for (long i = 0; i < d.train_x.size(); ++i) d.train_x.data()[i] = 0.25 * double(i % 9);
  for (long i = 0; i < d.test_x.size(); ++i) d.test_x.data()[i] = 0.5 * double(i % 5);
  for (long i = 0; i < d.train_y.size(); ++i) d.train_y.data()[i] = 0.125 * double(i % 7);
  for (long i = 0; i < d.test_y.size(); ++i) d.test_y.data()[i] = 0.375 * double(i % 3);
  return d;
}

bool exists(const std::string &p) { return std::ifstream(p).good(); }

std::vector<std::string> lines(const std::string &p) {
  std::ifstream f(p);
  std::vector<std::string> v;
  for (std::string s; std::getline(f, s);) v.push_back(s);
  return v;
}

// ---- references for the host scan, from the same table, in long double ----------------------------------------
// the documented scan (lbfgs_amd.h): best = 0, m = -1e20; a strictly larger value takes over; NaN never does
int scan_argmax(const long double *row, int n) {
  int best = 0;
  long double m = -1e20L;
  for (int o = 0; o < n; ++o)
    if (row[o] > m) {
      m = row[o];
      best = o;
    }
  return best;
}

struct ScanRef {
  long double loss_sum = 0; // MSE: sum of squared differences; cross-entropy: sum over samples
  long correct = 0;
  long double scale = 0;    // cross-entropy: max over samples of (|lse| + max |z|) * sum y
};

ScanRef scan_reference(const std::vector<float> &z, const std::vector<double> &y, long batch, bool xent) {
  ScanRef r;
  for (long i = 0; i < batch; ++i) {
    long double zr[Out], yr[Out];
    for (int o = 0; o < Out; ++o) {
      zr[o] = (long double)z[size_t(o + i * Out)];
      yr[o] = (long double)y[size_t(o + i * Out)];
    }
    if (scan_argmax(zr, Out) == scan_argmax(yr, Out)) ++r.correct;
    if (!xent) {
      for (int o = 0; o < Out; ++o) r.loss_sum += (zr[o] - yr[o]) * (zr[o] - yr[o]);
    } else {
      long double m = zr[0], amax = fabsl(zr[0]), ysum = 0;
      for (int o = 1; o < Out; ++o) {
        if (zr[o] > m) m = zr[o];
        if (fabsl(zr[o]) > amax) amax = fabsl(zr[o]);
      }
      long double se = 0;
      for (int o = 0; o < Out; ++o) se += expl(zr[o] - m);
      const long double lse = m + logl(se);
      for (int o = 0; o < Out; ++o) {
        r.loss_sum += yr[o] * (lse - zr[o]);
        ysum += yr[o];
      }
      const long double sc = (fabsl(lse) + amax) * ysum;
      if (sc > r.scale) r.scale = sc;
    }
  }
  return r;
}

// ---- sections ------------------------------------------------------------------------------------------------

void test_host_matrix() {
  HostMatrix m(3, 4);
  CHECK(m.rows() == 3 && m.cols() == 4 && m.size() == 12);
  for (long i = 0; i < 12; ++i) CHECK(m.data()[i] == 0.0);
  m(2, 1) = 7.0; // column-major: element (i, j) at i + j * rows
  CHECK(m.data()[2 + 1 * 3] == 7.0);
  m.data()[1 + 3 * 3] = 9.0;
  const HostMatrix &cm = m;
  CHECK(cm(1, 3) == 9.0 && cm(2, 1) == 7.0 && cm.data() == m.data());
  HostMatrix e;
  CHECK(e.rows() == 0 && e.cols() == 0 && e.size() == 0);
}

void test_device_buffer_and_handle() {
  auto &st = fake::state();
  {
    hip_mlp::HipHandle h(0);
    CHECK(h.get() != nullptr && st.live_ctxs == 1);
    h.sync();
    CHECK(fake::last("ctx_sync") && fake::last("ctx_sync")->ctx == h.get());
    const std::vector<char> id = hip_mlp::HipHandle::unique_id();
    CHECK(id.size() == 128 && id[5] == 5 && id[127] == 127);
    hip_mlp::DeviceBuffer<float> b(h);
    CHECK(b.data() == nullptr && b.size() == 0 && st.live_allocs == 0);
    b.resize(10);
    float *p = b.data();
    CHECK(p != nullptr && b.size() == 10 && st.live_allocs == 1);
    const long long allocs = st.total_allocs;
    b.resize(10); // the same size keeps the allocation: no second one, not even at the same address
    CHECK(b.data() == p && st.live_allocs == 1 && st.total_allocs == allocs);
    float src[10], dst[10];
    for (int i = 0; i < 10; ++i) src[i] = 0.5f * float(i), dst[i] = -1.0f;
    b.copy_from_host(src, 10);
    b.copy_to_host(dst, 10);
    for (int i = 0; i < 10; ++i) CHECK(dst[i] == src[i]);
    b.resize(3);
    CHECK(b.size() == 3 && st.live_allocs == 1);
    b.resize(0); // frees
    CHECK(b.data() == nullptr && b.size() == 0 && st.live_allocs == 0);
    hip_mlp::DeviceBuffer<double> c(h, 4);
    CHECK(c.size() == 4 && st.live_allocs == 1);
  }
  CHECK(st.live_allocs == 0 && st.live_ctxs == 0);
}

void test_recorder() {
  IterationRecorder<HipBackend> r;
  lbf_record v0 = r.view();
  CHECK(v0.cap == 0 && v0.size == 0);
  r.init(0); // no-op
  r.init(-3);
  CHECK(r.size() == 0 && r.view().cap == 0);
  r.init(4);
  lbf_record v = r.view();
  CHECK(v.cap == 4 && v.size == 0 && v.loss && v.grad_norm && v.time_ms);
  CHECK(v.alpha == nullptr && v.ls_trials == nullptr && v.accepted == nullptr);
  CHECK(v.loss != v.grad_norm && v.loss != v.time_ms && v.grad_norm != v.time_ms);
  // the engine writes through the view, then the owner sets the size
  for (int i = 0; i < 4; ++i) v.loss[i] = 1.0 + i, v.grad_norm[i] = 10.0 + i, v.time_ms[i] = 20.0 + i;
  r.set_size(3);
  CHECK(r.size() == 3);
  std::vector<double> l, g, t;
  r.copy_to_host(l, g);
  CHECK(l.size() == 3 && g.size() == 3 && l[2] == 3.0 && g[0] == 10.0 && g[2] == 12.0);
  r.copy_to_host(l, g, t);
  CHECK(l.size() == 3 && g.size() == 3 && t.size() == 3 && t[1] == 21.0);
  r.set_size(4); // a solver that filled the capacity
  r.copy_to_host(l, g, t);
  CHECK(l.size() == 4 && l[3] == 4.0 && g[3] == 13.0 && t[3] == 23.0);
  r.reset();
  CHECK(r.size() == 0);
  r.record(1, 5.0, 6.0, 7.0);
  r.record(-1, 9.0, 9.0);
  r.record(4, 9.0, 9.0); // outside the capacity: ignored
  CHECK(r.size() == 2);
  r.copy_to_host(l, g, t);
  CHECK(l.size() == 2 && l[1] == 5.0 && g[1] == 6.0 && t[1] == 7.0);
  r.init(2); // a new capacity clears
  CHECK(r.size() == 0 && r.view().cap == 2);
}

void test_csv() {
  IterationRecorder<HipBackend> r;
  r.init(8);
  for (int i = 0; i < 8; ++i) r.record(i, 1.5 + i, 2.5 + i, 0.25 * i);
  write_hip_history_csv("no_interval.csv", r, 0);
  write_hip_history_csv("neg_interval.csv", r, -2);
  CHECK(!exists("no_interval.csv") && !exists("neg_interval.csv"));
  IterationRecorder<HipBackend> empty;
  empty.init(8);
  write_hip_history_csv("empty.csv", empty, 1);
  CHECK(!exists("empty.csv"));
  write_hip_history_csv("every3.csv", r, 3);
  const auto v = lines("every3.csv");
  CHECK(v.size() == 4);
  CHECK(v[0] == "Iteration,Loss,GradNorm,TimeMs");
  CHECK(v[1] == "0,1.5,2.5,0");
  CHECK(v[2] == "3,4.5,5.5,0.75");
  CHECK(v[3] == "6,7.5,8.5,1.5");
  write_hip_history_csv("every1.csv", r, 1);
  CHECK(lines("every1.csv").size() == 9);
  UnifiedConfig c;
  c.name = "abc";
  CHECK(hip_log_filename(c) == "abc_history.csv");
  c.name = "";
  CHECK(hip_log_filename(c) == "run_history.csv");
}

void test_mnist_loader() {
  { // 3 images of 2 x 2, big-endian header, magic 2051
    std::ofstream f("img.idx3-ubyte", std::ios::binary);
    const unsigned char h[16] = {0, 0, 8, 3, 0, 0, 0, 3, 0, 0, 0, 2, 0, 0, 0, 2};
    const unsigned char px[12] = {0, 255, 51, 102, 1, 2, 3, 4, 250, 251, 252, 253};
    f.write(reinterpret_cast<const char *>(h), 16);
    f.write(reinterpret_cast<const char *>(px), 12);
  }
  { // 3 labels, magic 2049; a label >= 10 stays all-zero
    std::ofstream f("lab.idx1-ubyte", std::ios::binary);
    const unsigned char h[8] = {0, 0, 8, 1, 0, 0, 0, 3};
    const unsigned char lab[3] = {1, 9, 12};
    f.write(reinterpret_cast<const char *>(h), 8);
    f.write(reinterpret_cast<const char *>(lab), 3);
  }
  const unsigned char px[12] = {0, 255, 51, 102, 1, 2, 3, 4, 250, 251, 252, 253};
  HostMatrix X = hip_mlp::MNISTLoader::loadImages("img.idx3-ubyte");
  CHECK(X.rows() == 4 && X.cols() == 3); // (rows * cols) x N, one image per column
  for (int n = 0; n < 3; ++n)
    for (int p = 0; p < 4; ++p) {
      CHECK(std::fabs(X(p, n) - double(px[n * 4 + p]) / 255.0) <= 1.0 / 16777216.0); // an fp32 quotient
      CHECK(X(p, n) == double(float(X(p, n))));                                     // it came through fp32
    }
  CHECK(X(0, 0) == 0.0 && X(1, 0) == 1.0);
  HostMatrix X2 = hip_mlp::MNISTLoader::loadImages("img.idx3-ubyte", 2);
  CHECK(X2.rows() == 4 && X2.cols() == 2 && X2(3, 1) == X(3, 1));
  HostMatrix Y = hip_mlp::MNISTLoader::loadLabels("lab.idx1-ubyte");
  CHECK(Y.rows() == 10 && Y.cols() == 3);
  for (int n = 0; n < 3; ++n)
    for (int o = 0; o < 10; ++o) CHECK(Y(o, n) == ((n == 0 && o == 1) || (n == 1 && o == 9) ? 1.0 : 0.0));
  HostMatrix Y1 = hip_mlp::MNISTLoader::loadLabels("lab.idx1-ubyte", 1);
  CHECK(Y1.rows() == 10 && Y1.cols() == 1 && Y1(1, 0) == 1.0);
}

// ---- the minimizer classes -----------------------------------------------------------------------------------

struct Seen {
  const HipScalar *params = nullptr, *input = nullptr, *target = nullptr;
  HipScalar *grad = nullptr;
  int batch = -1, calls = 0;
};

void test_hip_lbfgs() {
  auto &st = fake::state();
  hip_mlp::HipHandle h;
  hip_mlp::DeviceBuffer<float> x(h, 12), in(h, 5), tg(h, 3);
  Seen seen;
  hip_mlp::HipMinimizerBase::LossGradFun fn = [&](const HipScalar *p, HipScalar *g, const HipScalar *i,
                                                  const HipScalar *t, int b) -> HipScalar {
    seen.params = p, seen.grad = g, seen.input = i, seen.target = t, seen.batch = b, ++seen.calls;
    return 1.2f; // not a double: the trampoline widens the float
  };
  st.rows_to_write = 6;
  st.iterations = 5;

  hip_mlp::HipLBFGS s(h);
  { // untouched setters: the class's own defaults (m = 16, 200 iterations, 1e-6f, 20 trials, 1e-4f, 0.5f)
    st.log.clear();
    s.solve(12, x.data(), in.data(), tg.data(), 21, fn);
    const fake::Call *c = fake::last("lbfgs_solve_fn");
    CHECK(c && c->lbfgs.m == 16 && c->lbfgs.max_iters == 200 && c->lbfgs.tol == double(1e-6f));
    CHECK(c->lbfgs.line_search == LBF_LS_ARMIJO && c->lbfgs.max_line_iters == 20);
    CHECK(c->lbfgs.c1 == double(1e-4f) && c->lbfgs.c2 == 0.9 && c->lbfgs.rho == 0.5);
    CHECK(c->rec == nullptr && c->info != nullptr);
    CHECK(s.iterations() == 5);
  }
  IterationRecorder<HipBackend> rec;
  rec.init(9);
  s.setRecorder(&rec);
  s.setMemory(5);
  s.setMaxIterations(33);
  s.setTolerance(0.015f);
  s.setLineSearchParams(17, 0.002f, 0.3f);
  { // Armijo: the setters' line-search values reach the engine
    st.log.clear();
    seen = Seen{};
    s.solve(12, x.data(), in.data(), tg.data(), 21, fn);
    CHECK(fake::count("lbfgs_solve_fn") == 1);
    const fake::Call *c = fake::last("lbfgs_solve_fn");
    CHECK(c->ctx == h.get() && c->n == 12 && c->params == x.data());
    CHECK(c->lbfgs.m == 5 && c->lbfgs.max_iters == 33 && c->lbfgs.tol == double(0.015f));
    CHECK(c->lbfgs.line_search == LBF_LS_ARMIJO && c->lbfgs.max_line_iters == 17);
    CHECK(c->lbfgs.c1 == double(0.002f) && c->lbfgs.c2 == 0.9 && c->lbfgs.rho == double(0.3f));
    // the callback got the engine's trial point and gradient buffer and the caller's data
    CHECK(seen.calls == 1 && seen.params == x.data() && seen.grad != nullptr);
    CHECK(seen.input == in.data() && seen.target == tg.data() && seen.batch == 21);
    CHECK(c->value == double(1.2f));
    // the record is the recorder's arrays, at its capacity, empty on entry
    lbf_record v = rec.view();
    CHECK(c->rec != nullptr && c->rec_loss == v.loss && c->rec_grad_norm == v.grad_norm && c->rec_time_ms == v.time_ms);
    CHECK(c->rec_cap == 9 && c->rec_size_in == 0 && c->rec_alpha == nullptr);
    CHECK(rec.size() == 6 && s.iterations() == 5);
    std::vector<double> l, g, t;
    rec.copy_to_host(l, g, t);
    CHECK(l.size() == 6 && l[0] == 100.0 && l[5] == 105.0 && g[5] == 205.0 && t[5] == 305.0);
  }
  { // Wolfe: the library's line-search defaults stay, setLineSearchParams is not applied
    st.log.clear();
    s.setLineSearch(LBF_LS_WOLFE);
    s.solve(12, x.data(), in.data(), tg.data(), 21, fn);
    const fake::Call *c = fake::last("lbfgs_solve_fn");
    CHECK(c->lbfgs.line_search == LBF_LS_WOLFE && c->lbfgs.max_line_iters == 50);
    CHECK(c->lbfgs.c1 == 1e-4 && c->lbfgs.c2 == 0.9 && c->lbfgs.rho == 0.5);
    CHECK(c->lbfgs.m == 5 && c->lbfgs.max_iters == 33 && c->lbfgs.tol == double(0.015f));
    s.setLineSearch(LBF_LS_ARMIJO);
  }
  { // fewer than one trial clamps to one
    st.log.clear();
    s.setLineSearchParams(0, 0.004f, 0.6f);
    s.solve(12, x.data(), in.data(), tg.data(), 21, fn);
    CHECK(fake::last("lbfgs_solve_fn")->lbfgs.max_line_iters == 1);
    s.setLineSearchParams(-5, 0.004f, 0.6f);
    s.solve(12, x.data(), in.data(), tg.data(), 21, fn);
    CHECK(fake::last("lbfgs_solve_fn")->lbfgs.max_line_iters == 1);
    CHECK(fake::last("lbfgs_solve_fn")->lbfgs.c1 == double(0.004f));
    CHECK(fake::last("lbfgs_solve_fn")->lbfgs.rho == double(0.6f));
  }
  { // a solver that fills the record
    st.rows_to_write = 1000;
    s.solve(12, x.data(), in.data(), tg.data(), 21, fn);
    CHECK(rec.size() == 9);
    st.rows_to_write = 6;
  }
  { // nothing to solve: no engine call, zero iterations
    st.log.clear();
    CHECK(s.iterations() == 5);
    s.solve(0, x.data(), in.data(), tg.data(), 21, fn);
    CHECK(s.iterations() == 0 && st.log.empty());
    s.solve(12, x.data(), in.data(), tg.data(), 21, fn);
    CHECK(s.iterations() == 5);
    s.solve(12, nullptr, in.data(), tg.data(), 21, fn);
    CHECK(s.iterations() == 0 && fake::count("lbfgs_solve_fn") == 1);
    s.solve(-4, x.data(), in.data(), tg.data(), 21, fn);
    CHECK(s.iterations() == 0 && fake::count("lbfgs_solve_fn") == 1);
  }
}

void build_net(hip_mlp::HipNetwork &net) {
  net.addLayer(In, Hid, hip_mlp::Tanh::id);
  net.addLayer(Hid, Out, hip_mlp::Linear::id);
}

void test_hip_hf_and_owlqn() {
  auto &st = fake::state();
  hip_mlp::HipHandle h;
  hip_mlp::HipNetwork net(h);
  build_net(net);
  net.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
  net.setL2(0.0321);
  net.bindParams(31);
  hip_mlp::DeviceBuffer<float> in(h, 8 * In), tg(h, 8 * Out), other(h, size_t(NParams));
  hip_mlp::HipMinimizerBase::LossGradFun unused;
  st.rows_to_write = 4;
  st.iterations = 3;
  IterationRecorder<HipBackend> rec;
  rec.init(6);
  {
    hip_mlp::HipHF s(h, net);
    st.log.clear();
    s.solve(int(NParams), net.params_data(), in.data(), tg.data(), 8, unused); // untouched: the class's defaults
    const fake::Call *d = fake::last("hf_solve");
    CHECK(d && d->hf.max_iters == 200 && d->hf.tol == double(1e-6f) && d->hf.cg_iters == 50 && d->hf.cg_rtol == 0.1);
    CHECK(d->hf.damping0 == 1.0 && d->hf.curv_rows == 0 && d->hf.max_line_iters == 20);
    CHECK(d->hf.c1 == double(1e-4f) && d->hf.rho == 0.5 && d->rec == nullptr);
    s.setRecorder(&rec);
    s.setMaxIterations(23);
    s.setTolerance(0.017f);
    s.setCG(13, 0.19);
    s.setDamping(2.5);
    s.setCurvatureRows(16);
    s.setLineSearchParams(9, 0.003f, 0.4f);
    st.log.clear();
    s.solve(int(NParams), other.data(), in.data(), tg.data(), 8, unused);
    CHECK(fake::count("hf_solve") == 1);
    const fake::Call *c = fake::last("hf_solve");
    CHECK(c->net == net.raw() && c->params == other.data() && c->X == in.data() && c->Y == tg.data());
    CHECK(c->n_local == 8 && c->n_global == 8);
    CHECK(c->net_loss == LBF_LOSS_SOFTMAX_XENT && c->net_l2 == 0.0321);
    CHECK(c->hf.max_iters == 23 && c->hf.tol == double(0.017f));
    CHECK(c->hf.cg_iters == 13 && c->hf.cg_rtol == 0.19 && c->hf.cg_check == 10);
    CHECK(c->hf.damping0 == 2.5 && c->hf.damp_up == 1.5 && c->hf.damp_down == 2.0 / 3.0);
    CHECK(c->hf.ratio_lo == 0.25 && c->hf.ratio_hi == 0.75);
    CHECK(c->hf.c1 == double(0.003f) && c->hf.rho == double(0.4f) && c->hf.max_line_iters == 9);
    CHECK(c->hf.curv_rows == 16);
    CHECK(c->hf.damping_trace == nullptr && c->hf.ratio_trace == nullptr && c->hf.cg_trace == nullptr);
    CHECK(c->hf.trace_cap == 0);
    CHECK(c->rec_loss == rec.view().loss && c->rec_cap == 6 && c->rec_size_in == 0);
    CHECK(rec.size() == 4 && s.iterations() == 3);
    st.log.clear();
    s.solve(0, other.data(), in.data(), tg.data(), 8, unused);
    CHECK(s.iterations() == 0 && st.log.empty());
    st.iterations = 3;
    s.solve(int(NParams), nullptr, in.data(), tg.data(), 8, unused);
    CHECK(s.iterations() == 0 && st.log.empty());
  }
  {
    hip_mlp::HipOWLQN s(h, net);
    st.owl = lbf_owlqn_stats{4, 40, 0.75, 1.5};
    st.log.clear();
    s.solve(int(NParams), net.params_data(), in.data(), tg.data(), 8, unused); // untouched: the class's defaults
    const fake::Call *d = fake::last("owlqn_solve");
    CHECK(d && d->owlqn.m == 10 && d->owlqn.max_iters == 200 && d->owlqn.tol == double(1e-6f));
    CHECK(d->owlqn.l1 == 0.0 && d->owlqn.l1_bias == 0 && d->owlqn.max_line_iters == 20);
    CHECK(d->owlqn.c1 == double(1e-4f) && d->owlqn.rho == 0.5 && d->rec == nullptr);
    s.setRecorder(&rec);
    s.setMaxIterations(27);
    s.setTolerance(0.019f);
    s.setL1(0.0047, true);
    s.setHistorySize(3);
    s.setLineSearchParams(8, 0.005f, 0.7f);
    st.owl = lbf_owlqn_stats{5, 50, 1.25, 2.5};
    st.log.clear();
    s.solve(int(NParams), other.data(), in.data(), tg.data(), 8, unused);
    CHECK(fake::count("owlqn_solve") == 1);
    const fake::Call *c = fake::last("owlqn_solve");
    CHECK(c->net == net.raw() && c->params == other.data() && c->X == in.data() && c->Y == tg.data());
    CHECK(c->n_local == 8 && c->n_global == 8);
    CHECK(c->net_loss == LBF_LOSS_SOFTMAX_XENT && c->net_l2 == 0.0321);
    CHECK(c->owlqn.m == 3 && c->owlqn.max_iters == 27 && c->owlqn.tol == double(0.019f));
    CHECK(c->owlqn.l1 == 0.0047 && c->owlqn.l1_bias == 1);
    CHECK(c->owlqn.c1 == double(0.005f) && c->owlqn.rho == double(0.7f) && c->owlqn.max_line_iters == 8);
    CHECK(c->owlqn.zeros_trace == nullptr && c->owlqn.trace_cap == 0);
    CHECK(c->stats == &s.stats());
    CHECK(s.stats().zeros == 5 && s.stats().penalised == 50 && s.stats().l1_term == 1.25 && s.stats().pg_norm == 2.5);
    CHECK(c->rec_loss == rec.view().loss && c->rec_cap == 6 && c->rec_size_in == 0);
    CHECK(rec.size() == 4 && s.iterations() == 3);
    s.setL1(0.002); // on_biases defaults to false
    s.solve(int(NParams), other.data(), in.data(), tg.data(), 8, unused);
    CHECK(fake::last("owlqn_solve")->owlqn.l1 == 0.002 && fake::last("owlqn_solve")->owlqn.l1_bias == 0);
    st.log.clear();
    s.solve(0, other.data(), in.data(), tg.data(), 8, unused);
    CHECK(s.iterations() == 0 && st.log.empty());
    s.solve(int(NParams), nullptr, in.data(), tg.data(), 8, unused);
    CHECK(s.iterations() == 0 && st.log.empty());
  }
}

// ---- HipNetwork ----------------------------------------------------------------------------------------------

void test_hip_network() {
  auto &st = fake::state();
  hip_mlp::HipHandle h;
  st.log.clear();
  {
    hip_mlp::HipNetwork net(h);
    build_net(net);
    CHECK(net.output_size() == Out && net.raw() == nullptr && net.params_size() == 0);
    CHECK(net.loss() == hip_mlp::Loss::MeanSquaredError && net.l2() == 0.0);
    CHECK(&net.handle() == &h);
    // before bindParams(): remembered, replayed when the engine's network is created
    net.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
    net.setL2(0.5);
    CHECK(st.log.empty());
    net.bindParams(); // seed 123, the CUDA stream
    CHECK(st.log.size() == 4);
    CHECK(st.log[0].fn == "mlp_create" && st.log[0].ctx == h.get());
    CHECK((st.log[0].dims == std::vector<int>{In, Hid, Out}));
    CHECK((st.log[0].acts == std::vector<int>{LBF_ACT_TANH, LBF_ACT_LINEAR}));
    CHECK(st.log[1].fn == "mlp_set_loss" && st.log[1].ivalue == LBF_LOSS_SOFTMAX_XENT);
    CHECK(st.log[2].fn == "mlp_set_l2" && st.log[2].value == 0.5);
    CHECK(st.log[3].fn == "mlp_init_params" && st.log[3].seed == 123u && st.log[3].init_mode == LBF_INIT_CUDA);
    CHECK(st.log[3].params == net.params_data() && st.log[3].net == net.raw());
    CHECK(net.params_size() == size_t(NParams) && net.grads_data() != nullptr);
    CHECK(net.grads_data() != net.params_data());
    CHECK((net.dims() == std::vector<int>{In, Hid, Out}));
    // after: at once
    net.setLoss(hip_mlp::Loss::MeanSquaredError);
    CHECK(st.log.size() == 5 && st.log[4].fn == "mlp_set_loss" && st.log[4].ivalue == LBF_LOSS_MSE);
    CHECK(net.loss() == hip_mlp::Loss::MeanSquaredError);
    net.setL2(0.25);
    CHECK(st.log.size() == 6 && st.log[5].fn == "mlp_set_l2" && st.log[5].value == 0.25 && net.l2() == 0.25);
    // a second bindParams() re-draws on the same network: no second create, loss and l2 not replayed
    net.bindParams(99, LBF_INIT_CPU);
    CHECK(st.log.size() == 7 && st.log[6].fn == "mlp_init_params" && st.log[6].seed == 99u);
    CHECK(st.log[6].init_mode == LBF_INIT_CPU && fake::count("mlp_create") == 1);

    hip_mlp::DeviceBuffer<float> x(h, 5 * In), y(h, 5 * Out), o(h, 5 * Out);
    hip_mlp::DeviceBuffer<int> pred(h, 5);
    // compute_loss_and_grad: the network's own buffers, the mean (1 / batch), no l2 and no gather
    st.loss_grad_value = 2.75;
    const HipScalar lv = net.compute_loss_and_grad(x.data(), y.data(), 5);
    const fake::Call *c = fake::last("mlp_loss_grad");
    CHECK(lv == 2.75f && c && c->net == net.raw() && c->params == net.params_data() && c->grad == net.grads_data());
    CHECK(c->X == x.data() && c->Y == y.data() && c->idx == nullptr && c->batch == 5);
    CHECK(c->inv_scale == 1.0 / 5 && c->l2_arg == 0.0);
    // forward_only
    st.forward_tables[5] = std::vector<float>(5 * Out, 0.5f);
    net.forward_only(x.data(), 5, o.data());
    c = fake::last("mlp_forward");
    CHECK(c && c->params == net.params_data() && c->X == x.data() && c->batch == 5 && c->out == o.data());
    float back[5 * Out];
    o.copy_to_host(back, 5 * Out);
    CHECK(back[0] == 0.5f && back[5 * Out - 1] == 0.5f);
    // evaluate: inv_scale 1 and the loss divided by the rows the engine counted
    st.eval = lbf_eval_result{10.5, 7, 5, 6, 0, 0};
    std::vector<long long> conf(2, 99); // a wrong size holding garbage: resized to Out * Out and zeroed
    hip_mlp::EvalResult e = net.evaluate(x.data(), y.data(), 5, 2, &conf, pred.data());
    c = fake::last("mlp_evaluate");
    CHECK(c && c->net == net.raw() && c->params == net.params_data() && c->X == x.data() && c->Y == y.data());
    CHECK(c->idx == nullptr && c->batch == 5 && c->inv_scale == 1.0 && c->k == 2 && c->chunk_rows == 0);
    CHECK(c->confusion == conf.data() && c->confusion_zeroed && c->pred == pred.data() && c->proba == nullptr);
    CHECK(conf.size() == size_t(Out * Out) && conf[0] == 1 && conf[Out * Out - 1] == Out * Out);
    CHECK(e.loss == 10.5 * (1.0 / 7.0) && e.rows == 7 && e.correct == 5 && e.topk == 6 && e.k == 2);
    CHECK(e.accuracy() == 5.0 / 7.0 && e.topk_accuracy() == 6.0 / 7.0);
    // defaults: k = 1, no confusion, no predictions
    e = net.evaluate(x.data(), y.data(), 5);
    c = fake::last("mlp_evaluate");
    CHECK(c->k == 1 && c->confusion == nullptr && c->pred == nullptr && e.k == 1);
    // an empty total: zero loss, no division by zero
    st.eval = lbf_eval_result{3.0, 0, 0, 0, 0, 0};
    e = net.evaluate(x.data(), y.data(), 0);
    CHECK(e.loss == 0.0 && e.rows == 0 && e.accuracy() == 0.0 && e.topk_accuracy() == 0.0);
    CHECK(st.live_nets == 1);
  }
  CHECK(st.live_nets == 0 && st.live_allocs == 0);
}

// ---- the launcher and the Unified* strategies ----------------------------------------------------------------

template <class L> void add_layers(L &l) {
  l.template addLayer<In, Hid, hip_mlp::Tanh>();
  l.template addLayer<Hid, Out, hip_mlp::Linear>();
}

// what every Unified* strategy must hand its solver besides the parameter struct
void check_unified_call(const fake::Call *c, UnifiedLauncher<HipBackend> &l, UnifiedOptimizer<HipBackend> &opt,
                        int cap) {
  auto &net = l.getWrapper().getInternal();
  CHECK(c && c->net == net.raw() && c->params == net.params_data());
  CHECK(c->X != nullptr && c->Y != nullptr && c->X != c->Y);
  CHECK(c->n_local == NTrain && c->n_global == NTrain); // train_x.cols()
  lbf_record v = opt.recorder.view();
  CHECK(c->rec_loss == v.loss && c->rec_grad_norm == v.grad_norm && c->rec_time_ms == v.time_ms);
  CHECK(c->rec_cap == cap && c->rec_size_in == 0 && c->info != nullptr);
}

void test_unified_strategies() {
  auto &st = fake::state();
  st.forward_tables[NTrain] = std::vector<float>(NTrain * Out, 0.25f);
  st.forward_tables[NTest] = std::vector<float>(NTest * Out, 0.25f);
  UnifiedLauncher<HipBackend> l;
  add_layers(l);
  l.buildNetwork();
  const UnifiedDataset d = dataset();
  l.setData(d);
  auto &net = l.getWrapper().getInternal();
  CHECK(l.getWrapper().getParamsSize() == size_t(NParams));
  const UnifiedConfig cfg = distinct_config();
  st.rows_to_write = 9;
  st.iterations = 9;

  { // the upload: fp32 rows of In / Out floats per sample == the column-major matrix
    UnifiedGD_HIP o;
    st.log.clear();
    l.train(o, cfg);
    const fake::Call *c = fake::last("gd_solve");
    const float *x = static_cast<const float *>(c->X);
    for (long i = 0; i < d.train_x.size(); ++i) CHECK(x[i] == float(d.train_x.data()[i]));
    const float *y = static_cast<const float *>(c->Y);
    for (long i = 0; i < d.train_y.size(); ++i) CHECK(y[i] == float(d.train_y.data()[i]));
  }
  {
    UnifiedLBFGS_HIP o; // Armijo unless told otherwise
    st.log.clear();
    l.train(o, cfg);
    CHECK(fake::count("lbfgs_solve") == 1);
    const fake::Call *c = fake::last("lbfgs_solve");
    check_unified_call(c, l, o, cfg.max_iters);
    CHECK(c->lbfgs.m == 7 && c->lbfgs.max_iters == 11 && c->lbfgs.tol == 0.0625);
    CHECK(c->lbfgs.line_search == LBF_LS_ARMIJO && c->lbfgs.max_line_iters == 20);
    CHECK(c->lbfgs.c1 == 1e-4 && c->lbfgs.c2 == 0.9 && c->lbfgs.rho == 0.5);
    CHECK(o.recorder.size() == 9);
    o.line_search = LBF_LS_WOLFE;
    l.train(o, cfg);
    c = fake::last("lbfgs_solve");
    CHECK(c->lbfgs.line_search == LBF_LS_WOLFE && c->lbfgs.max_line_iters == 50 && c->lbfgs.m == 7);
    CHECK(c->lbfgs.max_iters == 11 && c->lbfgs.tol == 0.0625);
    UnifiedConfig c0 = cfg; // m_param <= 0 gives 10
    c0.m_param = 0;
    l.train(o, c0);
    CHECK(fake::last("lbfgs_solve")->lbfgs.m == 10);
    c0.m_param = -3;
    l.train(o, c0);
    CHECK(fake::last("lbfgs_solve")->lbfgs.m == 10);
  }
  {
    UnifiedSLBFGS_HIP o;
    st.log.clear();
    l.train(o, cfg);
    CHECK(fake::count("slbfgs_solve") == 1);
    const fake::Call *c = fake::last("slbfgs_solve");
    check_unified_call(c, l, o, cfg.max_iters);
    CHECK(c->slbfgs.max_epochs == 11 && c->slbfgs.tol == 0.0625);
    CHECK(c->slbfgs.M == 7 && c->slbfgs.L == 5 && c->slbfgs.b == 14 && c->slbfgs.b_H == 9);
    CHECK(c->slbfgs.step == 0.03125 && c->slbfgs.hvp_exact == LBF_HVP_GAUSS_NEWTON);
    CHECK(c->slbfgs.lambda == 1e-4 && c->slbfgs.seed == 123u && c->slbfgs.fd_eps == 1e-4); // the library's
    CHECK(c->slbfgs.pair_trace == nullptr && c->slbfgs.pair_trace_cap == 0);
    CHECK(c->slbfgs.dp_mode == LBF_SLBFGS_DP_REPLICATED);
    UnifiedConfig c0 = cfg; // b_H_param <= 0 gives batch_size / 2
    c0.b_H_param = 0;
    c0.curvature = LBF_HVP_EXACT;
    l.train(o, c0);
    CHECK(fake::last("slbfgs_solve")->slbfgs.b_H == 7 && fake::last("slbfgs_solve")->slbfgs.hvp_exact == LBF_HVP_EXACT);
    c0.b_H_param = -1;
    c0.batch_size = 31;
    c0.curvature = LBF_HVP_FD;
    l.train(o, c0);
    CHECK(fake::last("slbfgs_solve")->slbfgs.b_H == 15 && fake::last("slbfgs_solve")->slbfgs.b == 31);
    CHECK(fake::last("slbfgs_solve")->slbfgs.hvp_exact == LBF_HVP_FD);
  }
  {
    UnifiedGD_HIP o;
    st.log.clear();
    l.train(o, cfg);
    CHECK(fake::count("gd_solve") == 1);
    const fake::Call *c = fake::last("gd_solve");
    check_unified_call(c, l, o, cfg.max_iters);
    CHECK(c->gd.lr == 0.03125 && c->gd.momentum == 0.71 && c->gd.max_iters == 11 && c->gd.tol == 0.0625);
  }
  {
    UnifiedSGD_HIP o;
    st.log.clear();
    st.rows_to_write = 1000; // the initial record and one per epoch fill the capacity
    l.train(o, cfg);
    st.rows_to_write = 9;
    CHECK(fake::count("sgd_solve") == 1);
    const fake::Call *c = fake::last("sgd_solve");
    check_unified_call(c, l, o, cfg.max_iters + 1);
    CHECK(c->sgd.lr == 0.03125 && c->sgd.momentum == 0.71 && c->sgd.batch == 14);
    CHECK(c->sgd.decay_rate == 0.37 && c->sgd.decay_step == 3 && c->sgd.max_epochs == 11);
    CHECK(c->sgd.tol == 1e-6); // SGD keeps its own tolerance
    CHECK(o.recorder.size() == cfg.max_iters + 1);
    std::vector<double> lo, g, t;
    o.recorder.copy_to_host(lo, g, t);
    CHECK(lo.size() == 12 && lo[11] == 111.0 && g[11] == 211.0 && t[11] == 311.0);
  }
  {
    UnifiedHF_HIP o;
    st.log.clear();
    l.train(o, cfg);
    CHECK(fake::count("hf_solve") == 1);
    const fake::Call *c = fake::last("hf_solve");
    check_unified_call(c, l, o, cfg.max_iters);
    CHECK(c->hf.max_iters == 11 && c->hf.tol == 0.0625);
    CHECK(c->hf.cg_iters == 13 && c->hf.cg_rtol == 0.19 && c->hf.cg_check == 10);
    CHECK(c->hf.damping0 == 2.5 && c->hf.damp_up == 1.5 && c->hf.damp_down == 2.0 / 3.0);
    CHECK(c->hf.ratio_lo == 0.25 && c->hf.ratio_hi == 0.75);
    CHECK(c->hf.c1 == 1e-4 && c->hf.rho == 0.5 && c->hf.max_line_iters == 20 && c->hf.curv_rows == 0);
    CHECK(c->hf.damping_trace == nullptr && c->hf.ratio_trace == nullptr && c->hf.cg_trace == nullptr);
    CHECK(c->hf.trace_cap == 0);
  }
  {
    UnifiedOWLQN_HIP o;
    st.owl = lbf_owlqn_stats{6, 60, 1.75, 3.5};
    st.log.clear();
    l.train(o, cfg);
    CHECK(fake::count("owlqn_solve") == 1);
    const fake::Call *c = fake::last("owlqn_solve");
    check_unified_call(c, l, o, cfg.max_iters);
    CHECK(c->owlqn.m == 7 && c->owlqn.max_iters == 11 && c->owlqn.tol == 0.0625);
    CHECK(c->owlqn.l1 == 0.0047 && c->owlqn.l1_bias == 0);
    CHECK(c->owlqn.c1 == 1e-4 && c->owlqn.rho == 0.5 && c->owlqn.max_line_iters == 20);
    CHECK(c->owlqn.zeros_trace == nullptr && c->owlqn.trace_cap == 0);
    CHECK(c->stats == &o.stats);
    CHECK(o.stats.zeros == 6 && o.stats.penalised == 60 && o.stats.l1_term == 1.75 && o.stats.pg_norm == 3.5);
  }
  { // the history file: named after the config, every log_interval-th row
    CHECK(exists("cfgname_history.csv"));
    const auto v = lines("cfgname_history.csv");
    CHECK(v.size() == 4 && v[0] == "Iteration,Loss,GradNorm,TimeMs"); // rows 0, 4, 8 of 9
    CHECK(v[1] == "0,100,200,300" && v[2] == "4,104,204,304" && v[3] == "8,108,208,308");
    UnifiedConfig c0 = cfg;
    c0.name = "";
    UnifiedGD_HIP o;
    l.train(o, c0);
    CHECK(exists("run_history.csv"));
    c0.name = "silent";
    c0.log_interval = 0;
    l.train(o, c0);
    CHECK(!exists("silent_history.csv"));
  }
  (void)net;
}

void test_launcher_sequencing() {
  auto &st = fake::state();
  st.forward_tables[NTrain] = std::vector<float>(NTrain * Out, 0.25f);
  st.forward_tables[NTest] = std::vector<float>(NTest * Out, 0.25f);
  st.rows_to_write = 2;
  st.log.clear();
  UnifiedLauncher<HipBackend> l;
  add_layers(l);
  // before buildNetwork(): replayed at creation
  l.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
  l.setL2(0.5);
  CHECK(st.log.empty());
  l.buildNetwork();
  CHECK(st.log.size() == 4 && st.log[0].fn == "mlp_create");
  CHECK(st.log[1].fn == "mlp_set_loss" && st.log[1].ivalue == LBF_LOSS_SOFTMAX_XENT);
  CHECK(st.log[2].fn == "mlp_set_l2" && st.log[2].value == 0.5);
  CHECK(st.log[3].fn == "mlp_init_params" && st.log[3].seed == 123u && st.log[3].init_mode == LBF_INIT_CUDA);
  // after: at once
  l.setLoss(hip_mlp::Loss::MeanSquaredError);
  CHECK(st.log.size() == 5 && st.log[4].fn == "mlp_set_loss" && st.log[4].ivalue == LBF_LOSS_MSE);
  l.setL2(0.0);
  CHECK(st.log.size() == 6 && st.log[5].fn == "mlp_set_l2" && st.log[5].value == 0.0);
  l.setData(dataset());

  UnifiedConfig cfg = distinct_config();
  cfg.log_interval = 0;
  UnifiedGD_HIP o;
  st.log.clear();
  l.train(o, cfg);
  // config.l2, then the re-draw with config.seed, then the solve, then the host scan's forward pass
  CHECK(st.log.size() == 4);
  CHECK(st.log[0].fn == "mlp_set_l2" && st.log[0].value == 0.0123);
  CHECK(st.log[1].fn == "mlp_init_params" && st.log[1].seed == 777u && st.log[1].init_mode == LBF_INIT_CUDA);
  CHECK(st.log[1].params == l.getWrapper().getInternal().params_data());
  CHECK(st.log[2].fn == "gd_solve" && st.log[2].net_l2 == 0.0123 && st.log[2].net_loss == LBF_LOSS_MSE);
  CHECK(st.log[3].fn == "mlp_forward" && st.log[3].batch == NTrain && st.log[3].X == st.log[2].X);
  CHECK(st.log[3].params == st.log[2].params);

  // l2 = 0 in a later config does not clear the network's l2 (documented; unified.py does the same), and
  // reset_params = false draws nothing
  cfg.l2 = 0.0;
  cfg.reset_params = false;
  st.log.clear();
  l.train(o, cfg);
  CHECK(st.log.size() == 2 && st.log[0].fn == "gd_solve" && st.log[0].net_l2 == 0.0123);
  CHECK(fake::count("mlp_init_params") == 0 && fake::count("mlp_set_l2") == 0);
  CHECK(l.getWrapper().getInternal().l2() == 0.0123);
  // test(): the other split's inputs
  st.log.clear();
  l.test();
  CHECK(st.log.size() == 1 && st.log[0].fn == "mlp_forward" && st.log[0].batch == NTest);
}

// ---- the host scan, through train() / test() / lastTrain() / lastTest() ----------------------------------------

void test_host_scan() {
  auto &st = fake::state();
  // Outputs and targets are halves and quarters: every squared difference and their sum are exact in double.
  const float Z[NTrain * Out] = {
      0.5f,  0.5f,   0.25f, // a tie: index 0 wins          target 0 -> correct
      0.25f, 0.75f,  0.75f, // a tie of 1 and 2: 1 wins     target 1 -> correct
      -1.5f, -0.25f, -2.0f, // all negative: 1              target 1 -> correct
      2.0f,  1.75f,  -0.5f, //                              target 0 (a soft row, tie of targets 0 and 1)
      0.0f,  0.0f,   0.0f,  // all equal: 0                 target 1 -> wrong
      1.25f, -3.0f,  1.5f,  // 2                            target 2 -> correct
      0.75f, 1.0f,   0.5f,  // 1                            target 1 -> correct
  };
  const double Y[NTrain * Out] = {1, 0, 0, 0, 1, 0, 0, 1, 0, 0.5, 0.5, 0, 0, 1, 0, 0, 0, 1, 0.25, 0.5, 0.25};
  // the test split: a NaN never wins, and a row with nothing above -1e20 gives class 0
  const float qnan = std::numeric_limits<float>::quiet_NaN();
  const float ZT[NTest * Out] = {
      qnan,  0.25f, 0.5f,    // 2          target 2 -> correct
      0.5f,  qnan,  0.25f,   // 0          target 1 -> wrong
      -2e20f, -3e20f, -1.5e20f, // nothing above -1e20: 0   target 0 -> correct
      qnan,  qnan,  qnan,    // 0          target 2 -> wrong
  };
  const double YT[NTest * Out] = {0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 1};

  UnifiedDataset d = dataset();
  for (int i = 0; i < NTrain; ++i)
    for (int o = 0; o < Out; ++o) d.train_y(o, i) = Y[o + i * Out];
  for (int i = 0; i < NTest; ++i)
    for (int o = 0; o < Out; ++o) d.test_y(o, i) = YT[o + i * Out];
  st.forward_tables[NTrain] = std::vector<float>(Z, Z + NTrain * Out);
  st.forward_tables[NTest] = std::vector<float>(ZT, ZT + NTest * Out);
  const std::vector<double> yv(Y, Y + NTrain * Out), ytv(YT, YT + NTest * Out);

  UnifiedLauncher<HipBackend> l;
  add_layers(l);
  l.buildNetwork();
  l.setData(d);
  CHECK(l.lastTrain() == std::make_pair(0.0, 0.0) && l.lastTest() == std::make_pair(0.0, 0.0));
  UnifiedConfig cfg;
  cfg.log_interval = 0;
  UnifiedGD_HIP o;
  st.rows_to_write = 1;

  { // MSE: the mean per element. The reference's sum is exact in long double and in double alike (dyadic
    // entries), so the one rounding left is the division, done here in double as well: no tolerance.
    l.train(o, cfg);
    const ScanRef r = scan_reference(st.forward_tables[NTrain], yv, NTrain, false);
    CHECK(r.correct == 6);
    CHECK((long double)double(r.loss_sum) == r.loss_sum);
    CHECK(l.lastTrain().first == double(r.loss_sum) / double(NTrain * Out));
    CHECK(l.lastTrain().second == double(r.correct) / double(NTrain) * 100.0);
    CHECK(l.lastTest() == std::make_pair(0.0, 0.0)); // train() leaves the test pair alone
    l.test();
    const ScanRef t = scan_reference(st.forward_tables[NTest], ytv, NTest, false);
    CHECK(t.correct == 2 && std::isnan(double(t.loss_sum)));
    CHECK(std::isnan(l.lastTest().first) && l.lastTest().second == 50.0);
  }
  { // cross-entropy: the mean per sample of sum_o y (lse - z)
    l.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
    l.train(o, cfg);
    const ScanRef r = scan_reference(st.forward_tables[NTrain], yv, NTrain, true);
    const double ref = double(r.loss_sum / (long double)NTrain);
    // double against long double: per sample, exp and log are each within 1 ulp (glibc), and the Out additions of
    // the sum, the addition of the maximum, and the Out subtractions, products and additions of the target sum
    // round to half an ulp each, all of quantities no larger than (|lse| + max |z|) sum_o y; the batch sum adds
    // half an ulp per sample of a running sum below batch times that, and the mean divides it out again.
    const double bound = double(4 * Out + 4 + NTrain) * DBL_EPSILON * double(r.scale);
    std::printf("host scan cross-entropy: %.17g, long double %.17g, |diff| %.3g, bound %.3g\n", l.lastTrain().first,
                ref, std::fabs(l.lastTrain().first - ref), bound);
    CHECK(ref > 0.5 && std::fabs(l.lastTrain().first - ref) <= bound);
    CHECK(l.lastTrain().second == double(r.correct) / double(NTrain) * 100.0 && r.correct == 6);
    l.test();
    CHECK(std::isnan(l.lastTest().first) && l.lastTest().second == 50.0);
  }
}

void test_metrics() {
  auto &st = fake::state();
  st.forward_tables[NTrain] = std::vector<float>(NTrain * Out, 0.25f);
  {
    UnifiedLauncher<HipBackend> l;
    add_layers(l);
    l.buildNetwork();
    l.setData(dataset());
    UnifiedGD_HIP o;
    UnifiedConfig cfg;
    cfg.log_interval = 0;
    l.train(o, cfg);
    const fake::Call *gd = fake::last("gd_solve");
    const void *train_x = gd->X, *train_y = gd->Y;
    auto &net = l.getWrapper().getInternal();

    st.eval = lbf_eval_result{21.0, NTrain, 3, 5, 0, 0};
    std::vector<long long> conf;
    st.log.clear();
    hip_mlp::EvalResult e = l.metrics(false, 2, &conf);
    CHECK(st.log.size() == 1);
    const fake::Call *c = fake::last("mlp_evaluate");
    CHECK(c && c->net == net.raw() && c->params == net.params_data() && c->X == train_x && c->Y == train_y);
    CHECK(c->idx == nullptr && c->batch == NTrain && c->inv_scale == 1.0 && c->k == 2 && c->chunk_rows == 0);
    CHECK(c->confusion == conf.data() && c->confusion_zeroed && conf.size() == size_t(Out * Out));
    CHECK(c->pred == nullptr && c->proba == nullptr);
    CHECK(e.loss == 21.0 * (1.0 / double(NTrain)) && e.rows == NTrain && e.correct == 3 && e.topk == 5 && e.k == 2);

    st.eval = lbf_eval_result{6.0, NTest, 1, 1, 0, 0};
    e = l.metrics(true);
    c = fake::last("mlp_evaluate");
    CHECK(c->X != train_x && c->Y != train_y && c->X != nullptr && c->Y != nullptr);
    CHECK(c->batch == NTest && c->k == 1 && c->confusion == nullptr && c->inv_scale == 1.0);
    CHECK(e.loss == 6.0 * (1.0 / double(NTest)) && e.rows == NTest && e.accuracy() == 0.25);
  }
  { // an empty split: a zero result and no engine call (the host scan returns zeros too)
    UnifiedLauncher<HipBackend> l;
    add_layers(l);
    l.buildNetwork();
    l.setData(dataset(NTrain, 0));
    st.log.clear();
    std::vector<long long> conf;
    hip_mlp::EvalResult e = l.metrics(true, 1, &conf);
    CHECK(st.log.empty() && e.loss == 0.0 && e.rows == 0 && e.correct == 0 && e.topk == 0 && e.accuracy() == 0.0);
    l.test();
    CHECK(st.log.empty() && l.lastTest() == std::make_pair(0.0, 0.0));
  }
}

} // namespace

int main(int argc, char **argv) {
  if (argc < 2 || chdir(argv[1]) != 0) {
    std::fprintf(stderr, "usage: dropin_harness <work dir> [abort_l2]\n");
    return 2;
  }
  if (argc > 2 && std::string(argv[2]) == "abort_l2") {
    hip_mlp::HipHandle h;
    hip_mlp::HipNetwork net(h);
    net.setL2(-1.0); // hip_check aborts: the process dies here
    std::printf("setL2(-1) returned\n");
    return 0;
  }
  test_host_matrix();
  test_device_buffer_and_handle();
  test_recorder();
  test_csv();
  test_mnist_loader();
  test_hip_lbfgs();
  test_hip_hf_and_owlqn();
  test_hip_network();
  test_unified_strategies();
  test_launcher_sequencing();
  test_host_scan();
  test_metrics();
  // every object above is gone: nothing of the fake's is left alive
  CHECK(fake::state().live_allocs == 0 && fake::state().live_nets == 0 && fake::state().live_ctxs == 0);
  std::printf("dropin harness ok\n");
  return 0;
}
