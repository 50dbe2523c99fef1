"""Compile check of the drop-in header's reference mode (include/lbfgs_amd/hip_backend.hpp with
LBF_USE_REFERENCE_UNIFIED_TYPES), next to the reference's own headers. Build container only: it reads
/root/reference at test time (-I on its src/ directory); nothing of it is copied into the repo.

What this checks: a translation unit that includes the reference's src/iteration_recorder.hpp (the
primary template IterationRecorder<Backend> and its CpuBackend specialization, Eigen-free) and then
hip_backend.hpp in reference mode compiles with g++ (C++17) and instantiates every HipBackend class a
reference driver uses (UnifiedLauncher<HipBackend>::setData / train / test, UnifiedLBFGS_HIP,
UnifiedSLBFGS_HIP, UnifiedGD_HIP, UnifiedSGD_HIP, the recorder and its CSV writer) — i.e. our forward
declarations and specializations coexist with the reference's templates — and that a strategy subclass written
against the reference's optimize parameter list (unified_optimization.hpp:433-438, const UnifiedDataset &host_data)
overrides UnifiedOptimizer<HipBackend>::optimize.

What it cannot check: the reference's UnifiedConfig / UnifiedDataset live in src/unified_optimization.hpp,
which needs Eigen3 (absent from this image). The TU therefore declares those two structs
itself with the reference's field names (unified_optimization.hpp:26-59) and a column-major matrix type
with Eigen::MatrixXd's rows() / cols() / data(); no Eigen stand-in is written.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = "/root/reference/src"

TU = r"""
#include "iteration_recorder.hpp"  // the reference's (REF_SRC on -I)

#include <string>
#include <vector>

// The reference's UnifiedConfig / UnifiedDataset (unified_optimization.hpp:26-59) need Eigen: the
// test declares them with the same fields and an Eigen-shaped column-major matrix.
struct TestMatrix {
  long r = 0, c = 0;
  std::vector<double> v;
  long rows() const { return r; }
  long cols() const { return c; }
  const double *data() const { return v.data(); }
};
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
};
struct UnifiedDataset {
  TestMatrix train_x, train_y, test_x, test_y;
};

#define LBF_USE_REFERENCE_UNIFIED_TYPES
#include "lbfgs_amd/hip_backend.hpp"

// the shape of tests/fashion-mnist/main_gpu_deep.cpp, not run (no GPU here): instantiation only
int drive(const UnifiedDataset &d) {
  UnifiedLauncher<HipBackend> launcher;
  launcher.addLayer<784, 256, hip_mlp::ReLU>();
  launcher.addLayer<256, 128, hip_mlp::ReLU>();
  launcher.addLayer<128, 64, hip_mlp::ReLU>();
  launcher.addLayer<64, 10, hip_mlp::Linear>();
  launcher.buildNetwork();
  launcher.setData(d);
  UnifiedConfig cfg;
  cfg.m_param = 100;
  UnifiedLBFGS_HIP lbfgs;
  launcher.train(lbfgs, cfg);
  launcher.test();
  UnifiedSLBFGS_HIP slbfgs;
  launcher.train(slbfgs, cfg);
  UnifiedGD_HIP gd;
  launcher.train(gd, cfg);
  UnifiedSGD_HIP sgd;
  launcher.train(sgd, cfg);
  IterationRecorder<CpuBackend> cpu_rec; // the reference's own specialization, same TU
  cpu_rec.init(4);
  return int(lbfgs.recorder.size());
}

// A strategy written against the reference's UnifiedOptimizer<CudaBackend>::optimize parameter list
// (unified_optimization.hpp:433-438: handle, net, const UnifiedDataset &host_data, d_train_x, d_train_y,
// config) with the backend's type names substituted: `override` makes the compiler prove it overrides ours.
class MyStrategy : public UnifiedOptimizer<HipBackend> {
public:
  long seen = 0;
  void optimize(hip_mlp::HipHandle &handle, NetworkWrapper<HipBackend> &net, const UnifiedDataset &host_data,
                hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &d_train_x, hip_mlp::DeviceBuffer<hip_mlp::HipScalar> &d_train_y,
                const UnifiedConfig &config) override {
    (void)handle, (void)net, (void)d_train_x, (void)d_train_y, (void)config;
    seen = long(host_data.train_x.cols());
  }
};
long drive_custom(const UnifiedDataset &d) {
  UnifiedLauncher<HipBackend> launcher;
  launcher.addLayer<784, 10, hip_mlp::Linear>();
  launcher.buildNetwork();
  launcher.setData(d);
  MyStrategy st;
  UnifiedConfig cfg;
  launcher.train(st, cfg);
  return st.seen;
}
"""


@pytest.mark.skipif(not os.path.isdir(REF_SRC), reason="reference tree not present (build container only)")
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_hip_backend_reference_mode_compiles(tmp_path):
    src = tmp_path / "dropin_tu.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-variable",
                        f"-I{REF_SRC}", f"-I{os.path.join(ROOT, 'include')}", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_hip_backend_standalone_compiles(tmp_path):
    """The standalone mode (own UnifiedConfig / UnifiedDataset / HostMatrix), no reference headers."""
    src = tmp_path / "standalone_tu.cpp"
    src.write_text('#include "lbfgs_amd/hip_backend.hpp"\n'
                   "int drive(const UnifiedDataset &d) { UnifiedLauncher<HipBackend> l; l.setData(d);\n"
                   "  UnifiedConfig c; UnifiedLBFGS_HIP o; l.train(o, c); l.test(); return 0; }\n"
                   "struct S : UnifiedOptimizer<HipBackend> { void optimize(hip_mlp::HipHandle &, "
                   "NetworkWrapper<HipBackend> &, const UnifiedDataset &d, hip_mlp::DeviceBuffer<float> &, "
                   "hip_mlp::DeviceBuffer<float> &, const UnifiedConfig &) override { (void)d.train_x.cols(); } };\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", f"-I{os.path.join(ROOT, 'include')}",
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
@pytest.mark.parametrize("driver", ["main_hip.cpp", "known_answer_hip.cpp", "parity_hip.cpp"])
def test_drivers_compile(driver):
    """The drivers over the standalone header (parity_hip.cpp: the HF / OWL-QN / metrics / cross-entropy calls),
    checked where there is no GPU to run them on."""
    src = os.path.join(ROOT, "lbfgs-ffnn_amd", "drivers", driver)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", f"-I{os.path.join(ROOT, 'include')}", src],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-4000:]
