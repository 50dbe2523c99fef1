// Adam through the C++ drop-in header: HipAdam and UnifiedAdam_HIP on one small problem, the results dumped as raw
// arrays so that tests/test_gpu_adam.py can repeat both runs through the ctypes wrappers and compare bit for bit.
// Plain C++17, links liblbfgs_amd_abi3.so.
//   usage: adam_hip <dir>
// <dir> holds fp32 row-major X.f32 [257][64] and Y.f32 [257][10] (one-hot). Network [64, 32, 10] relu / linear,
// softmax cross-entropy, l2 = 1e-3, bindParams(19).
//   HipAdam: lr 2e-3, weight decay 1e-2, clip 0.5, batch 16, shuffle seed 7, 3 epochs, tolerance 0. Writes
//     <dir>/params.f32 (the final parameters), loss.f64 (the recorder's losses), trace.f64 (the batch objectives)
//     and iterations.txt.
//   UnifiedAdam_HIP: the config's learning_rate 1e-3, batch_size 32, max_iters 2, seed 5. Writes
//     <dir>/u_params.f32, u_loss.f64 and u_trace.f64.
#include "lbfgs_amd/hip_backend.hpp"

#include <cstdio>
#include <string>
#include <vector>

using hip_mlp::HipScalar;

namespace {

constexpr int In = 64, Hid = 32, Out = 10, N = 257;
std::string g_dir;

std::vector<float> read_f32(const std::string &name, size_t count) {
  std::vector<float> v(count);
  std::FILE *f = std::fopen((g_dir + "/" + name).c_str(), "rb");
  if (!f || std::fread(v.data(), sizeof(float), count, f) != count) {
    std::cerr << "cannot read " << count << " floats from " << name << std::endl;
    std::exit(2);
  }
  std::fclose(f);
  return v;
}

void write_raw(const std::string &name, const void *p, size_t bytes) {
  std::FILE *f = std::fopen((g_dir + "/" + name).c_str(), "wb");
  if (!f || (bytes && std::fwrite(p, 1, bytes, f) != bytes)) {
    std::cerr << "cannot write " << name << std::endl;
    std::exit(2);
  }
  std::fclose(f);
}

void write_params(hip_mlp::HipHandle &h, hip_mlp::HipNetwork &net, const std::string &name) {
  std::vector<float> host(net.params_size());
  hip_mlp::hip_check(lbf_memcpy(h.get(), host.data(), net.params_data(), host.size() * sizeof(float), 1), "lbf_memcpy");
  write_raw(name, host.data(), host.size() * sizeof(float));
}

} // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::cerr << "usage: adam_hip <dir>" << std::endl;
    return 2;
  }
  g_dir = argv[1];
  const std::vector<float> xv = read_f32("X.f32", size_t(N) * In), yv = read_f32("Y.f32", size_t(N) * Out);
  {
    hip_mlp::HipHandle h;
    hip_mlp::HipNetwork net(h);
    net.addLayer(In, Hid, hip_mlp::ReLU::id);
    net.addLayer(Hid, Out, hip_mlp::Linear::id);
    net.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
    net.setL2(1e-3);
    net.bindParams(19u);
    hip_mlp::DeviceBuffer<HipScalar> x(h, xv.size()), y(h, yv.size());
    x.copy_from_host(xv.data(), xv.size());
    y.copy_from_host(yv.data(), yv.size());

    hip_mlp::HipAdam s(h, net);
    IterationRecorder<HipBackend> rec;
    rec.init(4);
    s.setRecorder(&rec);
    s.setMaxIterations(3);
    s.setTolerance(0.0f);
    s.setLearningRate(2e-3);
    s.setWeightDecay(1e-2);
    s.setClipNorm(0.5);
    s.setBatchSize(16);
    s.setShuffle(true, 7u);
    s.solve(int(net.params_size()), net.params_data(), x.data(), y.data(), N, {});

    write_params(h, net, "params.f32");
    std::vector<double> l, g;
    rec.copy_to_host(l, g);
    write_raw("loss.f64", l.data(), l.size() * sizeof(double));
    write_raw("trace.f64", s.lossTrace().data(), s.lossTrace().size() * sizeof(double));
    std::FILE *f = std::fopen((g_dir + "/iterations.txt").c_str(), "w");
    if (!f) return 2;
    std::fprintf(f, "%d\n", s.iterations());
    std::fclose(f);
  }
  {
    UnifiedLauncher<HipBackend> launcher;
    launcher.addLayer<In, Hid, hip_mlp::ReLU>();
    launcher.addLayer<Hid, Out, hip_mlp::Linear>();
    launcher.buildNetwork();
    launcher.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
    UnifiedDataset data;
    data.train_x = hip_mlp::HostMatrix(In, N);
    data.train_y = hip_mlp::HostMatrix(Out, N);
    for (size_t i = 0; i < xv.size(); ++i) data.train_x.data()[i] = xv[i];
    for (size_t i = 0; i < yv.size(); ++i) data.train_y.data()[i] = yv[i];
    launcher.setData(data);
    UnifiedConfig cfg;
    cfg.name = g_dir + "/HIP_ADAM";
    cfg.max_iters = 2;
    cfg.learning_rate = 1e-3;
    cfg.batch_size = 32;
    cfg.seed = 5u;
    cfg.log_interval = 1;
    UnifiedAdam_HIP opt;
    launcher.train(opt, cfg);
    auto &net = launcher.getWrapper().getInternal();
    hip_mlp::HipHandle h; // lbf_memcpy needs a context on the device; any will do for a synchronous copy
    write_params(h, net, "u_params.f32");
    std::vector<double> l, g;
    opt.recorder.copy_to_host(l, g);
    write_raw("u_loss.f64", l.data(), l.size() * sizeof(double));
    write_raw("u_trace.f64", opt.trace.data(), opt.trace.size() * sizeof(double));
  }
  std::printf("[RESULT] ok\n");
  return 0;
}
