// Preconditioned Hessian-free through the C++ drop-in header: HipHFPreconditioned and HipNetwork::gradSq on one
// small problem, the results dumped as raw arrays so that tests/test_gpu_pcg.py can repeat the case through the
// ctypes wrappers and compare bit for bit. Plain C++17, links liblbfgs_amd_abi3.so.
//   usage: pcg_hip <dir>
// <dir> holds fp32 row-major X.f32 [257][64] and Y.f32 [257][10] (one-hot). Network [64, 32, 10] relu / linear,
// softmax cross-entropy, l2 = 1e-3, bindParams(19). Writes <dir>/params.f32 (the final parameters), loss.f64 (the
// recorder's losses), gradsq.f32 (gradSq at the final parameters, scale 1 / 257) and iterations.txt.
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

} // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::cerr << "usage: pcg_hip <dir>" << std::endl;
    return 2;
  }
  g_dir = argv[1];
  const std::vector<float> xv = read_f32("X.f32", size_t(N) * In), yv = read_f32("Y.f32", size_t(N) * Out);
  hip_mlp::HipHandle h;
  hip_mlp::HipNetwork net(h);
  net.addLayer(In, Hid, hip_mlp::ReLU::id);
  net.addLayer(Hid, Out, hip_mlp::Linear::id);
  net.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
  net.setL2(1e-3);
  net.bindParams(19u);
  hip_mlp::DeviceBuffer<HipScalar> x(h, xv.size()), y(h, yv.size()), dsq(h, 0);
  x.copy_from_host(xv.data(), xv.size());
  y.copy_from_host(yv.data(), yv.size());

  hip_mlp::HipHFPreconditioned s(h, net);
  IterationRecorder<HipBackend> rec;
  rec.init(6);
  s.setRecorder(&rec);
  s.setMaxIterations(6);
  s.setTolerance(1e-9f);
  s.setCG(8, 0.1);
  s.setDamping(0.1);
  s.setPreconditioner(0.75, 2);
  s.solve(int(net.params_size()), net.params_data(), x.data(), y.data(), N, {});

  const size_t n = net.params_size();
  std::vector<float> host(n);
  hip_mlp::hip_check(lbf_memcpy(h.get(), host.data(), net.params_data(), n * sizeof(float), 1), "lbf_memcpy");
  write_raw("params.f32", host.data(), n * sizeof(float));
  dsq.resize(n);
  net.gradSq(x.data(), y.data(), N, 1.0 / N, dsq.data());
  hip_mlp::hip_check(lbf_memcpy(h.get(), host.data(), dsq.data(), n * sizeof(float), 1), "lbf_memcpy");
  write_raw("gradsq.f32", host.data(), n * sizeof(float));
  std::vector<double> l, g;
  rec.copy_to_host(l, g);
  write_raw("loss.f64", l.data(), l.size() * sizeof(double));
  std::FILE *f = std::fopen((g_dir + "/iterations.txt").c_str(), "w");
  if (!f) return 2;
  std::fprintf(f, "%d\n", s.iterations());
  std::fclose(f);
  std::printf("[RESULT] ok\n");
  return 0;
}
