// The curvature spectrum through the C++ drop-in header: HipSpectrum on one small problem, the results dumped as raw
// arrays so that tests/test_gpu_lanczos.py can repeat the case through the ctypes wrappers and compare bit for bit.
// Plain C++17, links liblbfgs_amd_abi3.so.
//   usage: lanczos_hip <dir> [gn|hessian]
// <dir> holds fp32 row-major X.f32 [257][64], Y.f32 [257][10] (one-hot) and v0.f32 (the start vector, parameter
// count floats). Network [64, 32, 10] relu / linear, softmax cross-entropy, bindParams(19), 12 steps with full
// re-orthogonalisation, l2 = 1e-3. Writes <dir>/params.f32, alpha.f64, beta.f64 (12 each), ritz.f64 and
// weights.f64 (steps each) and info.txt (steps, status).
#include "lbfgs_amd/hip_backend.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using hip_mlp::HipScalar;

namespace {

constexpr int In = 64, Hid = 32, Out = 10, N = 257, Steps = 12;
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
    std::cerr << "usage: lanczos_hip <dir> [gn|hessian]" << std::endl;
    return 2;
  }
  g_dir = argv[1];
  const bool exact = argc > 2 && std::strcmp(argv[2], "hessian") == 0;
  const std::vector<float> xv = read_f32("X.f32", size_t(N) * In), yv = read_f32("Y.f32", size_t(N) * Out);
  hip_mlp::HipHandle h;
  hip_mlp::HipNetwork net(h);
  net.addLayer(In, Hid, hip_mlp::ReLU::id);
  net.addLayer(Hid, Out, hip_mlp::Linear::id);
  net.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
  net.bindParams(19u);
  const size_t n = net.params_size();
  const std::vector<float> v0 = read_f32("v0.f32", n);
  hip_mlp::DeviceBuffer<HipScalar> x(h, xv.size()), y(h, yv.size()), dv(h, n);
  x.copy_from_host(xv.data(), xv.size());
  y.copy_from_host(yv.data(), yv.size());
  dv.copy_from_host(v0.data(), n);

  hip_mlp::HipSpectrum sp(h, net);
  sp.setSteps(Steps);
  sp.setMatrix(exact ? LBF_HVP_EXACT : LBF_HVP_GAUSS_NEWTON);
  sp.setL2(1e-3);
  sp.lanczos(dv.data(), x.data(), y.data(), N);
  std::vector<double> weights;
  const std::vector<double> ritz = sp.ritz(&weights);

  std::vector<float> host(n);
  net.handle().sync();
  hip_mlp::hip_check(lbf_memcpy(h.get(), host.data(), net.params_data(), n * sizeof(float), 1), "lbf_memcpy");
  write_raw("params.f32", host.data(), n * sizeof(float));
  write_raw("alpha.f64", sp.alpha().data(), sp.alpha().size() * sizeof(double));
  write_raw("beta.f64", sp.beta().data(), sp.beta().size() * sizeof(double));
  write_raw("ritz.f64", ritz.data(), ritz.size() * sizeof(double));
  write_raw("weights.f64", weights.data(), weights.size() * sizeof(double));
  std::FILE *f = std::fopen((g_dir + "/info.txt").c_str(), "w");
  if (!f) return 2;
  std::fprintf(f, "%d %d\n", sp.steps(), sp.status());
  std::fclose(f);
  std::printf("[RESULT] ok\n");
  return 0;
}
