// Stand-alone program over csrc/tridiag.cpp (no GPU, no library): built with -fsanitize=address,undefined by
// tests/test_lanczos_host.py and run as a process of its own.
//   tridiag_harness            : the self-checks below, then "tridiag harness ok"
//   tridiag_harness m seed     : a random T of order m from a 64-bit LCG; prints "alpha ..", "beta ..", "theta ..",
//                                "weight .." with 17 significant digits for the test to compare with numpy
#include "tridiag.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

int fails = 0;
void expect(bool ok, const char *what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s\n", what);
    ++fails;
  }
}

struct Lcg {
  unsigned long long s;
  double next() { // uniform in (-1, 1)
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return double(s >> 11) / 4503599627370496.0 - 1.0;
  }
};

// |T v_k - theta_k v_k|_inf over all k, and |V^T V - I|_inf
void residuals(int m, const std::vector<double> &a, const std::vector<double> &b, const std::vector<double> &th,
               const std::vector<double> &V, double *res, double *orth) {
  *res = *orth = 0.0;
  for (int k = 0; k < m; ++k) {
    for (int i = 0; i < m; ++i) {
      double t = a[size_t(i)] * V[size_t(i) * m + k];
      if (i > 0) t += b[size_t(i - 1)] * V[size_t(i - 1) * m + k];
      if (i + 1 < m) t += b[size_t(i)] * V[size_t(i + 1) * m + k];
      *res = std::fmax(*res, std::fabs(t - th[size_t(k)] * V[size_t(i) * m + k]));
    }
    for (int l = 0; l < m; ++l) {
      double d = 0.0;
      for (int i = 0; i < m; ++i) d += V[size_t(i) * m + k] * V[size_t(i) * m + l];
      *orth = std::fmax(*orth, std::fabs(d - (k == l ? 1.0 : 0.0)));
    }
  }
}

void check_case(int m, const std::vector<double> &a, const std::vector<double> &b, double scale, const char *what) {
  // exactly-sized allocations, so that an access past either end is an AddressSanitizer report
  const size_t n = size_t(m);
  std::vector<double> th(n), w(n), V(n * n), th2(n), w2(n);
  expect(lbf::tridiag_eig(m, a.data(), m > 1 ? b.data() : nullptr, th.data(), w.data(), V.data()), what);
  expect(lbf::tridiag_eig(m, a.data(), m > 1 ? b.data() : nullptr, th2.data(), w2.data(), nullptr), what);
  double res, orth, wsum = 0.0;
  residuals(m, a, b, th, V, &res, &orth);
  for (int k = 0; k < m; ++k) {
    wsum += w[size_t(k)];
    expect(k == 0 || th[size_t(k - 1)] <= th[size_t(k)], "ascending");
    expect(th[size_t(k)] == th2[size_t(k)], "eigenvalues do not depend on whether the vectors are asked for");
    expect(std::fabs(w[size_t(k)] - w2[size_t(k)]) <= 1e-13, "weights do not depend on it either");
    expect(std::fabs(w[size_t(k)] - V[size_t(k)] * V[size_t(k)]) <= 1e-15, "weights are the squared first row");
  }
  const double tol = 64.0 * m * 2.220446049250313e-16 * scale;
  expect(res <= tol, what);
  expect(orth <= 64.0 * m * 2.220446049250313e-16, "orthonormal vectors");
  expect(std::fabs(wsum - 1.0) <= 1e-13, "weights sum to 1");
}

} // namespace

int main(int argc, char **argv) {
  if (argc >= 3) {
    const int m = std::atoi(argv[1]);
    Lcg g{(unsigned long long)std::atoll(argv[2])};
    const size_t n = size_t(m);
    std::vector<double> a(n), b(n > 1 ? n - 1 : 0), th(n), w(n);
    for (double &v : a) v = g.next();
    for (double &v : b) v = g.next();
    if (!lbf::tridiag_eig(m, a.data(), b.empty() ? nullptr : b.data(), th.data(), w.data(), nullptr)) return 1;
    auto dump = [](const char *tag, const std::vector<double> &v) {
      std::printf("%s", tag);
      for (double x : v) std::printf(" %.17g", x);
      std::printf("\n");
    };
    dump("alpha", a);
    dump("beta", b);
    dump("theta", th);
    dump("weight", w);
    return 0;
  }
  Lcg g{12345};
  for (int m : {1, 2, 3, 7, 32, 128}) {
    const size_t n = size_t(m);
    std::vector<double> a(n), b(n > 1 ? n - 1 : 0);
    for (double &v : a) v = g.next();
    for (double &v : b) v = g.next();
    check_case(m, a, b, 3.0, "random");
    if (m >= 3) {
      b[size_t(m / 2)] = 0.0; // decoupled blocks
      check_case(m, a, b, 3.0, "zero beta");
      for (double &v : b) v = 0.0; // diagonal, with repeated eigenvalues
      for (double &v : a) v = 2.0;
      check_case(m, a, b, 2.0, "diagonal");
    }
  }
  { // widely graded
    const int m = 24;
    std::vector<double> a(24), b(23);
    for (int i = 0; i < m; ++i) a[size_t(i)] = std::pow(10.0, 8.0 - i);
    for (int i = 0; i + 1 < m; ++i) b[size_t(i)] = 0.1 * std::pow(10.0, 8.0 - i - 1);
    check_case(m, a, b, 1e8, "graded");
  }
  { // bad arguments are refused, a non-finite entry ends without a report
    double one = 1.0, out = 0.0, nan = std::nan("");
    expect(!lbf::tridiag_eig(0, &one, nullptr, &out, nullptr, nullptr), "m = 0");
    expect(!lbf::tridiag_eig(1, nullptr, nullptr, &out, nullptr, nullptr), "null alpha");
    std::vector<double> a{1.0, nan, 2.0}, b{0.5, 0.5}, th(3);
    expect(!lbf::tridiag_eig(3, a.data(), b.data(), th.data(), nullptr, nullptr), "a NaN entry");
  }
  if (fails) return 1;
  std::printf("tridiag harness ok\n");
  return 0;
}
