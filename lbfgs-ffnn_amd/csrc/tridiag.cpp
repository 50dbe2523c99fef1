// Implicit QL on a symmetric tridiagonal matrix (tridiag.hpp), after EISPACK's tql2. The rotations are applied to
// `rows` rows of Z = I: all m of them when the eigenvectors are wanted, else the first alone, which is all the
// quadrature weights need.
#include "tridiag.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace lbf {

bool tridiag_eig(int m, const double *alpha, const double *beta, double *theta, double *first_sq, double *vecs) {
  if (m < 1 || !alpha || !theta || (m > 1 && !beta)) return false;
  const int rows = vecs ? m : 1;
  std::vector<double> d(alpha, alpha + m), e(size_t(m), 0.0), z(size_t(rows) * size_t(m), 0.0);
  for (int i = 0; i + 1 < m; ++i) e[size_t(i)] = beta[i];
  for (int i = 0; i < rows; ++i) z[size_t(i) * m + i] = 1.0;
  for (int l = 0; l < m; ++l) {
    for (int iter = 0;; ++iter) {
      int mm = l;
      for (; mm + 1 < m; ++mm) {
        const double dd = std::fabs(d[mm]) + std::fabs(d[mm + 1]);
        if (std::fabs(e[mm]) + dd == dd) break; // negligible beside its neighbours (also e == 0)
      }
      if (mm == l) break;
      if (iter == 60) return false;
      double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
      double r = std::hypot(g, 1.0);
      g = d[mm] - d[l] + e[l] / (g + std::copysign(r, g));
      double s = 1.0, c = 1.0, p = 0.0;
      int i = mm - 1;
      for (; i >= l; --i) {
        double f = s * e[i];
        const double b = c * e[i];
        r = std::hypot(f, g);
        e[i + 1] = r;
        if (r == 0.0) { // underflow: deflate and start the sweep again
          d[i + 1] -= p;
          e[mm] = 0.0;
          break;
        }
        s = f / r;
        c = g / r;
        g = d[i + 1] - p;
        r = (d[i] - g) * s + 2.0 * c * b;
        p = s * r;
        d[i + 1] = g + p;
        g = c * r - b;
        for (int k = 0; k < rows; ++k) {
          double *zk = &z[size_t(k) * m];
          f = zk[i + 1];
          zk[i + 1] = s * zk[i] + c * f;
          zk[i] = c * zk[i] - s * f;
        }
      }
      if (r == 0.0 && i >= l) continue;
      d[l] -= p;
      e[l] = g;
      e[mm] = 0.0;
    }
  }
  for (int i = 0; i < m; ++i)
    if (!std::isfinite(d[i])) return false;
  std::vector<int> order(size_t(m), 0);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return d[a] < d[b]; });
  for (int k = 0; k < m; ++k) {
    const int src = order[size_t(k)];
    theta[k] = d[src];
    if (first_sq) first_sq[k] = z[src] * z[src];
    if (vecs)
      for (int i = 0; i < m; ++i) vecs[size_t(i) * m + k] = z[size_t(i) * m + src];
  }
  return true;
}

} // namespace lbf
