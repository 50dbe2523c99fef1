// Device-side conjugate gradients (kernels.hpp has the contract; Mlp::gn_cg drives it).
//
// The three sweeps of an iteration read and write n floats each. A sweep's grid is cg_nwg(n) workgroups of 256
// threads in a grid-stride loop over 16-byte groups, so the partial tables have a fixed length and every sum
// has a fixed order: thread-private fp64 accumulation in loop order, wave_sum_f64, then ((v0 + v1) + v2) + v3.
// A table is summed by every workgroup of the launch that consumes it with that same pattern (table_sum), so
// all workgroups form alpha, beta and the stopping decision from the same bits.
//
// Pointers: 4-byte aligned. When every vector of a launch has the same offset from a 16-byte
// boundary, a scalar head brings them to it and the body runs on float4; the n % 4 tail is scalar again. With
// mixed offsets (a caller's x or b one float off, the solver's own r, p, Ap aligned) the whole sweep is scalar.
#include "internal.hpp"
#include "kernels.hpp"
#include "sweep.hpp"

#include <algorithm>
#include <cmath>

namespace lbf {

namespace {

constexpr int kCgMaxWg = 1024; // the cap of loss_partials_wg: 4 workgroups on each of 256 CUs, 1024-word tables

// PC (all three sweeps): preconditioned CG with the diagonal inverse preconditioner minv. z = minv .* r is formed
// in registers wherever it is needed and never stored; rz holds the partials of r.z like rr those of r.r. With
// minv == 1 every product 1 * r is exact and the r.z partials are the r.r partials in the same order, so the PC
// sweeps then write the bits of the plain ones. The plain instantiations compile from the code they always did.
template <bool PC>
__global__ __launch_bounds__(256) void cg_init_kernel(Span sp, float *x, float *r, float *p, const float *b,
                                                      float bscale, double *rr, const float *minv, double *rz) {
  __shared__ double wv[4];
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  double q = 0.0, qz = 0.0;
  for (long long v = gid; v < sp.nvec; v += stride) {
    const long long e = sp.head + 4 * v;
    const f32x4 bv = bscale * *reinterpret_cast<const f32x4 *>(b + e);
    *reinterpret_cast<f32x4 *>(r + e) = bv;
    if constexpr (PC) {
      const f32x4 zv = *reinterpret_cast<const f32x4 *>(minv + e) * bv;
      *reinterpret_cast<f32x4 *>(p + e) = zv;
      qz += double(bv.x) * double(zv.x) + double(bv.y) * double(zv.y) + double(bv.z) * double(zv.z) +
            double(bv.w) * double(zv.w);
    } else {
      *reinterpret_cast<f32x4 *>(p + e) = bv;
    }
    *reinterpret_cast<f32x4 *>(x + e) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    q += double(bv.x) * double(bv.x) + double(bv.y) * double(bv.y) + double(bv.z) * double(bv.z) +
         double(bv.w) * double(bv.w);
  }
  for (long long j = gid; j < span_nscalar(sp); j += stride) {
    const long long e = span_elem(sp, j);
    const float bv = bscale * b[e];
    r[e] = bv;
    if constexpr (PC) {
      const float zv = minv[e] * bv;
      p[e] = zv;
      qz += double(bv) * double(zv);
    } else {
      p[e] = bv;
    }
    x[e] = 0.0f;
    q += double(bv) * double(bv);
  }
  q = block_sum_all(q, wv);
  if (threadIdx.x == 0) rr[blockIdx.x] = q;
  if constexpr (PC) {
    qz = block_sum_all(qz, wv);
    if (threadIdx.x == 0) rz[blockIdx.x] = qz;
  }
}

// One workgroup: rr0 and the first status block. b = 0 is solved by x = 0 in 0 iterations; a non-finite b
// cannot be solved. Either way the abort word freezes the iterations enqueued behind this launch.
// rz (PC only, else null): a non-finite or non-positive r.z of a non-zero b cannot start either.
__global__ __launch_bounds__(256) void cg_start_kernel(const double *rr, int nwg, double *st, int *abort,
                                                       const double *rz) {
  __shared__ double wv[4];
  const double rr0 = table_sum(rr, nwg, wv);
  const double rz0 = rz ? table_sum(rz, nwg, wv) : 1.0;
  if (threadIdx.x != 0) return;
  int status = CG_RUNNING;
  if (rr0 == 0.0) status = CG_CONVERGED;
  else if (!finite_pos(rr0) || !finite_pos(rz0)) status = CG_BREAKDOWN;
  st[CG_ITER] = 0.0;
  st[CG_RR] = rr0;
  st[CG_RR0] = rr0;
  st[CG_STATUS] = double(status);
  st[CG_XB] = st[CG_XR] = st[CG_XX] = 0.0;
  if (status != CG_RUNNING) *abort = 1;
}

__global__ __launch_bounds__(256) void cg_pap_kernel(Span sp, const float *p, const float *Ap, double *pap,
                                                     const int *abort) {
  __shared__ double wv[4];
  if (block_aborted(abort)) return;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  double q = 0.0;
  for (long long v = gid; v < sp.nvec; v += stride) {
    const long long e = sp.head + 4 * v;
    const f32x4 a = *reinterpret_cast<const f32x4 *>(p + e), c = *reinterpret_cast<const f32x4 *>(Ap + e);
    q += double(a.x) * double(c.x) + double(a.y) * double(c.y) + double(a.z) * double(c.z) +
         double(a.w) * double(c.w);
  }
  for (long long j = gid; j < span_nscalar(sp); j += stride) {
    const long long e = span_elem(sp, j);
    q += double(p[e]) * double(Ap[e]);
  }
  q = block_sum_all(q, wv);
  if (threadIdx.x == 0) pap[blockIdx.x] = q;
}

// x += alpha p, r -= alpha Ap with alpha = float(rr_k / pAp); partials of the new r.r into table (k + 1) & 1.
// pAp <= 0 or non-finite: no workgroup writes a vector, workgroup 0 records the breakdown.
// PC: alpha = float(rz_k / pAp); partials of the new r.z (z = minv .* r) into table (k + 1) & 1 of rz as well. A
// non-finite or non-positive rz_k is a breakdown like pAp's.
template <bool PC>
__global__ __launch_bounds__(256) void cg_step_kernel(Span sp, int k, float *x, float *r, const float *p,
                                                      const float *Ap, const double *pap, double *rr, int nwg,
                                                      double *st, int *abort, const float *minv, double *rz) {
  __shared__ double wv[4];
  if (block_aborted(abort)) return;
  const double pAp = table_sum(pap, nwg, wv);
  const double rrk = table_sum(rr + size_t(k & 1) * nwg, nwg, wv);
  double num = rrk;
  bool bad = !finite_pos(pAp);
  if constexpr (PC) {
    num = table_sum(rz + size_t(k & 1) * nwg, nwg, wv);
    bad = bad || !finite_pos(num);
  }
  if (bad) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      st[CG_ITER] = double(k);
      st[CG_RR] = rrk;
      st[CG_STATUS] = double(CG_BREAKDOWN);
      *abort = 1;
    }
    return;
  }
  const float alpha = float(num / pAp);
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  double q = 0.0, qz = 0.0;
  for (long long v = gid; v < sp.nvec; v += stride) {
    const long long e = sp.head + 4 * v;
    const f32x4 pv = *reinterpret_cast<const f32x4 *>(p + e), av = *reinterpret_cast<const f32x4 *>(Ap + e);
    f32x4 xv = *reinterpret_cast<f32x4 *>(x + e), rv = *reinterpret_cast<f32x4 *>(r + e);
    xv.x = __builtin_fmaf(alpha, pv.x, xv.x);
    xv.y = __builtin_fmaf(alpha, pv.y, xv.y);
    xv.z = __builtin_fmaf(alpha, pv.z, xv.z);
    xv.w = __builtin_fmaf(alpha, pv.w, xv.w);
    rv.x = __builtin_fmaf(-alpha, av.x, rv.x);
    rv.y = __builtin_fmaf(-alpha, av.y, rv.y);
    rv.z = __builtin_fmaf(-alpha, av.z, rv.z);
    rv.w = __builtin_fmaf(-alpha, av.w, rv.w);
    *reinterpret_cast<f32x4 *>(x + e) = xv;
    *reinterpret_cast<f32x4 *>(r + e) = rv;
    q += double(rv.x) * double(rv.x) + double(rv.y) * double(rv.y) + double(rv.z) * double(rv.z) +
         double(rv.w) * double(rv.w);
    if constexpr (PC) {
      const f32x4 zv = *reinterpret_cast<const f32x4 *>(minv + e) * rv;
      qz += double(rv.x) * double(zv.x) + double(rv.y) * double(zv.y) + double(rv.z) * double(zv.z) +
            double(rv.w) * double(zv.w);
    }
  }
  for (long long j = gid; j < span_nscalar(sp); j += stride) {
    const long long e = span_elem(sp, j);
    x[e] = __builtin_fmaf(alpha, p[e], x[e]);
    const float rv = __builtin_fmaf(-alpha, Ap[e], r[e]);
    r[e] = rv;
    q += double(rv) * double(rv);
    if constexpr (PC) qz += double(rv) * double(minv[e] * rv);
  }
  q = block_sum_all(q, wv);
  if (threadIdx.x == 0) rr[size_t((k + 1) & 1) * nwg + blockIdx.x] = q;
  if constexpr (PC) {
    qz = block_sum_all(qz, wv);
    if (threadIdx.x == 0) rz[size_t((k + 1) & 1) * nwg + blockIdx.x] = qz;
  }
}

// The stopping test on rr_{k+1}; p = r + beta p with beta = float(rr_{k+1} / rr_k) when the solve goes on.
// On a stop no workgroup writes p; workgroup 0 writes the status block either way.
// PC: the test is unchanged (on r.r); p = minv .* r + beta p with beta = float(rz_{k+1} / rz_k). A solve that would
// go on with a non-finite or non-positive rz_{k+1} stops as a breakdown instead (x and r are the iterate's).
template <bool PC>
__global__ __launch_bounds__(256) void cg_dir_kernel(Span sp, int k, const float *r, float *p, const double *rr,
                                                     int nwg, double *st, int *abort, int max_iters,
                                                     double tol2, const float *minv, const double *rz) {
  __shared__ double wv[4];
  if (block_aborted(abort)) return;
  const double rrn = table_sum(rr + size_t((k + 1) & 1) * nwg, nwg, wv);
  const double rrk = table_sum(rr + size_t(k & 1) * nwg, nwg, wv);
  const double rr0 = st[CG_RR0]; // written by cg_start, an earlier launch
  double bn = rrn, bk = rrk;
  if constexpr (PC) {
    bn = table_sum(rz + size_t((k + 1) & 1) * nwg, nwg, wv);
    bk = table_sum(rz + size_t(k & 1) * nwg, nwg, wv);
  }
  int status = CG_RUNNING;
  if (rrn <= tol2 * rr0) status = CG_CONVERGED;
  else if (k + 1 >= max_iters) status = CG_MAXITER;
  else if (PC && !finite_pos(bn)) status = CG_BREAKDOWN;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st[CG_ITER] = double(k + 1);
    st[CG_RR] = rrn;
    st[CG_STATUS] = double(status);
    if (status != CG_RUNNING) *abort = 1;
  }
  if (status != CG_RUNNING) return;
  const float beta = float(bn / bk);
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  for (long long v = gid; v < sp.nvec; v += stride) {
    const long long e = sp.head + 4 * v;
    f32x4 rv = *reinterpret_cast<const f32x4 *>(r + e);
    if constexpr (PC) rv = *reinterpret_cast<const f32x4 *>(minv + e) * rv;
    f32x4 pv = *reinterpret_cast<f32x4 *>(p + e);
    pv.x = __builtin_fmaf(beta, pv.x, rv.x);
    pv.y = __builtin_fmaf(beta, pv.y, rv.y);
    pv.z = __builtin_fmaf(beta, pv.z, rv.z);
    pv.w = __builtin_fmaf(beta, pv.w, rv.w);
    *reinterpret_cast<f32x4 *>(p + e) = pv;
  }
  for (long long j = gid; j < span_nscalar(sp); j += stride) {
    const long long e = span_elem(sp, j);
    float rv = r[e];
    if constexpr (PC) rv = minv[e] * rv;
    p[e] = __builtin_fmaf(beta, p[e], rv);
  }
}

// minv = (d + kappa)^(-alpha): the inverse of the diagonal preconditioner (d + kappa)^alpha. alpha == 0 gives ones.
__global__ __launch_bounds__(256) void precond_minv_kernel(long long n, const float *d, float kappa, float alpha,
                                                           float *minv) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) minv[e] = powf(d[e] + kappa, -alpha);
}

// Partials of x.(bscale b), x.r, x.x: tables 0, 1, 2 of xd.
__global__ __launch_bounds__(256) void cg_xdots_kernel(Span sp, const float *x, const float *r, const float *b,
                                                       float bscale, double *xd, int nwg) {
  __shared__ double wv[4];
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  double qb = 0.0, qr = 0.0, qx = 0.0;
  for (long long v = gid; v < sp.nvec; v += stride) {
    const long long e = sp.head + 4 * v;
    const f32x4 xv = *reinterpret_cast<const f32x4 *>(x + e), rv = *reinterpret_cast<const f32x4 *>(r + e);
    const f32x4 bv = bscale * *reinterpret_cast<const f32x4 *>(b + e);
    qb += double(xv.x) * double(bv.x) + double(xv.y) * double(bv.y) + double(xv.z) * double(bv.z) +
          double(xv.w) * double(bv.w);
    qr += double(xv.x) * double(rv.x) + double(xv.y) * double(rv.y) + double(xv.z) * double(rv.z) +
          double(xv.w) * double(rv.w);
    qx += double(xv.x) * double(xv.x) + double(xv.y) * double(xv.y) + double(xv.z) * double(xv.z) +
          double(xv.w) * double(xv.w);
  }
  for (long long j = gid; j < span_nscalar(sp); j += stride) {
    const long long e = span_elem(sp, j);
    const float xv = x[e], bv = bscale * b[e];
    qb += double(xv) * double(bv);
    qr += double(xv) * double(r[e]);
    qx += double(xv) * double(xv);
  }
  qb = block_sum_all(qb, wv);
  qr = block_sum_all(qr, wv);
  qx = block_sum_all(qx, wv);
  if (threadIdx.x == 0) {
    xd[blockIdx.x] = qb;
    xd[size_t(nwg) + blockIdx.x] = qr;
    xd[2 * size_t(nwg) + blockIdx.x] = qx;
  }
}
__global__ __launch_bounds__(256) void cg_xfin_kernel(const double *xd, int nwg, double *st) {
  __shared__ double wv[4];
  const double qb = table_sum(xd, nwg, wv), qr = table_sum(xd + nwg, nwg, wv), qx = table_sum(xd + 2 * size_t(nwg), nwg, wv);
  if (threadIdx.x == 0) {
    st[CG_XB] = qb;
    st[CG_XR] = qr;
    st[CG_XX] = qx;
  }
}

} // namespace

int cg_nwg(long long n) { return int(std::max(1LL, std::min<long long>(cdiv(n, 1024), kCgMaxWg))); }

void cg_init(hipStream_t s, const CgArgs &a) {
  const int nwg = cg_nwg(a.n);
  if (a.minv)
    hipLaunchKernelGGL(cg_init_kernel<true>, dim3(unsigned(nwg)), dim3(256), 0, s,
                       make_span(a.n, a.x, a.r, a.p, a.b, a.minv), a.x, a.r, a.p, a.b, a.bscale, a.rr, a.minv, a.rz);
  else
    hipLaunchKernelGGL(cg_init_kernel<false>, dim3(unsigned(nwg)), dim3(256), 0, s,
                       make_span(a.n, a.x, a.r, a.p, a.b), a.x, a.r, a.p, a.b, a.bscale, a.rr, nullptr, nullptr);
  LBF_KERNEL_CHECK();
  hipLaunchKernelGGL(cg_start_kernel, dim3(1), dim3(256), 0, s, a.rr, nwg, a.st, a.abort,
                     a.minv ? (const double *)a.rz : nullptr);
  LBF_KERNEL_CHECK();
}

void cg_pap(hipStream_t s, const CgArgs &a) {
  hipLaunchKernelGGL(cg_pap_kernel, dim3(unsigned(cg_nwg(a.n))), dim3(256), 0, s, make_span(a.n, a.p, a.Ap), a.p,
                     a.Ap, a.pap, a.abort);
  LBF_KERNEL_CHECK();
}

void cg_step(hipStream_t s, const CgArgs &a, int k) {
  const int nwg = cg_nwg(a.n);
  if (a.minv)
    hipLaunchKernelGGL(cg_step_kernel<true>, dim3(unsigned(nwg)), dim3(256), 0, s,
                       make_span(a.n, a.x, a.r, a.p, a.Ap, a.minv), k, a.x, a.r, a.p, a.Ap, a.pap, a.rr, nwg, a.st,
                       a.abort, a.minv, a.rz);
  else
    hipLaunchKernelGGL(cg_step_kernel<false>, dim3(unsigned(nwg)), dim3(256), 0, s,
                       make_span(a.n, a.x, a.r, a.p, a.Ap), k, a.x, a.r, a.p, a.Ap, a.pap, a.rr, nwg, a.st, a.abort,
                       nullptr, nullptr);
  LBF_KERNEL_CHECK();
}

void cg_dir(hipStream_t s, const CgArgs &a, int k) {
  const int nwg = cg_nwg(a.n);
  if (a.minv)
    hipLaunchKernelGGL(cg_dir_kernel<true>, dim3(unsigned(nwg)), dim3(256), 0, s, make_span(a.n, a.r, a.p, a.minv), k,
                       a.r, a.p, a.rr, nwg, a.st, a.abort, a.max_iters, a.tol2, a.minv, (const double *)a.rz);
  else
    hipLaunchKernelGGL(cg_dir_kernel<false>, dim3(unsigned(nwg)), dim3(256), 0, s, make_span(a.n, a.r, a.p), k, a.r,
                       a.p, a.rr, nwg, a.st, a.abort, a.max_iters, a.tol2, nullptr, nullptr);
  LBF_KERNEL_CHECK();
}

void cg_xdots(hipStream_t s, const CgArgs &a) {
  const int nwg = cg_nwg(a.n);
  hipLaunchKernelGGL(cg_xdots_kernel, dim3(unsigned(nwg)), dim3(256), 0, s, make_span(a.n, a.x, a.r, a.b), a.x, a.r,
                     a.b, a.bscale, a.xd, nwg);
  LBF_KERNEL_CHECK();
  hipLaunchKernelGGL(cg_xfin_kernel, dim3(1), dim3(256), 0, s, a.xd, nwg, a.st);
  LBF_KERNEL_CHECK();
}

void precond_minv(hipStream_t s, long long n, const float *d, double kappa, double alpha, float *minv) {
  if (n <= 0) return;
  hipLaunchKernelGGL(precond_minv_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, n, d, float(kappa),
                     float(alpha), minv);
  LBF_KERNEL_CHECK();
}

} // namespace lbf
