// The output layer's loss kernels on the generic route, the gradient's finishing dots and the line-search
// decision (gfx950, wave64). Partials are fp64, one word per workgroup, summed in a fixed order (block_sum).
//
// Replaces: diff_kernel (src/cuda/kernels.cuh:136-153) with network.cuh:97-107 and layer.cuh:72, cublasSdot with
// host pointer mode (kernels.cuh:28-50), the S-LBFGS L2 term (unified_optimization.hpp:375) and the host's
// Wolfe / Armijo tests (full_batch_minimizer.hpp:136-152, src/cuda/lbfgs.cuh:159-163).
//
// Implements (kernels.hpp): loss_partials_wg, loss_diff, loss_xent, dots_partials_wg, finalize_grad_dots,
// add_l2_rows, dot_partials, ls_ctl.
#include "act.hpp"
#include "internal.hpp"
#include "kernels.hpp"
#include "wave.hpp"

namespace lbf {

// ---------------------------------------------------------------------------------------------
// Output layer: diff = A_out - Y ; dZ = diff * act'(A_out) * inv_scale ; partial sum(diff^2).
// src/cuda/network.cuh:97-107 (diff, 0.5*dot(diff,diff)/B, diff*=1/B) and layer.cuh:72 (act').
// ---------------------------------------------------------------------------------------------
int loss_partials_wg(long long B, int Out) {
  long long e = B * Out;
  long long w = cdiv(e, 256 * 8);
  return int(w < 1 ? 1 : (w > 1024 ? 1024 : w));
}

template <bool XACT> // XACT: all seven activation bodies (act.hpp), else the four
__global__ __launch_bounds__(256) void loss_diff_kernel(const float *A, long long lda, const float *Y, long long ldy,
                                                        const int *idx, long long B, int Out, int act,
                                                        double inv_scale, float *dZ, long long ldz,
                                                        double *partials) {
  __shared__ double scratch[16];
  const long long total = B * Out;
  const long long stride = (long long)gridDim.x * blockDim.x;
  double acc[1] = {0.0};
  const float sc = float(inv_scale);
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const long long b = e / Out;
    const int o = int(e - b * Out);
    const float a = A[b * lda + o];
    const long long yr = idx ? (long long)idx[b] : b;
    const float d = a - Y[yr * ldy + o];
    acc[0] += double(d) * double(d);
    dZ[b * ldz + o] = d * (XACT ? dact_rt(act, a) : dact_rt4(act, a)) * sc;
  }
  block_sum<1>(acc, scratch);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}

void loss_diff(hipStream_t s, const float *Aout, long long lda, const float *Y, long long ldy, const int *idx,
               long long B, int Out, int act, double inv_scale, float *dZ, long long ldz, double *partials) {
  hipLaunchKernelGGL(act_in_heads(act) ? loss_diff_kernel<false> : loss_diff_kernel<true>, dim3(loss_partials_wg(B, Out)), dim3(256), 0, s, Aout, lda, Y, ldy, idx, B,
                     Out, act, inv_scale, dZ, ldz, partials);
  LBF_KERNEL_CHECK();
}

// Softmax cross-entropy on the logits Z (LOSS_XENT), row-wise: wave w of block k takes rows 4k + w,
// 4k + w + 4 gridDim, ...; its lanes stride over the Out logits in three passes (maximum; exp-sum, Ysum;
// loss terms and dZ: the row is a few cache lines, re-read from L1/L2). lse - z_o = (m - z_o) + log(se).
// Partial per block: 2 sum y (lse - z), fp64, fixed order (lane accumulators, block_sum).
__global__ __launch_bounds__(256) void loss_xent_kernel(const float *Z, long long ldz_in, const float *Y, long long ldy,
                                                        const int *idx, long long B, int Out, double inv_scale,
                                                        float *dZ, long long ldz, double *partials) {
  __shared__ double scratch[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float sc = float(inv_scale);
  double acc[1] = {0.0};
  for (long long b = (long long)blockIdx.x * 4 + wave; b < B; b += (long long)gridDim.x * 4) { // wave-uniform
    const float *z = Z + b * ldz_in;
    const float *y = Y + (idx ? (long long)idx[b] : b) * ldy;
    float m = -INFINITY;
    for (int o = lane; o < Out; o += 64) m = fmaxf(m, z[o]);
    m = wave_max_f32(m);
    double se = 0.0, ys = 0.0;
    for (int o = lane; o < Out; o += 64) {
      se += double(expf(z[o] - m));
      ys += double(y[o]);
    }
    const float sef = float(wave_sum_f64(se)), ysum = float(wave_sum_f64(ys));
    const float lg = logf(sef), rs = 1.0f / sef;
    for (int o = lane; o < Out; o += 64) {
      const float zo = z[o], yo = y[o];
      acc[0] += 2.0 * double(yo) * double((m - zo) + lg);
      dZ[b * ldz + o] = (expf(zo - m) * rs * ysum - yo) * sc;
    }
  }
  block_sum<1>(acc, scratch);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}

void loss_xent(hipStream_t s, const float *Z, long long ldz_in, const float *Y, long long ldy, const int *idx,
               long long B, int Out, double inv_scale, float *dZ, long long ldz, double *partials) {
  hipLaunchKernelGGL(loss_xent_kernel, dim3(loss_partials_wg(B, Out)), dim3(256), 0, s, Z, ldz_in, Y, ldy, idx, B,
                     Out, inv_scale, dZ, ldz, partials);
  LBF_KERNEL_CHECK();
}

// ---------------------------------------------------------------------------------------------
// finalize: g += lambda*w (S-LBFGS L2 term, unified_optimization.hpp:375) ; partial (g.g, g.p, w.w)
// ---------------------------------------------------------------------------------------------
int dots_partials_wg(long long n) {
  long long w = cdiv(n, 256 * 8);
  return int(w < 1 ? 1 : (w > 512 ? 512 : w));
}

// g_in (nullable): read the gradient there and always write g (a data-parallel evaluation's all-reduced
// words buffer -> the live gradient, only when the speculative chain was not aborted)
__global__ __launch_bounds__(256) void finalize_kernel(long long n, float *g, const float *g_in, const float *w,
                                                       double lambda, const float *p, double *partials,
                                                       const int *abort) {
  if (abort && *abort) return;
  __shared__ double scratch[48];
  double acc[3] = {0.0, 0.0, 0.0};
  const long long stride = (long long)gridDim.x * blockDim.x;
  const float lf = float(lambda);
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    float gv = (g_in ? g_in : g)[e];
    const float wv = w ? w[e] : 0.0f;
    if (lambda != 0.0) gv = gv + lf * wv;
    if (lambda != 0.0 || g_in) g[e] = gv;
    acc[0] += double(gv) * double(gv);
    if (p) acc[1] += double(gv) * double(p[e]);
    acc[2] += double(wv) * double(wv);
  }
  block_sum<3>(acc, scratch);
  if (threadIdx.x == 0) {
    partials[blockIdx.x * 3 + 0] = acc[0];
    partials[blockIdx.x * 3 + 1] = acc[1];
    partials[blockIdx.x * 3 + 2] = acc[2];
  }
}

// G[r * ld + e] += lambda w[e] for r < rows, e < n: finalize_kernel's update (same fp32 expression) on
// each of a block of per-minibatch gradients (Mlp::batch_grads).
__global__ __launch_bounds__(256) void add_l2_rows_kernel(long long n, int rows, long long ld, float *G,
                                                          const float *w, double lambda) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const float lf = float(lambda), wv = w[e];
  float *g = G + e;
  // written as the fused multiply-add the contracted `gv + lf * wv` of finalize_kernel / reduce_all
  // compiles to (here the product is loop-invariant and would otherwise be hoisted and rounded once)
  for (int r = 0; r < rows; ++r) g[r * ld] = __builtin_fmaf(lf, wv, g[r * ld]);
}

void add_l2_rows(hipStream_t s, long long n, int rows, long long ld, float *G, const float *w, double lambda) {
  if (n <= 0 || rows <= 0 || lambda == 0.0) return;
  hipLaunchKernelGGL(add_l2_rows_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, n, rows, ld, G, w, lambda);
  LBF_KERNEL_CHECK();
}

void finalize_grad_dots(hipStream_t s, long long n, float *g, const float *w, double lambda, const float *p,
                        double *partials, const int *abort, const float *g_in) {
  hipLaunchKernelGGL(finalize_kernel, dim3(dots_partials_wg(n)), dim3(256), 0, s, n, g, g_in, w, lambda, p, partials,
                     abort);
  LBF_KERNEL_CHECK();
}

__global__ __launch_bounds__(256) void dot_kernel(long long n, const float *x, const float *y, double *partials) {
  __shared__ double scratch[16];
  double acc[1] = {0.0};
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride)
    acc[0] += double(x[e]) * double(y[e]);
  block_sum<1>(acc, scratch);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}

void dot_partials(hipStream_t s, long long n, const float *x, const float *y, double *partials) {
  hipLaunchKernelGGL(dot_kernel, dim3(dots_partials_wg(n)), dim3(256), 0, s, n, x, y, partials);
  LBF_KERNEL_CHECK();
}

// Acceptance test of the first line-search trial, evaluated exactly as the host would (no FMA
// contraction, same precision): Wolfe in fp64 (full_batch_minimizer.hpp:136-152), Armijo in fp32
// (lbfgs.cuh:159-163). Convergence uses the next iteration's entry test (lbfgs.hpp:42, lbfgs.cuh:143).
__global__ __launch_bounds__(64) void ls_ctl_kernel(const LsCtlArgs a) {
  if (threadIdx.x != 0 || *a.abort) return;
  double *sc = a.scal;
  const double fn = sc[SC_LOSS], gfo = sc[SC_GTP], gnp = sc[SC_TGP], tgg = sc[SC_TGG];
  bool ok, conv;
  if (!a.armijo) {
    const double fold = a.host_fold ? a.fold : sc[SC_FOLD];
    ok = a.first || (!(fn > __dadd_rn(fold, __dmul_rn(__dmul_rn(a.c1, a.alpha), gfo))) && !(gnp < __dmul_rn(a.c2, gfo)));
    conv = sqrt(tgg) < a.tol;
    if (ok) sc[SC_FOLD] = fn;
  } else {
    const float foldf = a.host_fold ? a.foldf : float(sc[SC_FOLDF]);
    const float lnew = float(fn), gdp = float(gfo);
    ok = lnew <= __fadd_rn(foldf, __fmul_rn(__fmul_rn(float(a.c1), a.alphaf), gdp));
    conv = float(sqrt(tgg)) < float(a.tol);
    if (ok) sc[SC_FOLDF] = double(lnew);
  }
  const int status = !ok ? SPEC_REJECT : (conv ? SPEC_CONVERGED : SPEC_ACCEPT);
  if (status != SPEC_ACCEPT) *a.abort = 1;
  // The record lives in host memory. Every field is stored write-through (system-scope relaxed
  // atomic stores: sc0 sc1, no cache write-back), the payload is acknowledged before the sequence word
  // is stored, so a host that sees seq sees the payload. (A system-scope release fence would write
  // back the whole L2 - microseconds for nothing here.)
  SpecRecord *r = a.rec;
  const double alpha0 = sc[SC_ALPHA0], accept_prev = sc[SC_ACCEPT];
  __hip_atomic_store(&r->loss, fn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&r->tgg, tgg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&r->alpha0, alpha0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&r->accept_prev, accept_prev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&r->status, status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(&r->seq, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

void ls_ctl(hipStream_t s, const LsCtlArgs &a) {
  hipLaunchKernelGGL(ls_ctl_kernel, dim3(1), dim3(64), 0, s, a);
  LBF_KERNEL_CHECK();
}

} // namespace lbf
