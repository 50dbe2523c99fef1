// Exact Hessian-vector product of the MLP's MSE loss (Pearlmutter's R-operator), SURVEY.md §8(f)
// rank 4: the option that replaces S-LBFGS's finite-difference HVP (s_lbfgs.hpp:88-101, which loses
// ~1e-2 relative to fp32 cancellation) by H(w) v computed in one forward + backward R-pass.
//
// With Z_l = A_{l-1} W_l + b_l, A_l = act_l(Z_l), e = (A_L - y) * s (s = inv_scale),
// dZ_L = e .* act'_L, delta_{l-1} = dZ_l W_l^T, dZ_{l-1} = delta_{l-1} .* act'_{l-1}, and the
// direction V = [V_l ; v_l] in the parameter layout:
//   R{Z_l}  = R{A_{l-1}} W_l + A_{l-1} V_l + v_l          (R{A_{-1}} = R{X} = 0)
//   R{A_l}  = act'_l .* R{Z_l}
//   R{dZ_L} = s (act'_L^2 + (A_L - y) act''_L) .* R{Z_L}
//   R{dZ_{l-1}} = (R{dZ_l} W_l^T + dZ_l V_l^T) .* act'_{l-1} + delta_{l-1} .* act''_{l-1} .* R{Z_{l-1}}
//   (H v)_l = [A_{l-1} | 1]^T R{dZ_l} + [R{A_{l-1}} | 0]^T dZ_l   (+ lambda v)
// With the softmax cross-entropy loss (linear last layer, dZ_L = s (p Ysum - y)) only the output step changes:
//   R{dZ_L} = s Ysum p .* (R{Z_L} - sum_k p_k R{Z_L}_k)                      (rop_out_xent)
// The products are the engine's MFMA GEMMs (mlp_curvature.cpp Mlp::hvp); this file holds the elementwise
// R-steps. act' and act'' are taken through the post-activation value a (act.hpp convention):
// tanh 1-a^2, -2a(1-a^2); sigmoid a(1-a), a(1-a)(1-2a); relu [a>0], 0; linear 1, 0; leaky relu [a>0] + 0.01 [a<=0], 0;
// elu (a<=0: a+1, a+1; else 1, 0); softplus 1-e^-a, e^-a (1-e^-a).
//
// Gauss-Newton product G v = J^T H_L J v (Mlp::gnvp): the same R-forward, the convex loss's Hessian
// H_L applied to R{Z_L}, then an ordinary backward pass. The loss is split from the network at A_L for the
// squared error (H_L = s I) and at the logits for the cross-entropy (H_L = s Ysum (diag p - p p^T)):
//   T_l = A_{l-1} V_l + v_l,  R{Z_l} = T_l + R{A_{l-1}} W_l,  R{A_l} = act'_l .* R{Z_l}          (gn_act)
//   M_L = s act'_L^2 .* R{Z_L}  (gn_out_mse)  |  s Ysum p .* (R{Z_L} - sum_k p_k R{Z_L}_k)       (gn_out_xent)
//   (G v)_l = [A_{l-1} | 1]^T M_l,  M_{l-1} = (M_l W_l^T) .* act'_{l-1}    (+ lambda v)
// i.e. the exact product without (A_L - y) act''_L, [R{A_{l-1}} | 0]^T dZ_l, dZ_l V_l^T and delta act'' R{Z}.
#include "act.hpp"
#include "internal.hpp"
#include "kernels.hpp"
#include "wave.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace lbf {

namespace {

__device__ __forceinline__ float d2act_rt(int act, float a) {
  switch (act) {
  case ACT_TANH: return -2.0f * a * (1.0f - a * a);
  case ACT_SIGMOID: return a * (1.0f - a) * (1.0f - 2.0f * a);
  case ACT_ELU: return a > 0.0f ? 0.0f : a + 1.0f;
  case ACT_SOFTPLUS: return expf(-a) * -expm1f(-a);
  default: return 0.0f;
  }
}

// RA = act'(A) .* RZ
__global__ __launch_bounds__(256) void rop_act_kernel(long long n, const float *A, const float *RZ, int act,
                                                      float *RA) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) RA[e] = dact_rt(act, A[e]) * RZ[e];
}

// RdZ = s (act'(A)^2 + (A - y) act''(A)) .* RZ on the output layer (rows gathered by idx)
__global__ __launch_bounds__(256) void rop_out_kernel(long long B, int Out, const float *A, const float *Y,
                                                      const int *idx, const float *RZ, int act, float s,
                                                      float *RdZ) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * Out) return;
  const long long b = e / Out;
  const int o = int(e - b * Out);
  const float a = A[e], y = Y[(idx ? (long long)idx[b] : b) * Out + o];
  const float d1 = dact_rt(act, a);
  RdZ[e] = s * (d1 * d1 + (a - y) * d2act_rt(act, a)) * RZ[e];
}

// Softmax cross-entropy on logits Z: dZ = s (p Ysum - y), so RdZ = s Ysum p .* (RZ - sum_k p_k RZ_k), the
// softmax Jacobian applied to RZ. One wave per row (rows 4 blockIdx + wave, + 4 gridDim, ...), lanes strided
// over Out; the sums are fp64 wave reductions.
__global__ __launch_bounds__(256) void rop_out_xent_kernel(long long B, int Out, const float *Z, const float *Y,
                                                           const int *idx, const float *RZ, float s, float *RdZ) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long b = (long long)blockIdx.x * 4 + wave; b < B; b += (long long)gridDim.x * 4) { // wave-uniform
    const float *z = Z + b * Out, *rz = RZ + b * Out;
    const float *y = Y + (idx ? (long long)idx[b] : b) * Out;
    float m = -INFINITY;
    for (int o = lane; o < Out; o += 64) m = fmaxf(m, z[o]);
    m = wave_max_f32(m);
    double se = 0.0, ys = 0.0, er = 0.0;
    for (int o = lane; o < Out; o += 64) {
      const float e = expf(z[o] - m);
      se += double(e);
      er += double(e) * double(rz[o]);
      ys += double(y[o]);
    }
    se = wave_sum_f64(se);
    const float rs = float(1.0 / se), dot = float(wave_sum_f64(er) / se), k = s * float(wave_sum_f64(ys));
    for (int o = lane; o < Out; o += 64) RdZ[b * Out + o] = k * (expf(z[o] - m) * rs) * (rz[o] - dot);
  }
}

// out = T1 + T2 (+ delta .* act''(A) .* RZ when delta is non-null)
__global__ __launch_bounds__(256) void rop_back_kernel(long long n, const float *T1, const float *T2, const float *delta,
                                                       const float *A, const float *RZ, int act, float *out) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float v = T1[e] + T2[e];
  if (delta) v += delta[e] * d2act_rt(act, A[e]) * RZ[e];
  out[e] = v;
}

// ---- Gauss-Newton product (Mlp::gnvp). R{Z} = T0 + T1 (T0 = A_prev V + v, T1 = R{A_prev} W; null for layer 0)
// is formed in the launch that consumes it and never stored. ----

// RA = act'(A) .* (T0 + T1)
__global__ __launch_bounds__(256) void gn_act_kernel(long long n, const float *A, const float *T0, const float *T1,
                                                     int act, float *RA, const int *abort) {
  if (abort && *abort) return;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float rz = T0[e];
  if (T1) rz += T1[e];
  RA[e] = dact_rt(act, A[e]) * rz;
}

// M = s act'(A)^2 .* (T0 + T1): the squared error's Hessian s I at the outputs A_L, pulled back to Z_L
__global__ __launch_bounds__(256) void gn_out_mse_kernel(long long n, const float *A, const float *T0,
                                                         const float *T1, int act, float s, float *M,
                                                         const int *abort) {
  if (abort && *abort) return;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float rz = T0[e];
  if (T1) rz += T1[e];
  const float d1 = dact_rt(act, A[e]);
  M[e] = s * (d1 * d1) * rz;
}

// M = s Ysum p .* (RZ - sum_k p_k RZ_k) with RZ = T0 + T1: rop_out_xent_kernel's row layout, sums and
// arithmetic (the cross-entropy's Hessian at the logits is the whole second-order term of that loss)
__global__ __launch_bounds__(256) void gn_out_xent_kernel(long long B, int Out, const float *Z, const float *Y,
                                                          const int *idx, const float *T0, const float *T1, float s,
                                                          float *M, const int *abort) {
  if (abort && *abort) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long b = (long long)blockIdx.x * 4 + wave; b < B; b += (long long)gridDim.x * 4) { // wave-uniform
    const float *z = Z + b * Out, *t0 = T0 + b * Out, *t1 = T1 ? T1 + b * Out : nullptr;
    const float *y = Y + (idx ? (long long)idx[b] : b) * Out;
    float m = -INFINITY;
    for (int o = lane; o < Out; o += 64) m = fmaxf(m, z[o]);
    m = wave_max_f32(m);
    double se = 0.0, ys = 0.0, er = 0.0;
    for (int o = lane; o < Out; o += 64) {
      const float e = expf(z[o] - m), rz = t1 ? t0[o] + t1[o] : t0[o];
      se += double(e);
      er += double(e) * double(rz);
      ys += double(y[o]);
    }
    se = wave_sum_f64(se);
    const float rs = float(1.0 / se), dot = float(wave_sum_f64(er) / se), k = s * float(wave_sum_f64(ys));
    for (int o = lane; o < Out; o += 64) {
      const float rz = t1 ? t0[o] + t1[o] : t0[o];
      M[b * Out + o] = k * (expf(z[o] - m) * rs) * (rz - dot);
    }
  }
}

} // namespace

void gn_act(hipStream_t s, long long n, const float *A, const float *T0, const float *T1, int act, float *RA,
            const int *abort) {
  if (n <= 0) return;
  hipLaunchKernelGGL(gn_act_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, n, A, T0, T1, act, RA, abort);
  LBF_KERNEL_CHECK();
}

void gn_out_mse(hipStream_t s, long long n, const float *A, const float *T0, const float *T1, int act,
                double inv_scale, float *M, const int *abort) {
  if (n <= 0) return;
  hipLaunchKernelGGL(gn_out_mse_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, n, A, T0, T1, act,
                     float(inv_scale), M, abort);
  LBF_KERNEL_CHECK();
}

void gn_out_xent(hipStream_t s, long long B, int Out, const float *Z, const float *Y, const int *idx, const float *T0,
                 const float *T1, double inv_scale, float *M, const int *abort) {
  if (B <= 0) return;
  hipLaunchKernelGGL(gn_out_xent_kernel, dim3(unsigned(std::min<long long>(cdiv(B, 4), 4096))), dim3(256), 0, s, B,
                     Out, Z, Y, idx, T0, T1, float(inv_scale), M, abort);
  LBF_KERNEL_CHECK();
}

void rop_act(hipStream_t s, long long n, const float *A, const float *RZ, int act, float *RA) {
  if (n <= 0) return;
  hipLaunchKernelGGL(rop_act_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, n, A, RZ, act, RA);
  LBF_KERNEL_CHECK();
}

void rop_out(hipStream_t s, long long B, int Out, const float *A, const float *Y, const int *idx, const float *RZ,
             int act, double inv_scale, float *RdZ) {
  if (B <= 0) return;
  hipLaunchKernelGGL(rop_out_kernel, dim3(unsigned(cdiv(B * Out, 256))), dim3(256), 0, s, B, Out, A, Y, idx, RZ, act,
                     float(inv_scale), RdZ);
  LBF_KERNEL_CHECK();
}

void rop_out_xent(hipStream_t s, long long B, int Out, const float *Z, const float *Y, const int *idx,
                  const float *RZ, double inv_scale, float *RdZ) {
  if (B <= 0) return;
  hipLaunchKernelGGL(rop_out_xent_kernel, dim3(unsigned(std::min<long long>(cdiv(B, 4), 4096))), dim3(256), 0, s, B,
                     Out, Z, Y, idx, RZ, float(inv_scale), RdZ);
  LBF_KERNEL_CHECK();
}

void rop_back(hipStream_t s, long long n, const float *T1, const float *T2, const float *delta, const float *A,
              const float *RZ, int act, float *out) {
  if (n <= 0) return;
  hipLaunchKernelGGL(rop_back_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, n, T1, T2, delta, A, RZ, act,
                     out);
  LBF_KERNEL_CHECK();
}

bool act_has_d2(int act) { return act == ACT_TANH || act == ACT_SIGMOID || act == ACT_ELU || act == ACT_SOFTPLUS; }

} // namespace lbf
