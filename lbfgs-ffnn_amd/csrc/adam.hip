// The Adam / AdamW step in one sweep (gfx950, wave64; kernels.hpp has the contract, solve_adam.cpp drives it,
// DESIGN §20). Per element, every operation rounded once and none contracted:
//   gi = g c;  m = b1 m + a1 gi;  v = b2 v + a2 (gi gi);  w = w decay - step (m / (sqrt(v) rbc2 + eps))
// Four reads and three writes of n floats; no atomics, no workgroup waits on another.
//
// c, the global-norm clip, is derived by every thread from the same device double (the evaluation's g.g), so all
// workgroups scale by the same bits and no host read sits between the evaluation and the step.
//
// Pointers: 4-byte aligned. When g, m, v and w share their offset from a 16-byte boundary a scalar
// head brings them to it and the body runs on float4, the tail is scalar again; with mixed offsets the whole sweep
// is scalar. One float4 group or one scalar element per thread.
//
// Part of vec.hip's translation unit (a further code object costs the default bench.py line); it
// compiles alone too.
#include "internal.hpp"
#include "kernels.hpp"
#include "wave.hpp"

#include <algorithm>

namespace lbf {

namespace {

// Elements [0, head) and [tail0, n) one at a time, [head, tail0) as nvec float4 groups.
struct AdamSpan {
  long long n, head, nvec, tail0;
};

struct AdamElem {
  float m, v, w;
};
// One element. The arithmetic is written as plain operators under contract(off): the compiler's __fmul_rn /
// __fadd_rn / __fsub_rn / __fdiv_rn are these same operators (and so could be contracted into an fma where the
// pragma is missing), and its __fsqrt_rn is the native 1-ulp square root, while sqrtf and / are the correctly
// rounded ones that a numpy restatement reproduces bit for bit.
__device__ __forceinline__ AdamElem adam_one(const AdamCoef &k, float c, float g, float m, float v, float w) {
#pragma clang fp contract(off)
  const float gi = g * c;
  const float mn = (k.b1 * m) + (k.a1 * gi);
  const float vn = (k.b2 * v) + (k.a2 * (gi * gi));
  const float den = (sqrtf(vn) * k.rbc2) + k.eps;
  return AdamElem{mn, vn, (w * k.decay) - (k.step * (mn / den))};
}

__global__ __launch_bounds__(256) void adam_step_kernel(AdamSpan sp, AdamCoef k, const float *g, float *m, float *v,
                                                        float *w, const double *gg, AdamLoss ls) {
#pragma clang fp contract(off)
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid == 0 && ls.scal) { // SGD's epoch_loss_acc, in fp64, and the step's entry of the loss trace
    const double loss = ls.scal[SC_LOSS];
    *ls.esum = *ls.esum + (loss * ls.rows);
    if (ls.trace) *ls.trace = loss;
  }
  float c = 1.0f;
  if (gg && k.clip > 0.0f) {
    const float nrm = sqrtf(float(*gg));
    if (nrm > k.clip) c = k.clip / nrm;
  }
  if (gid < sp.nvec) {
    const long long e = sp.head + 4 * gid;
    const f32x4 gv = *reinterpret_cast<const f32x4 *>(g + e);
    f32x4 mv = *reinterpret_cast<const f32x4 *>(m + e), vv = *reinterpret_cast<const f32x4 *>(v + e),
          wv = *reinterpret_cast<const f32x4 *>(w + e);
    const AdamElem r0 = adam_one(k, c, gv.x, mv.x, vv.x, wv.x), r1 = adam_one(k, c, gv.y, mv.y, vv.y, wv.y),
                   r2 = adam_one(k, c, gv.z, mv.z, vv.z, wv.z), r3 = adam_one(k, c, gv.w, mv.w, vv.w, wv.w);
    mv = f32x4{r0.m, r1.m, r2.m, r3.m};
    vv = f32x4{r0.v, r1.v, r2.v, r3.v};
    wv = f32x4{r0.w, r1.w, r2.w, r3.w};
    *reinterpret_cast<f32x4 *>(m + e) = mv;
    *reinterpret_cast<f32x4 *>(v + e) = vv;
    *reinterpret_cast<f32x4 *>(w + e) = wv;
  }
  if (gid < sp.head + (sp.n - sp.tail0)) {
    const long long e = gid < sp.head ? gid : sp.tail0 + (gid - sp.head);
    const AdamElem r = adam_one(k, c, g[e], m[e], v[e], w[e]);
    m[e] = r.m;
    v[e] = r.v;
    w[e] = r.w;
  }
}

} // namespace

void adam_step(hipStream_t s, long long n, const AdamCoef &k, const float *g, float *m, float *v, float *w,
               const double *gg, const AdamLoss &ls) {
  if (n <= 0 && !ls.scal) return;
  n = std::max(0LL, n);
  const int lead = common_lead(g, m, v, w);
  AdamSpan sp{n, n, 0, n};
  if (lead >= 0) {
    sp.head = std::min<long long>(n, lead);
    sp.nvec = (n - sp.head) / 4;
    sp.tail0 = sp.head + 4 * sp.nvec;
  }
  const long long threads = std::max<long long>(1, std::max(sp.nvec, sp.head + (n - sp.tail0)));
  hipLaunchKernelGGL(adam_step_kernel, dim3(unsigned(cdiv(threads, 256))), dim3(256), 0, s, sp, k, g, m, v, w, gg, ls);
  LBF_KERNEL_CHECK();
}

} // namespace lbf
