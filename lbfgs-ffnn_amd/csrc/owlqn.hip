// Orthant-wise sweeps of OWL-QN (kernels.hpp has the contract; run_owlqn drives them).
//
// Both sweeps use the block map of the w.w partials (kernels.hpp WwPart): workgroup b owns elements
// [b E, (b + 1) E), E = ww_block_elems(n), so the grid and every partial table have ww_partials_n(n) entries, a
// function of n only, and the trial's x+.x+ table is the WwPart that loss_only takes. Every sum has a fixed order:
// thread-private fp64 accumulation in loop order, wave_sum_f64, then ((v0 + v1) + v2) + v3; the one-workgroup
// finisher sums each table with ww_sum's pattern (so its w.w is the word sse_loss forms from the same table). No
// atomics.
//
// Pointers: 4-byte aligned. E is a multiple of 4, so when every vector of a launch has the same
// offset from a 16-byte boundary each workgroup has the same scalar head (`lead` elements), a float4 body and a
// scalar tail of at most three elements; with mixed offsets the whole sweep is scalar.
//
// Which coordinates carry the penalty is a per-layer table of the bias ranges (OwlCoef), not an n-float mask: a
// workgroup whose elements touch no bias range, nearly all of them, takes the coefficient as a constant.
#include "internal.hpp"
#include "kernels.hpp"
#include "wave.hpp"

#include <algorithm>
#include <cmath>

namespace lbf {

namespace {

struct OwlMap {
  long long n, E;
  int vec, lead; // vec: float4 body after `lead` scalar elements of each workgroup
  OwlCoef coef;
};

template <class... P> OwlMap make_map(long long n, const OwlCoef &coef, P... ptrs) {
  const int lead = common_lead(ptrs...);
  return OwlMap{n, ww_block_elems(n), lead >= 0 ? 1 : 0, lead >= 0 ? lead : 0, coef};
}

// The element ranges of workgroup blockIdx.x: [e0, a0) and [a1, e1) one at a time, [a0, a1) as nv float4 groups.
struct OwlBlock {
  long long e0, e1, a0, a1, nv;
  bool mixed; // some element may lie in an unpenalised range
};
__device__ __forceinline__ OwlBlock owl_block(const OwlMap &m) {
  OwlBlock b;
  b.e0 = (long long)blockIdx.x * m.E;
  b.e1 = b.e0 + m.E < m.n ? b.e0 + m.E : m.n;
  b.a0 = b.a1 = b.e1;
  b.nv = 0;
  if (m.vec) {
    b.a0 = b.e0 + m.lead < b.e1 ? b.e0 + m.lead : b.e1;
    b.nv = (b.e1 - b.a0) / 4;
    b.a1 = b.a0 + 4 * b.nv;
  }
  b.mixed = false;
  for (int i = 0; i < m.coef.nfree; ++i) b.mixed = b.mixed || (m.coef.f0[i] < b.e1 && m.coef.f1[i] > b.e0);
  return b;
}
__device__ __forceinline__ bool owl_penalised(const OwlMap &m, const OwlBlock &b, long long e) {
  if (!b.mixed) return true;
  bool fr = false;
  for (int i = 0; i < m.coef.nfree; ++i) fr = fr || (e >= m.coef.f0[i] && e < m.coef.f1[i]);
  return !fr;
}
// scalar element j of the block (j < scalar count): the head, then the tail; without a float4 body every element
__device__ __forceinline__ long long owl_nscalar(const OwlMap &m, const OwlBlock &b) {
  return m.vec ? (b.a0 - b.e0) + (b.e1 - b.a1) : b.e1 - b.e0;
}
__device__ __forceinline__ long long owl_scalar(const OwlMap &m, const OwlBlock &b, long long j) {
  if (!m.vec) return b.e0 + j;
  return j < b.a0 - b.e0 ? b.e0 + j : b.a1 + (j - (b.a0 - b.e0));
}

// The pseudo-gradient of f + c |x| at one coordinate; each value is one fp32 add.
__device__ __forceinline__ float owl_pg(float x, float g, float c) {
  const float gp = __fadd_rn(g, c), gm = __fsub_rn(g, c);
  if (x > 0.0f) return gp;
  if (x < 0.0f) return gm;
  if (gm > 0.0f) return gm;
  if (gp < 0.0f) return gp;
  return 0.0f;
}

struct PseudoAcc {
  double pp = 0.0, ax = 0.0, nz = 0.0;
};
__device__ __forceinline__ float pseudo_one(float x, float g, float c, bool pen, PseudoAcc &q) {
  const float p = owl_pg(x, g, pen ? c : 0.0f);
  q.pp += double(p) * double(p);
  if (pen) {
    q.ax += fabs(double(x));
    q.nz += x == 0.0f ? 1.0 : 0.0;
  }
  return p;
}

// tab: [pg.pg | sum |x| over the penalised | zeros among the penalised], nb words each
__global__ __launch_bounds__(256) void owl_pseudo_kernel(OwlMap m, const float *x, const float *g, float *pg,
                                                         double *tab, int nb) {
  __shared__ double wv[4];
  const OwlBlock b = owl_block(m);
  const float c = m.coef.c;
  PseudoAcc q;
  for (long long v = threadIdx.x; v < b.nv; v += 256) {
    const long long e = b.a0 + 4 * v;
    const f32x4 xv = *reinterpret_cast<const f32x4 *>(x + e), gv = *reinterpret_cast<const f32x4 *>(g + e);
    f32x4 pv;
    pv.x = pseudo_one(xv.x, gv.x, c, owl_penalised(m, b, e), q);
    pv.y = pseudo_one(xv.y, gv.y, c, owl_penalised(m, b, e + 1), q);
    pv.z = pseudo_one(xv.z, gv.z, c, owl_penalised(m, b, e + 2), q);
    pv.w = pseudo_one(xv.w, gv.w, c, owl_penalised(m, b, e + 3), q);
    *reinterpret_cast<f32x4 *>(pg + e) = pv;
  }
  for (long long j = threadIdx.x; j < owl_nscalar(m, b); j += 256) {
    const long long e = owl_scalar(m, b, j);
    pg[e] = pseudo_one(x[e], g[e], c, owl_penalised(m, b, e), q);
  }
  const double pp = block_sum_all(q.pp, wv), ax = block_sum_all(q.ax, wv), nz = block_sum_all(q.nz, wv);
  if (threadIdx.x == 0) {
    tab[blockIdx.x] = pp;
    tab[size_t(nb) + blockIdx.x] = ax;
    tab[2 * size_t(nb) + blockIdx.x] = nz;
  }
}

struct TrialAcc {
  double ww = 0.0, ax = 0.0, dec = 0.0, nz = 0.0;
};
// The direction's sign test against pg, the step, the projection onto the orthant of x (of -pg where x == 0).
__device__ __forceinline__ float trial_one(float x, float d, float p, float alpha, bool pen, int dneg, TrialAcc &q) {
  if (dneg) d = -p; // no stored pairs: the direction is -pg
  // a free coordinate takes the plain step; a penalised one the sign test and the projection
  const bool keep = !pen || (d > 0.0f && p < 0.0f) || (d < 0.0f && p > 0.0f); // d p < 0 by signs, not a rounded product
  const float t = __builtin_fmaf(alpha, keep ? d : 0.0f, x);
  const bool up = x > 0.0f || (x == 0.0f && p < 0.0f), down = x < 0.0f || (x == 0.0f && p > 0.0f);
  const float xn = (!pen || (up && t > 0.0f) || (down && t < 0.0f)) ? t : 0.0f;
  q.ww += double(xn) * double(xn);
  q.dec += double(p) * (double(xn) - double(x));
  if (pen) {
    q.ax += fabs(double(xn));
    q.nz += xn == 0.0f ? 1.0 : 0.0;
  }
  return xn;
}

// tab: [x+.x+ (the WwPart of x+) | sum |x+| over the penalised | pg.(x+ - x) | zeros among the penalised]
__global__ __launch_bounds__(256) void owl_trial_kernel(OwlMap m, const float *x, const float *d, const float *pg,
                                                        float alpha, int dneg, float *xn, double *tab, int nb) {
  __shared__ double wv[4];
  const OwlBlock b = owl_block(m);
  TrialAcc q;
  for (long long v = threadIdx.x; v < b.nv; v += 256) {
    const long long e = b.a0 + 4 * v;
    const f32x4 xv = *reinterpret_cast<const f32x4 *>(x + e), dv = *reinterpret_cast<const f32x4 *>(d + e);
    const f32x4 pv = *reinterpret_cast<const f32x4 *>(pg + e);
    f32x4 o;
    o.x = trial_one(xv.x, dv.x, pv.x, alpha, owl_penalised(m, b, e), dneg, q);
    o.y = trial_one(xv.y, dv.y, pv.y, alpha, owl_penalised(m, b, e + 1), dneg, q);
    o.z = trial_one(xv.z, dv.z, pv.z, alpha, owl_penalised(m, b, e + 2), dneg, q);
    o.w = trial_one(xv.w, dv.w, pv.w, alpha, owl_penalised(m, b, e + 3), dneg, q);
    *reinterpret_cast<f32x4 *>(xn + e) = o;
  }
  for (long long j = threadIdx.x; j < owl_nscalar(m, b); j += 256) {
    const long long e = owl_scalar(m, b, j);
    xn[e] = trial_one(x[e], d[e], pg[e], alpha, owl_penalised(m, b, e), dneg, q);
  }
  const double ww = block_sum_all(q.ww, wv), ax = block_sum_all(q.ax, wv), dec = block_sum_all(q.dec, wv),
               nz = block_sum_all(q.nz, wv);
  if (threadIdx.x == 0) {
    tab[blockIdx.x] = ww;
    tab[size_t(nb) + blockIdx.x] = ax;
    tab[2 * size_t(nb) + blockIdx.x] = dec;
    tab[3 * size_t(nb) + blockIdx.x] = nz;
  }
}

// One workgroup: table t summed in ww_sum's order into st[slot[t]]; the |x| sum times l1 is the penalty.
struct OwlFin {
  int ntab = 0;
  int slot[4] = {};
};
__global__ __launch_bounds__(256) void owl_fin_kernel(const double *tab, int nb, OwlFin f, double l1, double *st) {
  __shared__ double wv[4];
  for (int t = 0; t < f.ntab; ++t) {
    const double q = ww_sum_wave(tab + size_t(t) * nb, nb, threadIdx.x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = q;
    __syncthreads();
    if (threadIdx.x == 0) {
      const double v = ww_sum_fin(wv);
      st[f.slot[t]] = f.slot[t] == OWL_L1 ? l1 * v : v;
    }
  }
}

} // namespace

int owl_table_words(long long n) { return 4 * ww_partials_n(n); }

void owl_pseudo(hipStream_t s, const OwlArgs &a) {
  LBF_REQUIRE(a.n > 0 && a.x && a.g && a.out && a.tab && a.st, "owl_pseudo: null argument");
  const int nb = ww_partials_n(a.n);
  hipLaunchKernelGGL(owl_pseudo_kernel, dim3(unsigned(nb)), dim3(256), 0, s, make_map(a.n, a.coef, a.x, a.g, a.out),
                     a.x, a.g, a.out, a.tab, nb);
  LBF_KERNEL_CHECK();
}

void owl_pseudo_finish(hipStream_t s, const OwlArgs &a) {
  const int nb = ww_partials_n(a.n);
  OwlFin f;
  f.ntab = 3;
  f.slot[0] = OWL_PGPG;
  f.slot[1] = OWL_L1;
  f.slot[2] = OWL_ZEROS;
  hipLaunchKernelGGL(owl_fin_kernel, dim3(1), dim3(256), 0, s, a.tab, nb, f, a.l1, a.st);
  LBF_KERNEL_CHECK();
}

void owl_trial(hipStream_t s, const OwlArgs &a) {
  LBF_REQUIRE(a.n > 0 && a.x && a.pg && a.out && a.tab && a.st, "owl_trial: null argument");
  const int nb = ww_partials_n(a.n);
  const float *d = a.d ? a.d : a.pg; // no direction: d = -pg, formed from pg in registers
  hipLaunchKernelGGL(owl_trial_kernel, dim3(unsigned(nb)), dim3(256), 0, s, make_map(a.n, a.coef, a.x, d, a.pg, a.out),
                     a.x, d, a.pg, a.alpha, a.d ? 0 : 1, a.out, a.tab, nb);
  LBF_KERNEL_CHECK();
}

void owl_trial_finish(hipStream_t s, const OwlArgs &a) {
  const int nb = ww_partials_n(a.n);
  OwlFin f;
  f.ntab = 4;
  f.slot[0] = OWL_WW;
  f.slot[1] = OWL_L1;
  f.slot[2] = OWL_DEC;
  f.slot[3] = OWL_ZEROS;
  hipLaunchKernelGGL(owl_fin_kernel, dim3(1), dim3(256), 0, s, a.tab, nb, f, a.l1, a.st);
  LBF_KERNEL_CHECK();
}

} // namespace lbf
