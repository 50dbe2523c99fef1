// Device-side evaluation of a classifier's outputs (gfx950, wave64): predicted and target class, accuracy,
// top-k, the data loss, the confusion matrix, softmax probabilities. One pass over the rows of the outputs
// Z [B][Out] that Mlp::forward stored (post-activation values of an MSE net, logits of a cross-entropy net).
//
// Replaces the host loop of UnifiedLauncher::evaluate (src/unified_launcher.hpp:154-199), which copies all
// B x Out outputs to the host and scans them there.
//
// Argmax rule (the reference's scan, not numpy's): best = 0, m = -1e20; for o = 0 .. Out-1: if z_o > m take it.
// So the lowest index wins a tie, a NaN never wins, and a row with nothing above -1e20 gives class 0.
// Top-k rule: rank of the target class t = #{o : z_o > z_t} + #{o < t : z_o == z_t}; the row counts when
// rank < k. For finite logits k = 1 equals pred == t. Rows holding a non-finite logit are outside the top-k
// contract (they are counted in rows and never fault: every index used is in [0, Out)).
//
// Layout: a row is taken by a group of G lanes, G = the power of two >= Out up to 64 (a wave takes 64 / G rows
// at once; above 64 outputs the 64 lanes stride over the row, re-reading it from L1 in each pass, as
// loss_xent_kernel does). Loads are unconditional from clamped addresses and masked afterwards. The loss is
// accumulated in fp64 per lane and summed per workgroup in a fixed order into one partial per workgroup; the three
// counts go to a per-workgroup table as well (ordinary stores, summed by the finishing launch: no contended
// atomics); the confusion matrix takes integer atomics, one per workgroup and non-empty cell (privatised in LDS up
// to 64 classes, global atomics per row above).
#include "eval_limbs.hpp"
#include "internal.hpp"
#include "kernels.hpp"
#include "wave.hpp"

#include <hip/hip_runtime.h>

#include <climits>

namespace lbf {

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_MAX_WG = 4096;
constexpr int MT_CONF_LDS_MAX = 64; // classes whose Out x Out table of 32-bit counts is privatised in LDS (16 KB)

template <int G> __device__ __forceinline__ int group_sum_i32(int v) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
template <int G> __device__ __forceinline__ double group_sum_f64(double v) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
template <int G> __device__ __forceinline__ float group_max_f32(float v) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
// The scan's winner over the group: the larger value, the lower index among equals. (-inf, INT_MAX) stands for
// "nothing above -1e20 here"; the order is total (no NaN reaches it), so every lane ends with the same pair.
template <int G> __device__ __forceinline__ int group_argmax(float v, int i) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) {
    const float pv = __shfl_xor(v, o);
    const int pi = __shfl_xor(i, o);
    if (pv > v || (pv == v && pi < i)) {
      v = pv;
      i = pi;
    }
  }
  return i == INT_MAX ? 0 : i;
}
// one step of the scan on a lane's own (ascending) elements
__device__ __forceinline__ void scan_take(float z, int o, bool ok, float &bv, int &bi) {
  if (ok && double(z) > -1e20 && z > bv) {
    bv = z;
    bi = o;
  }
}

template <int G>
__global__ __launch_bounds__(MT_THREADS) void metrics_kernel(const MetricsArgs a) {
  extern __shared__ unsigned conf_lds[]; // Out * Out when a.conf_mode == 1
  __shared__ double scratch[MT_THREADS / 64];
  __shared__ int cscratch[3][MT_THREADS / 64];
  constexpr int RPB = MT_THREADS / G; // rows per block and step
  // Out <= G below 64 lanes (metrics() picks G so): each pass over the row is one step, and the compiler keeps the
  // lane's z and y in registers across the passes instead of re-reading them
  constexpr bool ONE = G < 64;
  const int t = threadIdx.x, gl = t % G, grp = t / G;
  const int Out = a.Out;
  const bool xent = a.loss == LOSS_XENT;
  const bool have_y = a.Y != nullptr;
  const bool want_se = xent && (have_y || a.proba);
  if (a.conf_mode == 1) {
    for (int c = t; c < Out * Out; c += MT_THREADS) conf_lds[c] = 0u;
    __syncthreads();
  }
  double acc = 0.0;
  int n_rows = 0, n_correct = 0, n_topk = 0;
  // block-uniform trip count: the shuffles below always run with every lane of the wave
  for (long long r0 = (long long)blockIdx.x * RPB; r0 < a.B; r0 += (long long)gridDim.x * RPB) {
    const long long row = r0 + grp;
    const bool live = row < a.B;
    const long long rc = live ? row : a.B - 1;
    const float *z = a.Z + rc * Out;
    const float *y = have_y ? a.Y + (a.idx ? (long long)a.idx[rc] : rc) * Out : a.Z + rc * Out;
    // pass 1: the two scans and the row maximum
    float pbv = -INFINITY, tbv = -INFINITY, mx = -INFINITY;
    int pbi = INT_MAX, tbi = INT_MAX;
    for (int o0 = 0; ONE ? o0 < 1 : o0 < Out; o0 += G) {
      const int o = o0 + gl, oc = o < Out ? o : Out - 1;
      const bool ok = o < Out;
      const float zo = z[oc], yo = y[oc];
      scan_take(zo, o, ok, pbv, pbi);
      scan_take(yo, o, ok, tbv, tbi);
      mx = fmaxf(mx, ok ? zo : -INFINITY);
    }
    const int pred = group_argmax<G>(pbv, pbi);
    const int tgt = have_y ? group_argmax<G>(tbv, tbi) : 0;
    if (want_se) mx = group_max_f32<G>(mx);
    // pass 2: rank of the target class, the softmax denominator, the squared error
    const float zt = z[tgt];
    int rank = 0;
    double se = 0.0;
    for (int o0 = 0; ONE ? o0 < 1 : o0 < Out; o0 += G) {
      const int o = o0 + gl, oc = o < Out ? o : Out - 1;
      const bool ok = o < Out;
      const float zo = z[oc], yo = y[oc];
      rank += (ok && (zo > zt || (zo == zt && o < tgt))) ? 1 : 0;
      if (want_se) se += ok ? double(expf(zo - mx)) : 0.0;
      if (!xent && have_y && ok && live) {
        const float d = zo - yo;
        acc += double(d) * double(d);
      }
    }
    if (have_y) rank = group_sum_i32<G>(rank);
    if (want_se) {
      const float sef = float(group_sum_f64<G>(se));
      const float lg = logf(sef);
      // pass 3: the cross-entropy terms 2 y (lse - z), lse - z = (m - z) + log(se); the probabilities
      for (int o0 = 0; ONE ? o0 < 1 : o0 < Out; o0 += G) {
        const int o = o0 + gl, oc = o < Out ? o : Out - 1;
        const bool ok = o < Out;
        const float zo = z[oc], yo = y[oc];
        if (ok && live) {
          if (have_y) acc += 2.0 * double(yo) * double((mx - zo) + lg);
          if (a.proba) a.proba[row * Out + o] = expf(zo - mx) / sef;
        }
      }
    }
    if (gl == 0 && live) {
      ++n_rows;
      if (a.pred) a.pred[row] = pred;
      if (have_y) {
        n_correct += pred == tgt ? 1 : 0;
        n_topk += rank < a.k ? 1 : 0;
        if (a.conf_mode == 1) atomicAdd(&conf_lds[tgt * Out + pred], 1u);
        else if (a.conf_mode == 2) atomicAdd(&a.conf[(long long)tgt * Out + pred], 1ull);
      }
    }
  }
  // workgroup totals: the loss partial in a fixed order, the counts as integers
  const int lane = t & 63, wave = t >> 6;
  const double wacc = wave_sum_f64(acc);
  const int w_rows = group_sum_i32<64>(n_rows), w_cor = group_sum_i32<64>(n_correct), w_top = group_sum_i32<64>(n_topk);
  if (lane == 0) {
    scratch[wave] = wacc;
    cscratch[0][wave] = w_rows;
    cscratch[1][wave] = w_cor;
    cscratch[2][wave] = w_top;
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    int c0 = 0, c1 = 0, c2 = 0;
    for (int w = 0; w < MT_THREADS / 64; ++w) {
      s += scratch[w];
      c0 += cscratch[0][w];
      c1 += cscratch[1][w];
      c2 += cscratch[2][w];
    }
    a.partials[blockIdx.x] = s;
    a.cpart[3 * blockIdx.x + 0] = unsigned(c0);
    a.cpart[3 * blockIdx.x + 1] = unsigned(c1);
    a.cpart[3 * blockIdx.x + 2] = unsigned(c2);
  }
  if (a.conf_mode == 1) {
    for (int c = t; c < Out * Out; c += MT_THREADS) {
      const unsigned v = conf_lds[c];
      if (v) atomicAdd(&a.conf[c], (unsigned long long)v);
    }
  }
}

// One workgroup: the loss partials of every chunk in table order (fixed: thread-strided, wave_sum_f64, the waves
// in order) -> sum[0] and the fp32 (hi, lo) words; the workgroups' three counts summed as integers (exact in any
// order); every count and confusion cell -> three 16-bit limbs as floats (eval_limbs.hpp).
__global__ __launch_bounds__(MT_THREADS) void metrics_finish_kernel(const double *partials, const unsigned *cpart,
                                                                    int npart, const unsigned long long *conf,
                                                                    int nconf, double *sum, float *words) {
  __shared__ double scratch[MT_THREADS / 64];
  __shared__ unsigned long long cscratch[3][MT_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double s = 0.0;
  unsigned long long c[3] = {0ull, 0ull, 0ull};
  for (int r = t; r < npart; r += MT_THREADS) {
    s += partials[r];
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] += cpart[3 * r + j];
  }
  s = wave_sum_f64(s);
#pragma unroll
  for (int j = 0; j < 3; ++j)
    for (int o = 1; o < 64; o <<= 1) c[j] += __shfl_xor(c[j], o);
  if (lane == 0) {
    scratch[wave] = s;
#pragma unroll
    for (int j = 0; j < 3; ++j) cscratch[j][wave] = c[j];
  }
  __syncthreads();
  if (t == 0) {
    double x = 0.0;
    for (int w = 0; w < MT_THREADS / 64; ++w) x += scratch[w];
    sum[0] = x;
    const float hi = float(x);
    words[0] = hi;
    words[1] = float(x - double(hi));
  }
  if (t < 3) {
    unsigned long long v = 0ull;
    for (int w = 0; w < MT_THREADS / 64; ++w) v += cscratch[t][w];
    eval_limbs_split(v, words + 2 + kEvalLimbs * t);
  }
  for (int q = t; q < nconf; q += MT_THREADS) eval_limbs_split(conf[q], words + 2 + kEvalLimbs * (3 + q));
}

template <int G> void launch_metrics(hipStream_t s, const MetricsArgs &a, int nwg, size_t lds) {
  hipLaunchKernelGGL(metrics_kernel<G>, dim3(unsigned(nwg)), dim3(MT_THREADS), lds, s, a);
}

int group_width(int Out) {
  int g = 1;
  while (g < Out && g < 64) g <<= 1;
  return g;
}

} // namespace

int metrics_nwg(long long B, int Out) {
  const long long rpb = MT_THREADS / group_width(Out);
  const long long w = cdiv(B, rpb); // one step per workgroup up to the cap, then a grid-stride loop
  return int(w < 1 ? 1 : (w > MT_MAX_WG ? MT_MAX_WG : w));
}

int metrics_conf_mode(int Out, bool want) { return !want ? 0 : (Out <= MT_CONF_LDS_MAX ? 1 : 2); }

void metrics(hipStream_t s, const MetricsArgs &a) {
  LBF_REQUIRE(a.B > 0 && a.Out > 0 && a.Z && a.partials && a.cpart, "metrics: bad argument");
  LBF_REQUIRE(a.k >= 1 && a.k <= a.Out, "metrics: k outside 1..Out");
  LBF_REQUIRE(a.conf_mode == 0 || (a.conf && a.Y), "metrics: confusion matrix without targets");
  LBF_REQUIRE(a.conf_mode != 1 || a.Out <= MT_CONF_LDS_MAX, "metrics: LDS confusion table too wide");
  const int nwg = metrics_nwg(a.B, a.Out);
  const size_t lds = a.conf_mode == 1 ? size_t(a.Out) * a.Out * sizeof(unsigned) : 0;
  switch (group_width(a.Out)) {
  case 1: launch_metrics<1>(s, a, nwg, lds); break;
  case 2: launch_metrics<2>(s, a, nwg, lds); break;
  case 4: launch_metrics<4>(s, a, nwg, lds); break;
  case 8: launch_metrics<8>(s, a, nwg, lds); break;
  case 16: launch_metrics<16>(s, a, nwg, lds); break;
  case 32: launch_metrics<32>(s, a, nwg, lds); break;
  default: launch_metrics<64>(s, a, nwg, lds); break;
  }
  LBF_KERNEL_CHECK();
}

void metrics_finish(hipStream_t s, const double *partials, const unsigned *cpart, int npart,
                    const unsigned long long *conf, int nconf, double *sum, float *words) {
  hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(MT_THREADS), 0, s, partials, cpart, npart, conf, nconf, sum,
                     words);
  LBF_KERNEL_CHECK();
}

} // namespace lbf
