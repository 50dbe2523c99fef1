// The evaluation's reductions and the scalars they end in (gfx950, wave64): partial-table row sums, split-K slab
// reductions, reduce_all with its finisher, and the one-workgroup tails that write the loss and the dots; fixed order.
//
// Replaces: sum_rows_kernel (src/cuda/kernels.cuh:136-153) and the cublasSdot / Snrm2 calls with host pointer
// mode behind every loss and gradient norm (kernels.cuh:28-50, each scalar a blocking device->host copy).
//
// Implements (kernels.hpp): reduce_rows, fold_rows, reduce_slabs, fwd_reduce_act, reduce_all, sse_loss,
// eval_status, pack_hilo, eval_tail, sse_pack.
#include "act.hpp"
#include "internal.hpp"
#include "kernels.hpp"
#include "wave.hpp"

namespace lbf {

// ---------------------------------------------------------------------------------------------
// reduce_rows: out[c] = sum_r P[r][c]   (one wave per column, lane-strided then butterfly)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reduce_rows_kernel(const double *P, int nrows, int ncols, double *out) {
  const int col = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (col >= ncols) return;
  double s = 0.0;
  for (int r = lane; r < nrows; r += 64) s += P[(long long)r * ncols + col];
  s = wave_sum_f64(s);
  if (lane == 0) out[col] = s;
}

void reduce_rows(hipStream_t s, const double *P, int nrows, int ncols, double *out) {
  if (ncols <= 0) return;
  hipLaunchKernelGGL(reduce_rows_kernel, dim3((ncols + 3) / 4), dim3(256), 0, s, P, nrows, ncols, out);
  LBF_KERNEL_CHECK();
}

// ---------------------------------------------------------------------------------------------
// fold_rows: out[j][c] = sum_{r in group j} P[r][c]; group j = rows [j*per, (j+1)*per). One block per
// (64-column group, row group): lane = column (coalesced 512-B row segments), wave w takes rows
// w, w+4, ... of the group, the four wave sums are added in a fixed order. Used to shrink a tall
// partial table (the Gram sweep's [nwg][6m+6] at large n) before a single-workgroup consumer.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fold_rows_kernel(const double *P, int nrows, int ncols, int per, double *out) {
  __shared__ double part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int r0 = blockIdx.y * per, r1 = min(nrows, r0 + per);
  double s = 0.0;
  if (c < ncols) {
    for (int r = r0 + wave; r < r1; r += 4 * 8) { // eight independent loads in flight per lane
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = P[(long long)min(r + 4 * u, r1 - 1) * ncols + c]; // clamped: no per-load branch
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (r + 4 * u < r1) s += v[u];
    }
  }
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < ncols)
    out[(long long)blockIdx.y * ncols + c] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

int fold_rows(hipStream_t s, const double *P, int nrows, int ncols, int groups, double *out) {
  const int per = int(cdiv(nrows, groups));
  const int g = int(cdiv(nrows, per));
  hipLaunchKernelGGL(fold_rows_kernel, dim3(unsigned(cdiv(ncols, 64)), unsigned(g)), dim3(256), 0, s, P, nrows,
                     ncols, per, out);
  LBF_KERNEL_CHECK();
  return g;
}

// ---------------------------------------------------------------------------------------------
// split-K slab reduction -> flat gradient segment
// ---------------------------------------------------------------------------------------------
// Block = CW columns x (256/CW) split stripes; each thread sums its stripe, stripes combine in LDS in
// a fixed order. CW = 64 for few splits (coalesced 256-B rows), 16 when splits are many (more
// parallelism per column for the tall-and-thin slabs of small layers).
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const float *slab, int splits, long long stride,
                                                           long long count, int cw, float *grad, const int *abort,
                                                           double scale) {
  if (abort && *abort) return;
  __shared__ double part[256];
  const int t = threadIdx.x;
  const int nst = 256 / cw;
  const long long col = (long long)blockIdx.x * cw + (t % cw);
  const int stripe = t / cw;
  double s = 0.0;
  if (col < count)
    for (int k = stripe; k < splits; k += nst) s += double(slab[k * stride + col]);
  part[t] = s;
  __syncthreads();
  if (stripe == 0 && col < count) {
    double r = 0.0;
    for (int q = 0; q < nst; ++q) r += part[q * cw + t];
    grad[col] = float(r * scale); // scale == 1: exact
  }
}

template <bool XACT> // XACT: all seven activation bodies (act.hpp), else the four
__global__ __launch_bounds__(256) void fwd_reduce_act_kernel(const float *slab, int splits, long long stride, int M,
                                                             int N, const float *bias, int act, float *out,
                                                             const int *abort) {
  if (abort && *abort) return;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)M * N) return;
  float v[8];
  float acc = 0.0f;
  int k = 0;
  for (; k + 8 <= splits; k += 8) { // independent loads in flight, summed in split order
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = slab[(long long)(k + u) * stride + e];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; k < splits; ++k) acc += slab[(long long)k * stride + e];
  const int n = int(e % N);
  const float z = acc + (bias ? bias[n] : 0.0f);
  out[e] = XACT ? act_rt(act, z) : act_rt4(act, z);
}

void fwd_reduce_act(hipStream_t s, const float *slab, int splits, long long stride, int M, int N, const float *bias,
                    int act, float *out, const int *abort) {
  const long long n = (long long)M * N;
  hipLaunchKernelGGL(act_in_heads(act) ? fwd_reduce_act_kernel<false> : fwd_reduce_act_kernel<true>,
                     dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, slab, splits, stride, M, N, bias, act, out, abort);
  LBF_KERNEL_CHECK();
}

void reduce_slabs(hipStream_t s, const float *slab, int splits, long long stride, long long count, float *grad,
                  const int *abort, double scale) {
  const int cw = splits > 64 ? 16 : 64;
  hipLaunchKernelGGL(reduce_slabs_kernel, dim3(unsigned(cdiv(count, cw))), dim3(256), 0, s, slab, splits, stride,
                     count, cw, grad, abort, scale);
  LBF_KERNEL_CHECK();
}

// ---------------------------------------------------------------------------------------------
// reduce_all: block = 64 columns x 4 split stripes (each stripe row a 256-B coalesced read).
// ---------------------------------------------------------------------------------------------
// Final value of one gradient column (+ its dot contributions). Lanes of wave 0 only.
__device__ __forceinline__ void ra_column(const RedAllArgs &a, const RedSeg &S, int cg, long long col, bool live,
                                          double colsum) {
  const int lane = threadIdx.x & 63;
  double d0 = 0.0, d1 = 0.0, d2 = 0.0;
  if (live) {
    const long long e = S.goff + col;
    float gv = S.splits > 0 ? float(colsum) : a.G[e];
    const float wv = (a.w && (a.dots || (a.l2 && a.lambda != 0.0))) ? a.w[e] : 0.0f;
    if (a.l2 && a.lambda != 0.0) gv = gv + float(a.lambda) * wv; // finalize_kernel's update
    if (a.dots) {
      d0 = double(gv) * double(gv);
      if (a.p) d1 = double(gv) * double(a.p[e]);
      d2 = double(wv) * double(wv);
    }
    if (S.splits > 0 || (a.l2 && a.lambda != 0.0)) a.G[e] = gv;
  }
  if (a.dots) {
    d0 = wave_sum_f64(d0);
    d1 = wave_sum_f64(d1);
    d2 = wave_sum_f64(d2);
    if (lane == 0) {
      a.partials[cg * 3 + 0] = d0;
      a.partials[cg * 3 + 1] = d1;
      a.partials[cg * 3 + 2] = d2;
    }
  }
}

// Segments reduced in one pass (parts == 1) take RA_GPB column groups per block, four columns per lane:
// every load of the block (slab values, then the operands of ra_columns) is issued before its first use,
// and a quarter of the blocks of one group each (a 535,818-parameter gradient was 8,372 blocks, several
// rounds per CU).
template <int J>
__device__ __forceinline__ void ra_columns(const RedAllArgs &a, const RedSeg &S, int cg0, long long cgl0,
                                           const double (&colsum)[J]) {
  const int lane = threadIdx.x & 63;
  const bool need_w = a.w && (a.dots || (a.l2 && a.lambda != 0.0));
  const bool lam = a.l2 && a.lambda != 0.0;
  long long e[J];
  bool live[J];
  float gv[J], wv[J], pv[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const long long col = (cgl0 + j) * RA_COLS + lane;
    live[j] = col < S.count;
    e[j] = S.goff + (live[j] ? col : 0);
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    gv[j] = S.splits > 0 ? float(colsum[j]) : a.G[e[j]];
    wv[j] = need_w ? a.w[e[j]] : 0.0f;
    pv[j] = (a.dots && a.p) ? a.p[e[j]] : 0.0f;
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    if ((cgl0 + j) * RA_COLS >= S.count) break; // wave-uniform: past the segment's last group
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    float g = gv[j];
    if (live[j]) {
      if (lam) g = g + float(a.lambda) * wv[j]; // finalize_kernel's update
      if (a.dots) {
        d0 = double(g) * double(g);
        if (a.p) d1 = double(g) * double(pv[j]);
        d2 = double(wv[j]) * double(wv[j]);
      }
      if (S.splits > 0 || lam) a.G[e[j]] = g;
    }
    if (a.dots) {
      d0 = wave_sum_f64(d0);
      d1 = wave_sum_f64(d1);
      d2 = wave_sum_f64(d2);
      if (lane == 0) {
        const int cg = cg0 + j;
        a.partials[cg * 3 + 0] = d0;
        a.partials[cg * 3 + 1] = d1;
        a.partials[cg * 3 + 2] = d2;
      }
    }
  }
}

// One block of a single-pass segment: J column groups (J * 64 columns, one per lane per group).
template <int J>
__device__ __forceinline__ void ra_block(const RedAllArgs &a, const RedSeg &S, int local, double (*part)[RA_GPB * RA_COLS]) {
  const int t = threadIdx.x, lane = t & 63, stripe = t >> 6;
  const long long cgl0 = (long long)local * J;
  double acc[J];
  const float *src[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const long long col = (cgl0 + j) * RA_COLS + lane;
    acc[j] = 0.0;
    src[j] = S.slab + (col < S.count ? col : 0); // clamped; masked when used
  }
  if (S.splits > 0) {
    // the stripe's splits k = stripe, stripe + 4, ...: rounds of four (4 x J loads in flight), then the
    // last up-to-three from clamped splits, masked; summed in split order either way
    int k = stripe;
    for (; k + 12 < S.splits; k += 16) {
      float x[4][J];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < J; ++j) x[u][j] = src[j][(long long)(k + 4 * u) * S.stride];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < J; ++j) acc[j] += double(x[u][j]);
    }
    float x[3][J];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const long long kk = k + 4 * u < S.splits ? k + 4 * u : 0;
#pragma unroll
      for (int j = 0; j < J; ++j) x[u][j] = src[j][kk * S.stride];
    }
#pragma unroll
    for (int u = 0; u < 3; ++u)
      if (k + 4 * u < S.splits) // wave-uniform
#pragma unroll
        for (int j = 0; j < J; ++j) acc[j] += double(x[u][j]);
  }
#pragma unroll
  for (int j = 0; j < J; ++j) part[stripe][j * RA_COLS + lane] = acc[j];
  __syncthreads();
  if (stripe != 0) return;
  double colsum[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int q = j * RA_COLS + lane;
    colsum[j] = ((part[0][q] + part[1][q]) + part[2][q]) + part[3][q];
  }
  ra_columns<J>(a, S, S.cg0 + int(cgl0), cgl0, colsum);
}

// One wave (lane t < 64): the rank's SSE partials in a fixed order, stored as an fp32 (hi, lo) pair.
__device__ __forceinline__ void sse_pack_body(const double *sse_part, int nsse, float *hilo, int t) {
  double s = 0.0;
  for (int r = t; r < nsse; r += 64) s += sse_part[r];
  s = wave_sum_f64(s);
  if (t == 0) {
    const float hi = float(s);
    hilo[0] = hi;
    hilo[1] = float(s - double(hi));
  }
}

__global__ __launch_bounds__(256) void reduce_all_kernel(const RedAllArgs a) {
  if (a.abort && *a.abort) return;
  __shared__ double part[4][RA_GPB * RA_COLS];
  const int t = threadIdx.x, lane = t & 63, stripe = t >> 6;
  const int b = blockIdx.x;
  if (b == a.nwg) { // the extra block of a data-parallel local reduction: the SSE words (sse_pack's launch)
    if (t < 64) sse_pack_body(a.sse_part, a.nsse, a.sse_hilo, t);
    return;
  }
  int si = 0;
  while (si + 1 < a.nseg && a.seg[si + 1].wg0 <= b) ++si;
  const RedSeg S = a.seg[si];
  const int local = b - S.wg0;
  if (S.parts == 1) { // wave-uniform
    if (S.gpb == RA_GPB) ra_block<RA_GPB>(a, S, local, part);
    else ra_block<1>(a, S, local, part);
    return;
  }
  const int cgl = local / S.parts, pi = local - cgl * S.parts;
  const int cg = S.cg0 + cgl;
  const long long col = (long long)cgl * RA_COLS + lane;
  const bool live = col < S.count;
  // this block's contiguous range of splits
  const int k0 = int((long long)S.splits * pi / S.parts), k1 = int((long long)S.splits * (pi + 1) / S.parts);
  double acc = 0.0;
  if (live && S.splits > 0) {
    const float *src = S.slab + col;
    int k = k0 + stripe;
    for (; k + 12 < k1; k += 16) { // four independent loads in flight, summed in split order
      const float x0 = src[(long long)k * S.stride], x1 = src[(long long)(k + 4) * S.stride];
      const float x2 = src[(long long)(k + 8) * S.stride], x3 = src[(long long)(k + 12) * S.stride];
      acc += double(x0);
      acc += double(x1);
      acc += double(x2);
      acc += double(x3);
    }
    for (; k < k1; k += 4) acc += double(src[(long long)k * S.stride]);
  }
  part[stripe][lane] = acc;
  __syncthreads();
  if (stripe != 0) return;
  const double colsum = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
  a.colpart[((long long)cg * RA_MAXPART + pi) * RA_COLS + lane] = colsum;
}

// One block: combine the split-range partials of the multi-range column groups, then (single rank)
// the eval_tail reduction. Everything it reads was written by earlier launches (stream order), so it
// needs no fence.
constexpr int RF_THREADS = 1024;
// The one summation of a point's SSE partials on a single rank, over the RF_THREADS threads of a block: thread t
// the words t, t + RF_THREADS, .. in order, each wave its lanes (wave_sum_f64); the caller stores wave w's value
// in ws[w * STRIDE], and after a barrier rf_sum_fin adds them in wave order. reduce_fin_kernel and sse_loss_kernel
// both go through these, so a trial's forward-only loss is bitwise the full evaluation's loss of the same point.
__device__ __forceinline__ double rf_sum_wave(const double *part, int n, int t) {
  double s = 0.0;
  for (int r = t; r < n; r += RF_THREADS) s += part[r];
  return wave_sum_f64(s);
}
template <int STRIDE> __device__ __forceinline__ double rf_sum_fin(const double *ws) {
  double x = 0.0;
  for (int w = 0; w < RF_THREADS / 64; ++w) x += ws[w * STRIDE];
  return x;
}
// WW: w.w (SC_WW, the penalty) from the point's partials (a.ww_part, ww_sum) instead of the dot partials
template <bool WW>
__global__ __launch_bounds__(RF_THREADS) void reduce_fin_kernel(const RedAllArgs a) {
  if (a.abort && *a.abort) return;
  KT(32);
  __shared__ double v[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int b = wave; b < a.nfin; b += RF_THREADS / 64) {
    int si = 0;
    while (!(a.seg[si].fin0 >= 0 && b >= a.seg[si].fin0 &&
             b < a.seg[si].fin0 + int((a.seg[si].count + RA_COLS - 1) / RA_COLS)))
      ++si;
    const RedSeg S = a.seg[si];
    const int cgl = b - S.fin0, cg = S.cg0 + cgl;
    const long long col = (long long)cgl * RA_COLS + lane;
    double pv[RA_MAXPART];
#pragma unroll
    for (int q = 0; q < RA_MAXPART; ++q)
      pv[q] = q < S.parts ? a.colpart[((long long)cg * RA_MAXPART + q) * RA_COLS + lane] : 0.0;
    double colsum = 0.0;
#pragma unroll
    for (int q = 0; q < RA_MAXPART; ++q)
      if (q < S.parts) colsum += pv[q];
    ra_column(a, S, cg, col, col < S.count, colsum);
  }
  KT(33);
  if (!a.dots) return;
  __syncthreads(); // this block's partials are visible to the whole block
  KT(34);
  // every thread a fixed set of rows, then a fixed-order tree: deterministic, one round of loads
  __shared__ double ws[RF_THREADS / 64][4];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int r = t; r < a.ncg; r += RF_THREADS) {
    acc[0] += a.partials[r * 3 + 0];
    acc[1] += a.partials[r * 3 + 1];
    acc[2] += a.partials[r * 3 + 2];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double w = wave_sum_f64(acc[i]);
    if (lane == 0) ws[wave][i] = w;
  }
  const double sse_w = rf_sum_wave(a.sse_part, a.nsse, t);
  if (lane == 0) ws[wave][3] = sse_w;
  __shared__ double wwv[WW ? 4 : 1];
  if constexpr (WW) {
    const double w = ww_sum_wave(a.ww_part, a.nww, t);
    if (lane == 0 && wave < 4) wwv[wave] = w;
  }
  __syncthreads();
  if (t < 4) v[t] = rf_sum_fin<4>(&ws[0][t]);
  __syncthreads();
  if (t == 0) {
    double *sc = a.scal;
    double ww = v[2];
    if constexpr (WW) ww = ww_sum_fin(wwv);
    sc[SC_TGG] = v[0];
    sc[SC_TGP] = v[1];
    sc[SC_SSE] = v[3];
    sc[SC_WW] = ww;
    sc[SC_LOSS] = point_loss<WW>(v[3], a.inv_scale, a.lambda, ww);
  }
  KT(35);
}

// Forward-only loss of a line-search trial: the SSE partials summed by the functions reduce_fin_kernel sums
// them with (rf_sum_wave, rf_sum_fin), so the loss is bitwise the one the full evaluation of the same point
// reports by construction; data parallel: from the all-reduced (hi, lo).
template <bool WW>
__global__ __launch_bounds__(RF_THREADS) void sse_loss_kernel(const double *sse_part, int nsse, const float *hilo,
                                                              double inv_scale, double *scal, const int *abort,
                                                              double lambda, const double *ww_part, int nww) {
  if (abort && *abort) return;
  __shared__ double ws[RF_THREADS / 64];
  __shared__ double wwv[WW ? 4 : 1];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const double w = rf_sum_wave(sse_part, hilo ? 0 : nsse, t);
  if (lane == 0) ws[wave] = w;
  if constexpr (WW) {
    const double q = ww_sum_wave(ww_part, nww, t);
    if (lane == 0 && wave < 4) wwv[wave] = q;
  }
  __syncthreads();
  if (t == 0) {
    const double sse = hilo ? (double(hilo[0]) + double(hilo[1])) : rf_sum_fin<1>(ws);
    scal[SC_SSE] = sse;
    const double ww = WW ? ww_sum_fin(wwv) : 0.0;
    if constexpr (WW) scal[SC_WW] = ww;
    scal[SC_LOSS] = point_loss<WW>(sse, inv_scale, WW ? lambda : 0.0, ww); // plain form: launched with lambda == 0
  }
}
void sse_loss(hipStream_t s, const double *sse_part, int nsse, const float *hilo, double inv_scale, double *scal,
              const int *abort, double lambda, WwPart ww) {
  LBF_REQUIRE(lambda == 0.0 || ww.part, "sse_loss: a penalised loss needs the point's w.w partials");
  if (lambda != 0.0)
    hipLaunchKernelGGL(sse_loss_kernel<true>, dim3(1), dim3(RF_THREADS), 0, s, sse_part, nsse, hilo, inv_scale, scal,
                       abort, lambda, ww.part, ww.n);
  else
    hipLaunchKernelGGL(sse_loss_kernel<false>, dim3(1), dim3(RF_THREADS), 0, s, sse_part, nsse, hilo, inv_scale, scal,
                       abort, 0.0, (const double *)nullptr, 0);
  LBF_KERNEL_CHECK();
}

void reduce_all(hipStream_t s, const RedAllArgs &a) {
  if (a.nwg <= 0 && !a.sse_hilo) return;
  hipLaunchKernelGGL(reduce_all_kernel, dim3(unsigned(a.nwg + (a.sse_hilo ? 1 : 0))), dim3(256), 0, s, a);
  LBF_KERNEL_CHECK();
  if (a.nfin > 0 || a.dots) {
    if (a.ww_part && a.lambda != 0.0 && a.dots)
      hipLaunchKernelGGL(reduce_fin_kernel<true>, dim3(1), dim3(RF_THREADS), 0, s, a);
    else
      hipLaunchKernelGGL(reduce_fin_kernel<false>, dim3(1), dim3(RF_THREADS), 0, s, a);
    LBF_KERNEL_CHECK();
  }
}

__global__ void eval_status_kernel(const double *sse_d, const float *hilo, double inv_scale, double lambda,
                                   double *scal) {
  const double sse = hilo ? (double(hilo[0]) + double(hilo[1])) : sse_d[0];
  scal[SC_SSE] = sse;
  scal[SC_LOSS] = point_loss<false>(sse, inv_scale, lambda, scal[SC_WW]);
}

void eval_status(hipStream_t s, const double *sse_d, const float *sse_hilo, double inv_scale, double lambda,
                 double *scal) {
  hipLaunchKernelGGL(eval_status_kernel, dim3(1), dim3(1), 0, s, sse_d, sse_hilo, inv_scale, lambda, scal);
  LBF_KERNEL_CHECK();
}

__global__ void pack_hilo_kernel(const double *x, float *hilo) {
  const float hi = float(x[0]);
  hilo[0] = hi;
  hilo[1] = float(x[0] - double(hi));
}
void pack_hilo(hipStream_t s, const double *x, float *hilo) {
  hipLaunchKernelGGL(pack_hilo_kernel, dim3(1), dim3(1), 0, s, x, hilo);
  LBF_KERNEL_CHECK();
}

// ---------------------------------------------------------------------------------------------
// Evaluation tail (one workgroup): fixed-order reductions of the finalize dots (g.g, g.p, w.w) and,
// on a single rank, of the SSE partials; then the loss (0.5*sse*inv_scale + 0.5*lambda*w.w).
// ---------------------------------------------------------------------------------------------
template <bool WW>
__global__ __launch_bounds__(256) void eval_tail_kernel(const double *dots_part, int nd, const double *sse_part,
                                                        int nsse, const float *hilo, double inv_scale,
                                                        double lambda, double *scal, const int *abort,
                                                        const double *ww_part, int nww) {
  if (abort && *abort) return;
  __shared__ double v[4];
  __shared__ double wwv[WW ? 4 : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double s = 0.0;
  if (wave < 3) {
    for (int r = lane; r < nd; r += 64) s += dots_part[r * 3 + wave];
  } else if (!hilo) {
    for (int r = lane; r < nsse; r += 64) s += sse_part[r];
  }
  s = wave_sum_f64(s);
  if (lane == 0) v[wave] = s;
  if constexpr (WW) {
    const double q = ww_sum_wave(ww_part, nww, threadIdx.x);
    if (lane == 0) wwv[wave] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sse = hilo ? (double(hilo[0]) + double(hilo[1])) : v[3];
    double ww = v[2];
    if constexpr (WW) ww = ww_sum_fin(wwv);
    scal[SC_TGG] = v[0];
    scal[SC_TGP] = v[1];
    scal[SC_SSE] = sse;
    scal[SC_WW] = ww;
    scal[SC_LOSS] = point_loss<WW>(sse, inv_scale, lambda, ww);
  }
}

void eval_tail(hipStream_t s, const double *dots_part, int nd, const double *sse_part, int nsse, const float *hilo,
               double inv_scale, double lambda, double *scal, const int *abort, WwPart ww) {
  if (ww.part && lambda != 0.0)
    hipLaunchKernelGGL(eval_tail_kernel<true>, dim3(1), dim3(256), 0, s, dots_part, nd, sse_part, nsse, hilo,
                       inv_scale, lambda, scal, abort, ww.part, ww.n);
  else
    hipLaunchKernelGGL(eval_tail_kernel<false>, dim3(1), dim3(256), 0, s, dots_part, nd, sse_part, nsse, hilo,
                       inv_scale, lambda, scal, abort, (const double *)nullptr, 0);
  LBF_KERNEL_CHECK();
}

// Data-parallel: reduce this rank's SSE partials and store them as an fp32 (hi, lo) pair behind the
// gradient, so one all-reduce of [grad | hi | lo] carries the loss with ~fp64 accuracy (sse_pack_body).
__global__ __launch_bounds__(64) void sse_pack_kernel(const double *sse_part, int nsse, float *hilo,
                                                      const int *abort) {
  if (abort && *abort) return;
  sse_pack_body(sse_part, nsse, hilo, threadIdx.x);
}

void sse_pack(hipStream_t s, const double *sse_part, int nsse, float *hilo, const int *abort) {
  hipLaunchKernelGGL(sse_pack_kernel, dim3(1), dim3(64), 0, s, sse_part, nsse, hilo, abort);
  LBF_KERNEL_CHECK();
}

} // namespace lbf
