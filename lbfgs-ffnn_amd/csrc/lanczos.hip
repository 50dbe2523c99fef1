// Device-side Lanczos sweeps (kernels.hpp has the contract; Mlp::lanczos drives them).
//
// Step j orthogonalises w = A q_j against the basis rows R_j and normalises it into q_{j+1}. Per pass: lz_proj
// forms the dots of w with the rows in one sweep over w per chunk of kLzChunk rows (each row streamed once), as
// per-workgroup partials [row][nwg]; lz_update has every workgroup sum the columns with the same pattern, subtract
// the combination and, on the last pass, leave the partials of w.w. lz_finish sums alpha_j and beta_j in every
// workgroup from those tables, takes the breakdown decision, and the grid writes q_{j+1} when the run goes on.
//
// The grid is cg_nwg(n) workgroups of 256 threads whatever j is, so steps can be enqueued ahead; sums follow
// cg.hip's rules (thread-private fp64 accumulation in loop order, wave_sum_f64, ((v0 + v1) + v2) + v3), and the
// spans are cg.hip's: a float4 body when every vector of a launch shares its offset from a 16-byte boundary.
#include "internal.hpp"
#include "kernels.hpp"
#include "sweep.hpp"

#include <cmath>

namespace lbf {

namespace {

constexpr int kLzChunk = 8; // rows per projection sweep: that many fp64 accumulators per lane

// Row i of the launch: slot0 + i, wrapped once when the rows live in a ring (reorth = 0).
__device__ __forceinline__ const float *lz_row(const LzRows &R, int i) {
  int s = R.slot0 + i;
  if (R.ring && s >= R.ring) s -= R.ring;
  return R.Q + (long long)s * R.ld;
}

__device__ __forceinline__ bool lz_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

__device__ __forceinline__ double dot4(const f32x4 a, const f32x4 b) {
  return double(a.x) * double(b.x) + double(a.y) * double(b.y) + double(a.z) * double(b.z) +
         double(a.w) * double(b.w);
}

// The dots of w with rows c0 .. c0 + NC - 1 of the launch: one pass over this thread's elements of w.
template <int NC>
__device__ __forceinline__ void proj_chunk(const Span &sp, const LzRows &R, int c0, const float *w, double *tab, int nwg,
                                           double *scratch) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  const float *q[NC];
  double acc[NC];
#pragma unroll
  for (int u = 0; u < NC; ++u) {
    q[u] = lz_row(R, c0 + u);
    acc[u] = 0.0;
  }
  for (long long v = gid; v < sp.nvec; v += stride) {
    const long long e = sp.head + 4 * v;
    const f32x4 wv4 = *reinterpret_cast<const f32x4 *>(w + e);
    f32x4 qv[NC];
#pragma unroll
    for (int u = 0; u < NC; ++u) qv[u] = *reinterpret_cast<const f32x4 *>(q[u] + e);
#pragma unroll
    for (int u = 0; u < NC; ++u) acc[u] += dot4(qv[u], wv4);
  }
  for (long long i = gid; i < span_nscalar(sp); i += stride) {
    const long long e = span_elem(sp, i);
    const double we = double(w[e]);
#pragma unroll
    for (int u = 0; u < NC; ++u) acc[u] += double(q[u][e]) * we;
  }
  block_sum<NC>(acc, scratch);
  if (threadIdx.x == 0)
#pragma unroll
    for (int u = 0; u < NC; ++u) tab[size_t(c0 + u) * nwg + blockIdx.x] = acc[u];
}

__global__ __launch_bounds__(256) void lz_proj_kernel(Span sp, LzRows R, const float *w, double *tab, int nwg,
                                                      const int *abort) {
  __shared__ double scratch[kLzChunk * 16];
  if (block_aborted(abort)) return;
  for (int c0 = 0; c0 < R.nrows; c0 += kLzChunk) {
    switch (min(kLzChunk, R.nrows - c0)) { // uniform over the grid
    case 8: proj_chunk<8>(sp, R, c0, w, tab, nwg, scratch); break;
    case 7: proj_chunk<7>(sp, R, c0, w, tab, nwg, scratch); break;
    case 6: proj_chunk<6>(sp, R, c0, w, tab, nwg, scratch); break;
    case 5: proj_chunk<5>(sp, R, c0, w, tab, nwg, scratch); break;
    case 4: proj_chunk<4>(sp, R, c0, w, tab, nwg, scratch); break;
    case 3: proj_chunk<3>(sp, R, c0, w, tab, nwg, scratch); break;
    case 2: proj_chunk<2>(sp, R, c0, w, tab, nwg, scratch); break;
    default: proj_chunk<1>(sp, R, c0, w, tab, nwg, scratch); break;
    }
  }
}

// coef[i] = float(sum of column i of tab), the same bits in every workgroup: wave v takes the columns v, v + 4, ..;
// lane l adds the words l, l + 64, .. in that order, then wave_sum_f64.
__device__ __forceinline__ void lz_col_sums(const double *tab, int nwg, int nrows, float *coef) {
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x >> 6; i < nrows; i += 4) {
    const double *t = tab + size_t(i) * nwg;
    double q = 0.0;
    for (int r = lane; r < nwg; r += 64) q += t[r];
    q = wave_sum_f64(q);
    if (lane == 0) coef[i] = float(q);
  }
}

// w -= sum_i coef_i q_i over the launch's rows in row order, one fused multiply-add per row and element; wwtab
// (nullable): the partials of the new w.w.
__global__ __launch_bounds__(256) void lz_update_kernel(Span sp, LzRows R, float *w, const double *tab, int nwg,
                                                        double *wwtab, const int *abort) {
  __shared__ float coef[LZ_MAX_STEPS];
  __shared__ double wv[4];
  if (block_aborted(abort)) return;
  lz_col_sums(tab, nwg, R.nrows, coef);
  __syncthreads();
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  double q2 = 0.0;
  for (long long v = gid; v < sp.nvec; v += stride) {
    const long long e = sp.head + 4 * v;
    f32x4 x = *reinterpret_cast<const f32x4 *>(w + e);
#pragma unroll 4
    for (int i = 0; i < R.nrows; ++i) {
      const f32x4 qv = *reinterpret_cast<const f32x4 *>(lz_row(R, i) + e);
      const float c = -coef[i];
      x.x = __builtin_fmaf(c, qv.x, x.x);
      x.y = __builtin_fmaf(c, qv.y, x.y);
      x.z = __builtin_fmaf(c, qv.z, x.z);
      x.w = __builtin_fmaf(c, qv.w, x.w);
    }
    *reinterpret_cast<f32x4 *>(w + e) = x;
    q2 += dot4(x, x);
  }
  for (long long k = gid; k < span_nscalar(sp); k += stride) {
    const long long e = span_elem(sp, k);
    float x = w[e];
#pragma unroll 4
    for (int i = 0; i < R.nrows; ++i) x = __builtin_fmaf(-coef[i], lz_row(R, i)[e], x);
    w[e] = x;
    q2 += double(x) * double(x);
  }
  if (!wwtab) return; // uniform
  q2 = block_sum_all(q2, wv);
  if (threadIdx.x == 0) wwtab[blockIdx.x] = q2;
}

// Partials of v.v.
__global__ __launch_bounds__(256) void lz_nrm2_kernel(Span sp, const float *v, double *tab) {
  __shared__ double wv[4];
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  double q = 0.0;
  for (long long g = gid; g < sp.nvec; g += stride) {
    const f32x4 x = *reinterpret_cast<const f32x4 *>(v + sp.head + 4 * g);
    q += dot4(x, x);
  }
  for (long long k = gid; k < span_nscalar(sp); k += stride) {
    const float x = v[span_elem(sp, k)];
    q += double(x) * double(x);
  }
  q = block_sum_all(q, wv);
  if (threadIdx.x == 0) tab[blockIdx.x] = q;
}

// dst = s src, and dst2 (nullable) the same.
__device__ __forceinline__ void lz_scale(const Span &sp, float s, const float *src, float *dst, float *dst2) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  for (long long v = gid; v < sp.nvec; v += stride) {
    const long long e = sp.head + 4 * v;
    const f32x4 x = s * *reinterpret_cast<const f32x4 *>(src + e);
    *reinterpret_cast<f32x4 *>(dst + e) = x;
    if (dst2) *reinterpret_cast<f32x4 *>(dst2 + e) = x;
  }
  for (long long k = gid; k < span_nscalar(sp); k += stride) {
    const long long e = span_elem(sp, k);
    const float x = s * src[e];
    dst[e] = x;
    if (dst2) dst2[e] = x;
  }
}

// q_0 = v0 float(1 / |v0|); a zero or non-finite |v0| cannot start: status LZ_FAILED with 0 steps.
__global__ __launch_bounds__(256) void lz_start_kernel(Span sp, const float *v0, float *q0, float *q0b,
                                                       const double *tab, int nwg, double *st, int *abort) {
  __shared__ double wv[4];
  const double vv = table_sum(tab, nwg, wv);
  const bool ok = finite_pos(vv);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st[LZ_STEPS] = 0.0;
    st[LZ_STATUS] = double(ok ? LZ_RUNNING : LZ_FAILED);
    st[LZ_V0NORM] = sqrt(vv);
    if (!ok) *abort = 1;
  }
  if (ok) lz_scale(sp, float(1.0 / sqrt(vv)), v0, q0, q0b);
}

// alpha_j, beta_j and the decision, formed by every workgroup from the same tables; workgroup 0 stores them. The
// scale of the breakdown test, max(|alpha_0..j|, beta_0..j-1), comes from the word the previous step's launch left
// in st[LZ_SCALE + j - 1], so no workgroup reads what this launch writes.
__global__ __launch_bounds__(256) void lz_finish_kernel(Span sp, int j, int steps, int npass, int col, const float *w,
                                                        float *qn, float *qnb, const double *tab, size_t pass_stride,
                                                        const double *wwtab, int nwg, double rtol, double *st,
                                                        int *abort) {
  __shared__ double wv[4];
  if (block_aborted(abort)) return;
  double alpha = 0.0;
  for (int p = 0; p < npass; ++p) alpha += table_sum(tab + p * pass_stride + size_t(col) * nwg, nwg, wv);
  const double beta = sqrt(table_sum(wwtab, nwg, wv));
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  if (!lz_finite(alpha) || !lz_finite(beta)) {
    if (lead) {
      st[LZ_STEPS] = double(j);
      st[LZ_STATUS] = double(LZ_FAILED);
      *abort = 1;
    }
    return;
  }
  const double scale = fmax(j > 0 ? st[LZ_SCALE + j - 1] : 0.0, fabs(alpha));
  const bool exhausted = beta <= rtol * scale;
  if (lead) {
    st[LZ_ALPHA + j] = alpha;
    st[LZ_BETA + j] = beta;
    st[LZ_SCALE + j] = fmax(scale, beta);
    st[LZ_STEPS] = double(j + 1);
    // The status as a table lookup, not as nested selects: hipcc 7 folds `exhausted ? 1 : last ? 0 : -1` into two
    // scalar selects on the one condition code of `last`, which stores +1 (exhausted) for a run that goes on. Seen
    // with the clang of ROCm 7 at -O3 for gfx950; with another compiler, look for the compare between the two selects
    // in this kernel's assembly. tests/test_gpu_lanczos.py runs longer than `check` steps catch the wrong word: they
    // would end with status 1 at their first status read.
    const double word[4] = {double(LZ_RUNNING), double(LZ_DONE), double(LZ_EXHAUSTED), double(LZ_EXHAUSTED)};
    st[LZ_STATUS] = word[(exhausted ? 2 : 0) + (j + 1 == steps ? 1 : 0)];
    if (exhausted) *abort = 1;
  }
  if (!exhausted) lz_scale(sp, float(1.0 / beta), w, qn, qnb);
}

} // namespace

void lz_start(hipStream_t s, const LzArgs &a, const float *v0, float *q0, float *q0b) {
  const int nwg = cg_nwg(a.n);
  hipLaunchKernelGGL(lz_nrm2_kernel, dim3(unsigned(nwg)), dim3(256), 0, s, make_span(a.n, v0), v0, a.wwtab);
  LBF_KERNEL_CHECK();
  const Span sp = q0b ? make_span(a.n, v0, q0, q0b) : make_span(a.n, v0, q0);
  hipLaunchKernelGGL(lz_start_kernel, dim3(unsigned(nwg)), dim3(256), 0, s, sp, v0, q0, q0b, a.wwtab, nwg, a.st,
                     a.abort);
  LBF_KERNEL_CHECK();
}

void lz_orth(hipStream_t s, const LzArgs &a, const LzRows &R, int pass, bool last) {
  const int nwg = cg_nwg(a.n);
  // the offsets of the rows this launch reads: the first row's and, with more than one row, the next one's as well
  // (every other row lies a multiple of ld further, ring or not); a single row does not bring the stride in
  const float *r0 = R.Q + (long long)R.slot0 * R.ld;
  const Span sp = R.nrows > 1 ? make_span(a.n, a.w, r0, r0 + R.ld) : make_span(a.n, a.w, r0);
  double *tab = a.tab + size_t(pass) * lz_pass_words(a.n);
  hipLaunchKernelGGL(lz_proj_kernel, dim3(unsigned(nwg)), dim3(256), 0, s, sp, R, a.w, tab, nwg, a.abort);
  LBF_KERNEL_CHECK();
  hipLaunchKernelGGL(lz_update_kernel, dim3(unsigned(nwg)), dim3(256), 0, s, sp, R, a.w, tab, nwg,
                     last ? a.wwtab : nullptr, a.abort);
  LBF_KERNEL_CHECK();
}

void lz_finish(hipStream_t s, const LzArgs &a, int j, int npass, int col, float *qn, float *qnb) {
  const int nwg = cg_nwg(a.n);
  const Span sp = qnb ? make_span(a.n, a.w, qn, qnb) : make_span(a.n, a.w, qn);
  hipLaunchKernelGGL(lz_finish_kernel, dim3(unsigned(nwg)), dim3(256), 0, s, sp, j, a.steps, npass, col, a.w, qn, qnb,
                     a.tab, lz_pass_words(a.n), a.wwtab, nwg, a.breakdown_rtol, a.st, a.abort);
  LBF_KERNEL_CHECK();
}

size_t lz_pass_words(long long n) { return size_t(LZ_MAX_STEPS) * size_t(cg_nwg(n)); }

} // namespace lbf
