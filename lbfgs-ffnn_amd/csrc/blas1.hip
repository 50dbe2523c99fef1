// Elementwise vector kernels (gfx950, wave64): axpy and its w.w partials, the GD / SGD step, row gather, the
// in-process rank sum, fingerprints and S-LBFGS's iterate average. One pass over n floats each.
//
// Replaces: cublasSaxpy / Sscal with host pointer mode (src/cuda/kernels.cuh:28-50), the GD / SGD updates
// (gd.cuh:77-85, sgd.cuh:115-126), batch_g's column gather (unified_optimization.hpp:361-364) and the iterate
// average (s_lbfgs.hpp:236-243).
//
// Implements (kernels.hpp): axpy_to, axpy, ww_block_elems, ww_partials_n, ww_partials, momentum_step,
// epoch_loss_acc, scal, lincomb, gather_rows, zero_fill, sum_ranks, fingerprint, diff_scale, average_slots.
#include "internal.hpp"
#include "kernels.hpp"
#include "wave.hpp"

#include <algorithm>

namespace lbf {

// y = x + alpha p on 16-byte lanes, the n % 4 tail per element
__global__ __launch_bounds__(256) void axpy_to_kernel(long long n, const float *x, float alpha, const float *p,
                                                      float *y) {
  const long long e = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (e + 3 < n) {
    const f32x4 a = *reinterpret_cast<const f32x4 *>(x + e);
    const f32x4 b = *reinterpret_cast<const f32x4 *>(p + e);
    *reinterpret_cast<f32x4 *>(y + e) = a + alpha * b;
  } else {
    for (long long j = e; j < n; ++j) y[j] = x[j] + alpha * p[j];
  }
}
// x, p or y off a 16-B boundary (a caller's pointer, lbf_axpy): one element per thread, the same fp32 expression
__global__ __launch_bounds__(256) void axpy_to_elem_kernel(long long n, const float *x, float alpha, const float *p,
                                                           float *y) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) y[e] = x[e] + alpha * p[e];
}
// w.w partials (kernels.hpp WwPart): one word per block of E = ww_block_elems(n) elements.
long long ww_block_elems(long long n) {
  long long e = 256;
  while (cdiv(n, e) > 8192) e *= 2;
  return e;
}
int ww_partials_n(long long n) { return int(std::max(1LL, cdiv(n, ww_block_elems(n)))); }
// block b: elements [b E, (b + 1) E), thread t the elements b E + t, + 256, .. in order
__global__ __launch_bounds__(256) void ww_partials_kernel(long long n, long long E, const float *x, double *part,
                                                          const int *abort) {
  if (abort && *abort) return;
  const long long e0 = (long long)blockIdx.x * E, e1 = e0 + E < n ? e0 + E : n;
  double q = 0.0;
  for (long long e = e0 + threadIdx.x; e < e1; e += 256) q += double(x[e]) * double(x[e]);
  ww_block_store(q, part);
}
void ww_partials(hipStream_t s, long long n, const float *x, double *part, const int *abort) {
  hipLaunchKernelGGL(ww_partials_kernel, dim3(unsigned(ww_partials_n(n))), dim3(256), 0, s, n, ww_block_elems(n), x,
                     part, abort);
  LBF_KERNEL_CHECK();
}
// axpy_to that also writes y's w.w partials (E == 256: one element per thread, one word per block)
__global__ __launch_bounds__(256) void axpy_to_ww_kernel(long long n, const float *x, float alpha, const float *p,
                                                         float *y, double *part) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  double q = 0.0;
  if (e < n) {
    const float o = x[e] + alpha * p[e];
    y[e] = o;
    q = double(o) * double(o);
  }
  ww_block_store(q, part);
}
// GD / SGD step (gd.cuh:77-85, sgd.cuh:115-124): v = m v - lr g ; x += v (m > 0), else x -= lr g. The
// reference's scal + two cuBLAS saxpys in one pass: v*m rounded, then the saxpys' fused multiply-adds.
// lr is read from the device (SGD's decayed rate lives there) when lr_dev is non-null.
__global__ __launch_bounds__(256) void momentum_step_kernel(long long n, float momentum, float lr, const float *lr_dev,
                                                            const float *g, float *v, float *x) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float r = lr_dev ? *lr_dev : lr;
  if (momentum > 0.0f) {
    const float vi = __fmaf_rn(-r, g[i], __fmul_rn(v[i], momentum));
    v[i] = vi;
    x[i] = __fadd_rn(x[i], vi);
  } else {
    x[i] = __fmaf_rn(-r, g[i], x[i]);
  }
}
void momentum_step(hipStream_t s, long long n, float momentum, float lr, const float *lr_dev, const float *g, float *v,
                   float *x) {
  if (n <= 0) return;
  hipLaunchKernelGGL(momentum_step_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, n, momentum, lr, lr_dev, g,
                     v, x);
  LBF_KERNEL_CHECK();
}

// SGD's epoch loss (sgd.cuh:126): esum += float(batch loss) * float(batch rows), fp32 like the reference's
// host scalars; one thread, after each batch evaluation (no host round trip per batch).
__global__ void epoch_loss_acc_kernel(const double *scal, float rows, float *esum) {
  *esum = __fadd_rn(*esum, __fmul_rn(float(scal[SC_LOSS]), rows));
}
void epoch_loss_acc(hipStream_t s, const double *scal, long long rows, float *esum) {
  hipLaunchKernelGGL(epoch_loss_acc_kernel, dim3(1), dim3(1), 0, s, scal, float(rows), esum);
  LBF_KERNEL_CHECK();
}

void axpy_to(hipStream_t s, long long n, const float *x, float alpha, const float *p, float *y, double *ww_part) {
  if (ww_part && ww_block_elems(n) == 256) {
    hipLaunchKernelGGL(axpy_to_ww_kernel, dim3(unsigned(ww_partials_n(n))), dim3(256), 0, s, n, x, alpha, p, y,
                       ww_part);
    LBF_KERNEL_CHECK();
    return;
  }
  if (aligned16(x, p, y))
    hipLaunchKernelGGL(axpy_to_kernel, dim3(unsigned(cdiv(cdiv(n, 4), 256))), dim3(256), 0, s, n, x, alpha, p, y);
  else if (n > 0)
    hipLaunchKernelGGL(axpy_to_elem_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, n, x, alpha, p, y);
  LBF_KERNEL_CHECK();
  if (ww_part) ww_partials(s, n, y, ww_part); // large n: the partials of wider blocks in a launch of their own
}
void axpy(hipStream_t s, long long n, float alpha, const float *x, float *y) { axpy_to(s, n, y, alpha, x, y); }

__global__ __launch_bounds__(256) void scal_kernel(long long n, float alpha, float *x) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) x[e] *= alpha;
}
void scal(hipStream_t s, long long n, float alpha, float *x) {
  hipLaunchKernelGGL(scal_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, n, alpha, x);
  LBF_KERNEL_CHECK();
}

__global__ __launch_bounds__(256) void lincomb_kernel(long long n, const float *a, double c, const float *b,
                                                      float *out, const int *abort) {
  if (abort && *abort) return;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) out[e] = float(double(a[e]) + c * double(b[e]));
}
void lincomb(hipStream_t s, long long n, const float *a, double c, const float *b, float *out, const int *abort) {
  hipLaunchKernelGGL(lincomb_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, n, a, c, b, out, abort);
  LBF_KERNEL_CHECK();
}

// Minibatch rows gathered into a contiguous block (S-LBFGS: both evaluations of an inner step read the
// same rows; batch_g's column gather, unified_optimization.hpp:361-364). 16-B lanes when cols % 4 == 0,
// ld % 4 == 0 and both base pointers are 16-B aligned (the caller's X may be any float pointer).
__global__ __launch_bounds__(256) void gather_rows_kernel(const float *src, long long ld, const int *idx,
                                                          long long count, int cols, int vec, float *dst) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec) {
    const int c4 = cols >> 2;
    if (q >= count * c4) return;
    const long long r = q / c4, c = (q - r * c4) * 4;
    *reinterpret_cast<f32x4 *>(dst + r * cols + c) = *reinterpret_cast<const f32x4 *>(src + (long long)idx[r] * ld + c);
  } else {
    if (q >= count * cols) return;
    const long long r = q / cols, c = q - r * cols;
    dst[r * cols + c] = src[(long long)idx[r] * ld + c];
  }
}
void gather_rows(hipStream_t s, const float *src, long long ld, const int *idx, long long count, int cols,
                 float *dst) {
  if (count <= 0) return;
  const int vec = (cols & 3) == 0 && (ld & 3) == 0 && aligned16(src, dst) ? 1 : 0;
  const long long per = vec ? cols / 4 : cols;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(unsigned(cdiv(count * per, 256))), dim3(256), 0, s, src, ld, idx, count,
                     cols, vec, dst);
  LBF_KERNEL_CHECK();
}

// x[0 .. n) = 0 unless the speculative chain was aborted (a data-parallel rank's empty share)
__global__ __launch_bounds__(256) void zero_fill_kernel(long long n, float *x, const int *abort) {
  if (abort && *abort) return;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) x[e] = 0.0f;
}
void zero_fill(hipStream_t s, long long n, float *x, const int *abort) {
  if (n <= 0) return;
  hipLaunchKernelGGL(zero_fill_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, n, x, abort);
  LBF_KERNEL_CHECK();
}

// In-process rank group (comm.cpp LocalComm): dst = src[0] + src[1] + ... in rank order, fp32, so
// every rank of the group computes the same bits.
__global__ __launch_bounds__(256) void sum_ranks_kernel(RankSrcs r, long long count, float *dst) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  float acc = r.p[0][e];
  for (int i = 1; i < r.n; ++i) acc += r.p[i][e];
  dst[e] = acc;
}
void sum_ranks(hipStream_t s, const RankSrcs &r, long long count, float *dst) {
  LBF_REQUIRE(r.n >= 1 && r.n <= kMaxLocalRanks, "sum_ranks: 1..16 ranks");
  if (count <= 0) return;
  hipLaunchKernelGGL(sum_ranks_kernel, dim3(unsigned(cdiv(count, 256))), dim3(256), 0, s, r, count, dst);
  LBF_KERNEL_CHECK();
}

// Order-independent 32-bit fingerprints (a sum and an xor of mixed element bits) of x[0 .. n), stored in
// out[4 slot .. 4 slot + 3] as four exact 16-bit halves in floats, so that a sum all-reduce of a zeroed
// [4 nranks] buffer in which each rank filled its own slot hands every rank every rank's fingerprints.
// One workgroup: called once per S-LBFGS epoch (the replicated data-parallel check).
__global__ __launch_bounds__(1024) void fingerprint_kernel(long long n, const float *x, int slot, float *out) {
  const int t = threadIdx.x;
  unsigned hs = 0u, hx = 0u;
  for (long long e = t; e < n; e += 1024) {
    unsigned h = (__float_as_uint(x[e]) ^ (unsigned(e) * 0x9E3779B9u)) * 0x85EBCA6Bu;
    h ^= h >> 13;
    hs += h;
    hx ^= h * 0xC2B2AE35u;
  }
  __shared__ unsigned ss[1024], sx[1024];
  ss[t] = hs;
  sx[t] = hx;
  __syncthreads();
  for (int k = 512; k > 0; k >>= 1) {
    if (t < k) {
      ss[t] += ss[t + k];
      sx[t] ^= sx[t + k];
    }
    __syncthreads();
  }
  if (t < 4) {
    const unsigned v = t < 2 ? ss[0] : sx[0];
    out[4 * slot + t] = float((t & 1) ? (v >> 16) : (v & 0xffffu));
  }
}
void fingerprint(hipStream_t s, long long n, const float *x, int slot, float *out) {
  hipLaunchKernelGGL(fingerprint_kernel, dim3(1), dim3(1024), 0, s, n, x, slot, out);
  LBF_KERNEL_CHECK();
}

// y = (a - b) * scale in fp32: the pair sweep's y of a finite-difference HVP (gram_kernel forms the
// same product when it writes the ring slot)
__global__ __launch_bounds__(256) void diff_scale_kernel(long long n, const float *a, const float *b, float scale,
                                                         float *out) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) out[e] = (a[e] - b[e]) * scale;
}
void diff_scale(hipStream_t s, long long n, const float *a, const float *b, float scale, float *out) {
  hipLaunchKernelGGL(diff_scale_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, n, a, b, scale, out);
  LBF_KERNEL_CHECK();
}

// S-LBFGS iterate averaging (s_lbfgs.hpp:236-243): u = (sum_i w_i) / cnt in logical order.
struct SlotList {
  int cnt;
  int slot[64];
};
__global__ __launch_bounds__(256) void average_kernel(long long n, const float *W, long long ld, SlotList sl,
                                                      float *u) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  double s = 0.0;
  for (int i = 0; i < sl.cnt; ++i) s += double(W[sl.slot[i] * ld + e]);
  u[e] = float(s / double(sl.cnt));
}
void average_slots(hipStream_t s, long long n, const float *W, long long ld, const int *h_slots, int cnt, float *u) {
  LBF_REQUIRE(cnt > 0 && cnt <= 64, "average_slots: 1..64 iterates supported (L+1 <= 64)");
  SlotList sl;
  sl.cnt = cnt;
  for (int i = 0; i < cnt; ++i) sl.slot[i] = h_slots[i];
  hipLaunchKernelGGL(average_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, s, n, W, ld, sl, u);
  LBF_KERNEL_CHECK();
}

} // namespace lbf
