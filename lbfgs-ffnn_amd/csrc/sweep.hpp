// What the fixed-grid fp64-partial sweeps share (cg.hip, lanczos.hip): the span of a sweep over vectors whose
// pointers are 4-byte aligned only, the sum of a partial table that every workgroup forms with the
// same bits, and the abort word read once per workgroup.
#pragma once

#include "internal.hpp"
#include "wave.hpp"

#include <algorithm>

namespace lbf {

// Elements [0, head) and [tail0, n) one at a time, [head, tail0) as nvec float4 groups.
struct Span {
  long long n, head, nvec, tail0;
};

template <class... P> Span make_span(long long n, P... ptrs) {
  const int lead = common_lead(ptrs...);
  Span sp{n, n, 0, n};
  if (lead >= 0) {
    sp.head = std::min<long long>(n, lead);
    sp.nvec = (n - sp.head) / 4;
    sp.tail0 = sp.head + 4 * sp.nvec;
  }
  return sp;
}

// The scalar elements of a span as one index range: j < head is element j, then tail0 + (j - head).
__device__ __forceinline__ long long span_nscalar(const Span &sp) { return sp.head + (sp.n - sp.tail0); }
__device__ __forceinline__ long long span_elem(const Span &sp, long long j) {
  return j < sp.head ? j : sp.tail0 + (j - sp.head);
}

// The sum of a partial table, the same bits in every workgroup that calls it.
__device__ __forceinline__ double table_sum(const double *t, int nwg, double *wv) {
  double q = 0.0;
  for (int i = threadIdx.x; i < nwg; i += 256) q += t[i];
  return block_sum_all(q, wv);
}

// The abort word read once per workgroup, so that all its waves take the same branch even when workgroup 0 of
// this very launch raises the word meanwhile.
__device__ __forceinline__ bool block_aborted(const int *abort) {
  __shared__ int flag;
  if (threadIdx.x == 0) flag = abort_flag(abort);
  __syncthreads();
  return flag != 0;
}

__device__ __forceinline__ bool finite_pos(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

} // namespace lbf
