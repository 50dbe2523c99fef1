// Wavefront (64-lane) primitives shared by the kernels, the workgroup sums built on them, and f32x4.
//
// wave_sum_f64: fixed-order fp64 reduction through DPP lane moves (quad_perm, row_half_mirror,
// row_mirror, row_bcast15/31) — VALU moves instead of the ds_bpermute round trips a __shfl_xor
// butterfly costs (each a trip through the LDS crossbar). The sum lands in lane 63 and is broadcast
// with v_readlane, so every lane returns the same value. Deterministic: the addition tree is fixed.
// lane_f64: v_readlane of a wave-uniform lane index (the two-loop recurrences' per-step scalar).
#pragma once

#include <hip/hip_runtime.h>

namespace lbf {

typedef float f32x4 __attribute__((ext_vector_type(4))); // one 16-byte lane access

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xF, false);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double lane_f64(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
  v += dpp_f64<0xB1, 0xF>(v);  // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E, 0xF>(v);  // quad_perm [2,3,0,1]: quad sums
  v += dpp_f64<0x141, 0xF>(v); // row_half_mirror: 8-lane sums
  v += dpp_f64<0x140, 0xF>(v); // row_mirror: 16-lane row sums
  v += dpp_f64<0x142, 0xA>(v); // row_bcast15 into rows 1, 3
  v += dpp_f64<0x143, 0xC>(v); // row_bcast31 into rows 2, 3: lane 63 holds the total
  return lane_f64(v, 63);
}

// The one summation of a point's w.w partials (kernels.hpp WwPart). Threads 0..255 of the block take the words
// r = t, t + 256, ..; each of waves 0..3 sums its lanes (wave_sum_f64); the caller stores wave w's value in
// v[w] (w < 4), and after a barrier ww_sum_fin(v) = ((v0 + v1) + v2) + v3. Every consumer goes through these
// two functions, so all of them form the same bits from the same words. Call with every thread of the block.
__device__ __forceinline__ double ww_sum_wave(const double *part, int n, int t) {
  double s = 0.0;
  if (t < 256)
    for (int r = t; r < n; r += 256) s += part[r];
  return wave_sum_f64(s);
}
__device__ __forceinline__ double ww_sum_fin(const double *v) { return ((v[0] + v[1]) + v[2]) + v[3]; }
// loss = data + 0.5 lambda w.w with the roundings fixed (one product, one fused multiply-add), whatever the
// surrounding code is contracted to
__device__ __forceinline__ double ww_loss(double data, double lambda, double ww) {
  return __fma_rn(__dmul_rn(0.5, lambda), ww, data);
}
// The loss of a point, 0.5 sse inv_scale + 0.5 lambda w.w, as every one-workgroup tail of reduce.hip forms it.
// WW: w.w is the sum of the point's partials and ww_loss adds the penalty; else the plain expression, if lambda != 0.
template <bool WW>
__device__ __forceinline__ double point_loss(double sse, double inv_scale, double lambda, double ww) {
  const double data = 0.5 * sse * inv_scale;
  if constexpr (WW) return ww_loss(data, lambda, ww);
  return lambda != 0.0 ? data + 0.5 * lambda * ww : data;
}

// The sum of a 256-thread block in a fixed order: wave sums, then ((v0 + v1) + v2) + v3; every thread returns the
// same bits. wv: four doubles of LDS, which may still hold a previous sum.
__device__ __forceinline__ double block_sum_all(double q, double *wv) {
  q = wave_sum_f64(q);
  __syncthreads(); // wv may still be read from a previous sum
  if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = q;
  __syncthreads();
  return ww_sum_fin(wv);
}
// One word of a w.w partial table (kernels.hpp WwPart): the 256-thread block's sum in block_sum_all's order,
// stored by thread 0 with an ordinary store.
__device__ __forceinline__ void ww_block_store(double q, double *part) {
  __shared__ double wv[4];
  q = wave_sum_f64(q);
  if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = q;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ww_sum_fin(wv);
}
// Sum NV values over a 256- or 512-thread block; result valid in thread 0. scratch: NV*16 doubles.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double *scratch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = wave_sum_f64(v[i]);
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < NV; ++i) scratch[i * 16 + wave] = v[i];
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      double s = 0.0;
      for (int w = 0; w < nw; ++w) s += scratch[i * 16 + w];
      v[i] = s;
    }
  }
  __syncthreads();
}

// Reductions over a DPP row (the 16 lanes l & ~15 .. l | 15): quad_perm [1,0,3,2] and [2,3,0,1], then
// row_half_mirror and row_mirror. Each step combines a lane's value with its partner's, and both partners
// form the same commutative pair, so all 16 lanes end with the same bits. Used by the softmax head, where
// lane (li, g) holds output li of a sample and a row group g is one DPP row.
template <int CTRL> __device__ __forceinline__ float dpp_row_f32(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row16_max_f32(float v) {
  v = fmaxf(v, dpp_row_f32<0xB1>(v));
  v = fmaxf(v, dpp_row_f32<0x4E>(v));
  v = fmaxf(v, dpp_row_f32<0x141>(v));
  v = fmaxf(v, dpp_row_f32<0x140>(v));
  return v;
}
__device__ __forceinline__ float row16_sum_f32(float v) {
  v += dpp_row_f32<0xB1>(v);
  v += dpp_row_f32<0x4E>(v);
  v += dpp_row_f32<0x141>(v);
  v += dpp_row_f32<0x140>(v);
  return v;
}
// Wave-wide maximum, the same bits on every lane (butterfly: each step pairs a lane with its partner).
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// Workgroup barrier that orders LDS only. __syncthreads() carries a workgroup-scope release, which on
// gfx950 means s_waitcnt vmcnt(0): every global store the wave has in flight must be acknowledged
// (~1 us) before the barrier. Where no thread reads, after the barrier, global memory written before
// it by another thread of the block, the LDS wait is all the barrier has to order.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The speculative chain's abort flag (null: never aborted), requested as a vector load (an agent-scope
// relaxed atomic load is a global_load, counted by vmcnt). A kernel that tests it only once its first loads
// are in flight then does not wait for it in front of them; a scalar load of the flag would be covered by the
// kernel's first lgkmcnt wait for its arguments. Test it wave-uniformly: aborted(flag).
__device__ __forceinline__ int abort_flag(const int *p) {
  return p ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
}
__device__ __forceinline__ bool aborted(int flag) { return __builtin_amdgcn_readfirstlane(flag) != 0; }

} // namespace lbf
