// Sum of squared per-example gradients of a dense layer (Mlp::grad_sq): the diagonal of the empirical
// Fisher matrix, and the Hessian-free solver's preconditioner (Martens 2010, section 4.7).
//
// Row b's gradient of layer l is a_{b,i} delta_{b,j} (bias: delta_{b,j}), so the layer's segment of
// sum_b (dl_b / dw)^2 is [A.A | 1]^T (D.D): the [dW ; db] product with both operands squared element by element.
//   C[i][j] = sum_b a_{bi}^2 d_{bj}^2,  i <= In (row In is the ones row), j < Out.
// No per-example gradient and no squared copy of an operand reaches memory: the operands are squared in registers
// on their way from global memory to LDS (which is why this is not gemm.hip's LDS-DMA path).
//
// Workgroup: 256 threads = 2 x 2 waves, one 32 x 32 tile of v_mfma_f32_32x32x2_f32 each (gemm.hip's lane layout:
// lane l feeds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; accumulator register r of lane l is
// C[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31]). Grid: (row tiles of 64, column tiles of 64, row chunks). A chunk
// is a contiguous range of batch rows, walked 32 at a time; chunk z writes slab z in the layer's
// [(In + 1) x Out] layout and reduce_slabs sums the slabs in chunk order. The chunk count is a function of
// (B, In, Out) only and nothing is accumulated atomically, so two calls give the same bits.
//
// Edges follow the head kernels' rule: an address past the operand is clamped to a valid one and the loaded value
// is masked to zero (rows >= the chunk's end, columns >= In + 1 or >= Out), so no lane reads out of bounds and no
// lane diverges around a load.
#include "internal.hpp"
#include "kernels.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace lbf {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int GS_T = 64;   // tile edge (rows i and columns j)
constexpr int GS_K = 32;   // batch rows per LDS stage
constexpr int GS_LD = 66;  // LDS row stride: rows k and k + 16 (the two lane halves of one step) 32 banks apart
constexpr int GS_MIN_CHUNK = 128; // batch rows per chunk, at least
constexpr int GS_MAX_WG = 1024;   // workgroups aimed at: 4 on each of 256 CUs
constexpr int GS_MAX_SPLITS = 256;

__global__ __launch_bounds__(256) void grad_sq_kernel(const float *__restrict__ A, int In, const int *__restrict__ idx,
                                                      const float *__restrict__ D, int Out, long long B,
                                                      long long chunk, float *__restrict__ slab) {
  __shared__ float As[GS_K * GS_LD], Ds[GS_K * GS_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int i0 = blockIdx.x * GS_T, j0 = blockIdx.y * GS_T;
  const long long k_begin = (long long)blockIdx.z * chunk, k_end = std::min(B, k_begin + chunk);

  // staging: thread t carries column t & 63 of rows (t >> 6) + 4 q, q < 8, of both operands
  const int sc = t & 63, sr = t >> 6;
  const int ai = i0 + sc, dj = j0 + sc;
  const bool a_in = ai < In, a_one = ai == In, d_in = dj < Out;
  const int ai_c = std::min(ai, In - 1), dj_c = std::min(dj, Out - 1);
  float ra[8], rd[8];
  auto load = [&](long long k0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const long long row = k0 + sr + 4 * q;
      const bool live = row < k_end;
      const long long rc = live ? row : k_end - 1; // k_begin < k_end: every chunk has a row
      const long long ar = idx ? (long long)idx[rc] : rc;
      const float av = A[ar * In + ai_c], dv = D[rc * Out + dj_c];
      ra[q] = live ? (a_in ? av : (a_one ? 1.0f : 0.0f)) : 0.0f;
      rd[q] = (live && d_in) ? dv : 0.0f;
    }
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;

  load(k_begin);
  for (long long k0 = k_begin; k0 < k_end; k0 += GS_K) {
    __syncthreads(); // the previous stage's fragments have been read
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      As[(sr + 4 * q) * GS_LD + sc] = ra[q] * ra[q];
      Ds[(sr + 4 * q) * GS_LD + sc] = rd[q] * rd[q];
    }
    __syncthreads();
    if (k0 + GS_K < k_end) load(k0 + GS_K); // the next stage's loads fly under this stage's MFMAs
#pragma unroll
    for (int s = 0; s < GS_K / 2; ++s) { // lane half h consumes row 16 h + s at step s (any order of k sums the same rows)
      const float av = As[(16 * lh + s) * GS_LD + wm * 32 + li];
      const float bv = Ds[(16 * lh + s) * GS_LD + wn * 32 + li];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
  }

  float *C = slab + (long long)blockIdx.z * (long long)(In + 1) * Out;
  const int j = j0 + wn * 32 + li;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = i0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    if (i <= In && j < Out) C[(long long)i * Out + j] = acc[r];
  }
}

} // namespace

int grad_sq_splits(long long B, int In, int Out, long long *chunk_out) {
  const long long tiles = cdiv((long long)In + 1, GS_T) * cdiv((long long)Out, GS_T);
  long long splits = std::max(1LL, std::min<long long>(cdiv(B, GS_MIN_CHUNK), std::max(1LL, GS_MAX_WG / tiles)));
  splits = std::min<long long>(splits, GS_MAX_SPLITS);
  const long long chunk = cdiv(cdiv(std::max(B, 1LL), splits), GS_K) * GS_K;
  if (chunk_out) *chunk_out = chunk;
  return int(std::max(1LL, cdiv(B, chunk))); // every chunk [z chunk, (z + 1) chunk) holds a row
}

void grad_sq_layer(hipStream_t s, const float *A, int In, const int *idx, const float *D, int Out, long long B,
                   double scale, float *slab, float *out) {
  if (B <= 0) return;
  long long chunk = 0;
  const int splits = grad_sq_splits(B, In, Out, &chunk);
  const long long seg = (long long)(In + 1) * Out;
  hipLaunchKernelGGL(grad_sq_kernel, dim3(unsigned(cdiv(In + 1, GS_T)), unsigned(cdiv(Out, GS_T)), unsigned(splits)),
                     dim3(256), 0, s, A, In, idx, D, Out, B, chunk, slab);
  LBF_KERNEL_CHECK();
  reduce_slabs(s, slab, splits, seg, seg, out, nullptr, scale);
}

} // namespace lbf
