// The device-resident history on the unfused path (gfx950, wave64): Gram sweep, the one-workgroup history step
// (push and coefficient two-loop, hist_core.hpp) and the linear-combination sweep that forms the direction and
// the trial point.
//
// Replaces: CudaLBFGS::compute_direction_ring (src/cuda/lbfgs.cuh:206-261, 2k+2 blocking dots + 2k axpys).
//
// Implements (kernels.hpp): gram_ncols, gram_nwg, gram_update, hist_stage_rows, hist_coef, hist_combine, hist_reset.
#include "hist_core.hpp"
#include "internal.hpp"
#include "kernels.hpp"
#include "wave.hpp"

#include <algorithm>

namespace lbf {

// ---------------------------------------------------------------------------------------------
// History: Gram sweep.
// Each workgroup owns a contiguous chunk of the n coordinates. Phase 1 forms the new vectors
// (s = sa - sb, y = (ya - yb)*yscale, g = ga - gb + gc) for the chunk into LDS, writes s/y into the
// ring slot (and g to g_out), and accumulates their 6 mutual dots. Phase 2 streams every live
// history vector once (one wave per vector, 8 waves) against the three LDS vectors.
// Partial columns per workgroup: live logical index i -> [S_i.s, Y_i.s, S_i.y, Y_i.y, S_i.g, Y_i.g]
// at 6*i..6*i+5 (i < m), then [s.s, s.y, y.y, g.s, g.y, g.g] at 6*m..6*m+5.
// ---------------------------------------------------------------------------------------------
// History loads: nontemporal (NT) when the ring is far larger than the 256 MB Infinity Cache, so the
// once-read stream does not evict what the evaluation keeps there (MI355X_MICROARCH.md nt-weights;
// profiles/micro/streams.hip: 5.2 -> 5.7 TB/s on the cfg-5 ring).
template <bool NT>
__device__ __forceinline__ f32x4 hist_load(const float *p) {
  const f32x4 *q = reinterpret_cast<const f32x4 *>(p);
  if constexpr (NT)
    return __builtin_nontemporal_load(q);
  else
    return *q;
}
static bool hist_nt(const HistView &h) { return double(2 * h.m) * double(h.ld) * 4.0 > 512.0 * 1024 * 1024; }

static constexpr int GRAM_THREADS = 512;
// Largest chunk per workgroup (3 x chunk x 4 B of LDS; 1024-8192-element chunks measured alike,
// profiles/r02/c4_chunk*.json).
static long long gram_max_chunk() { return 4096; }

int gram_ncols(int m) { return 6 * m + 6; }
int gram_nwg(long long n) {
  long long w = cdiv(n, 1024);
  if (w > 2048) w = 2048;
  // More chunks than the chip holds workgroups at once (n = 10.49M: 2561 chunks, 3.33 rounds of 768): rounding the
  // count up to whole rounds measured no faster, 5.35-5.41 against 5.44-5.47 TB/s, profiles/r06/h/
  const long long need = cdiv(n, gram_max_chunk());
  if (w < need) w = need;
  return int(w < 1 ? 1 : w);
}
static long long gram_chunk(long long n, int nwg) { return cdiv(cdiv(n, nwg), 4) * 4; }

// The new vectors of one element: gram_kernel's arithmetic (s = sa - sb, y = (ya - yb) * yscale into the
// ring's write slot, g = ga - gb + gc into g_out), staged in LDS, self dots accumulated.
struct GramNew {
  float sv, yv, gv;
};
__device__ __forceinline__ GramNew gram_new(const GramArgs &a, float sa, float sb, float ya, float yb, float ga, float gb,
                                            float gc, float ysc) {
  GramNew r{0.f, 0.f, 0.f};
  if (a.has_pair) {
    r.sv = sa - sb;
    r.yv = (ya - yb) * ysc;
  }
  if (a.has_g) {
    r.gv = ga;
    if (a.gb) r.gv = r.gv - gb;
    if (a.gc) r.gv = r.gv + gc;
  }
  return r;
}

// tr: partials stored transposed, [ncols][gridDim.x] (each column contiguous for gram_fin's column sums);
// else [gridDim.x][ncols] (hist_step / fold_rows). vec: every operand and the ring 16-B aligned (host
// check), so the new vectors are formed from 16-B loads, all issued before the first use.
// MODE 0: the fused sweep (the new vectors formed into LDS and the ring, then the history). The split sweep
// (large n, gram_update): MODE 1 forms the new vectors, writes s, y into the ring slot (and g_out), and stores the
// self dots' partial row entries, with the same chunks, threads and block sum as MODE 0 (bitwise its self dots);
// MODE 2 then stages s, y, g of its chunk from memory into LDS and runs the history phase. The fused form's
// phase-1 stores, made between the history streams, cost the sweep far more than their bytes (5.2-5.7 TB/s
// against 5.8-6.0 split, profiles/micro/ring_ld.hip gram3p_*, profiles/r06/k2/).
template <int U, bool NT, int MODE = 0>
__global__ __launch_bounds__(GRAM_THREADS) void gram_kernel(const GramArgs a, long long chunk, double *partials, int tr,
                                                            int vec) {
  if (a.h.abort && *a.h.abort) return;
  KT(16);
  extern __shared__ __attribute__((aligned(16))) float sh[];
  __shared__ double scratch[6 * 16];
  __shared__ int order[COEF_MAXK]; // the live slots in logical order, staged once: no global load per vector below
  float *ls = sh, *ly = sh + chunk, *lg = sh + 2 * chunk;
  const HistView &h = a.h;
  const int ncols = 6 * h.m + 6;
  const long long e0 = (long long)blockIdx.x * chunk;
  const long long e1 = min(h.n, e0 + chunk);
  const int len = int(e1 > e0 ? e1 - e0 : 0);
  const int w = hist_write_slot(h.ist, h.m, a.policy, a.reset);
  const int count = a.reset ? 0 : h.ist[IST_COUNT];
  if (blockIdx.x == 0 && threadIdx.x == 0) h.ist[IST_WSLOT] = w;
  for (int i = threadIdx.x; i < count; i += blockDim.x) order[i] = h.ist[IST_ORDER + i]; // visible after block_sum

  double self[6] = {0, 0, 0, 0, 0, 0};
  float *Sw = h.S + (long long)w * h.ld + e0;
  float *Yw = h.Y + (long long)w * h.ld + e0;
  const float ysc = float(a.yscale);
  auto put = [&](int i, const GramNew &r) {
    if (MODE == 0) {
      ls[i] = r.sv;
      ly[i] = r.yv;
      lg[i] = r.gv;
    }
    const double s = r.sv, y = r.yv, g = r.gv;
    self[0] += s * s;
    self[1] += s * y;
    self[2] += y * y;
    self[3] += g * s;
    self[4] += g * y;
    self[5] += g * g;
  };
  int i_scalar = 0;
  if (MODE == 2) { // staged: s, y from the ring slot MODE 1 wrote, g from g_out / ga (zeros where MODE 0 has them)
    const float *gsrc = (a.gb || a.gc) ? a.g_out : a.ga;
    if (vec) {
      const int nq = len >> 2;
      for (int q = threadIdx.x; q < nq; q += GRAM_THREADS) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 s4 = a.has_pair ? *reinterpret_cast<const f32x4 *>(Sw + 4 * q) : z;
        const f32x4 y4 = a.has_pair ? *reinterpret_cast<const f32x4 *>(Yw + 4 * q) : z;
        const f32x4 g4 = a.has_g ? *reinterpret_cast<const f32x4 *>(gsrc + e0 + 4 * q) : z;
        *reinterpret_cast<f32x4 *>(ls + 4 * q) = s4;
        *reinterpret_cast<f32x4 *>(ly + 4 * q) = y4;
        *reinterpret_cast<f32x4 *>(lg + 4 * q) = g4;
      }
      i_scalar = 4 * nq;
    }
    for (int i = i_scalar + int(threadIdx.x); i < len; i += blockDim.x) {
      ls[i] = a.has_pair ? Sw[i] : 0.f;
      ly[i] = a.has_pair ? Yw[i] : 0.f;
      lg[i] = a.has_g ? gsrc[e0 + i] : 0.f;
    }
    __syncthreads();
  } else if (vec) { // two quads per thread per round, all seven operand loads of both issued up front
    const int nq = len >> 2;
    const float *dflt = a.ga ? a.ga : a.sa; // null operands read this and are masked
    for (int q0 = threadIdx.x; q0 < nq; q0 += 2 * GRAM_THREADS) {
      f32x4 op[2][7];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int q = min(q0 + u * GRAM_THREADS, nq - 1);
        const long long e = e0 + 4LL * q;
        const float *src[7] = {a.sa, a.sb, a.ya, a.yb, a.ga, a.gb, a.gc};
#pragma unroll
        for (int j = 0; j < 7; ++j) op[u][j] = *reinterpret_cast<const f32x4 *>((src[j] ? src[j] : dflt) + e);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int q = q0 + u * GRAM_THREADS;
        if (q >= nq) break;
        f32x4 s4, y4, g4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const GramNew r = gram_new(a, op[u][0][c], op[u][1][c], op[u][2][c], op[u][3][c], op[u][4][c], op[u][5][c],
                                     op[u][6][c], ysc);
          s4[c] = r.sv;
          y4[c] = r.yv;
          g4[c] = r.gv;
          put(4 * q + c, r);
        }
        if (a.has_pair) {
          *reinterpret_cast<f32x4 *>(Sw + 4 * q) = s4;
          *reinterpret_cast<f32x4 *>(Yw + 4 * q) = y4;
        }
        if (a.has_g && a.g_out) *reinterpret_cast<f32x4 *>(a.g_out + e0 + 4 * q) = g4;
      }
    }
    i_scalar = 4 * nq;
  }
  if (MODE != 2)
    for (int i = i_scalar + int(threadIdx.x); i < len; i += blockDim.x) {
      const long long e = e0 + i;
      const GramNew r = gram_new(a, a.has_pair ? a.sa[e] : 0.f, a.has_pair ? a.sb[e] : 0.f, a.has_pair ? a.ya[e] : 0.f,
                                 a.has_pair ? a.yb[e] : 0.f, a.has_g ? a.ga[e] : 0.f, a.gb ? a.gb[e] : 0.f,
                                 a.gc ? a.gc[e] : 0.f, ysc);
      if (a.has_pair) {
        Sw[i] = r.sv;
        Yw[i] = r.yv;
      }
      if (a.has_g && a.g_out) a.g_out[e] = r.gv;
      put(i, r);
    }
  KT(17);
  const long long rs = tr ? (long long)gridDim.x : 1LL; // column stride of the partial table
  double *out = partials + (tr ? (long long)blockIdx.x : (long long)blockIdx.x * ncols);
  if (MODE != 2) {
    block_sum<6>(self, scratch); // includes __syncthreads: LDS vectors complete after this
    KT(18);
    if (threadIdx.x == 0)
      for (int j = 0; j < 6; ++j) out[(6 * h.m + j) * rs] = self[j];
    if (MODE == 1) return;
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int v = wave; v < 2 * count; v += nw) {
    const int li = v < count ? v : v - count;
    const int slot = order[li];
    if (a.has_pair && slot == w) { // overwritten in this sweep (CUDA full ring): dots from the self block
      if (lane == 0) {
        out[(6 * li + (v < count ? 0 : 1)) * rs] = 0.0;
        out[(6 * li + (v < count ? 2 : 3)) * rs] = 0.0;
        out[(6 * li + (v < count ? 4 : 5)) * rs] = 0.0;
      }
      continue;
    }
    const float *V = (v < count ? h.S : h.Y) + (long long)slot * h.ld + e0;
    double ds = 0.0, dy = 0.0, dg = 0.0;
    const int full = len & ~3; // elements in whole 16-B quads
    for (int i0 = lane * 4; i0 < full; i0 += 256 * U) { // U independent 16-B loads in flight per lane
      f32x4 xs[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int iu = i0 + 256 * u;
        xs[u] = hist_load<NT>(V + (iu < full ? iu : 0)); // clamped, masked below: no per-load branch
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int iu = i0 + 256 * u;
        if (iu < full) {
          const f32x4 s4 = *reinterpret_cast<const f32x4 *>(ls + iu);
          const f32x4 y4 = *reinterpret_cast<const f32x4 *>(ly + iu);
          const f32x4 g4 = *reinterpret_cast<const f32x4 *>(lg + iu);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double xv = xs[u][j];
            ds += xv * double(s4[j]);
            dy += xv * double(y4[j]);
            dg += xv * double(g4[j]);
          }
        }
      }
    }
    if (full < len && lane == ((full >> 2) & 63)) { // the partial quad, on the lane whose stride reaches it
      for (int j = full; j < len; ++j) {
        const double xv = V[j];
        ds += xv * double(ls[j]);
        dy += xv * double(ly[j]);
        dg += xv * double(lg[j]);
      }
    }
    ds = wave_sum_f64(ds);
    dy = wave_sum_f64(dy);
    dg = wave_sum_f64(dg);
    if (lane == 0) {
      const int c = v < count ? 0 : 1;
      out[(6 * li + c + 0) * rs] = ds;
      out[(6 * li + c + 2) * rs] = dy;
      out[(6 * li + c + 4) * rs] = dg;
    }
  }
  KT(19);
}

void gram_update(hipStream_t s, const GramArgs &a, double *partials, int transposed) {
  const int nwg = gram_nwg(a.h.n);
  const long long chunk = gram_chunk(a.h.n, nwg);
  const size_t shmem = size_t(3 * chunk) * sizeof(float);
  // 16-B loads in flight per lane while streaming a history vector (8 measured the same as 4,
  // profiles/r03/two_loop_gramU8.jsonl)
  if (shmem > 64 * 1024) { // once per process, thread-safe
    static const bool attr_set = [] {
      for (const void *f : {reinterpret_cast<const void *>(gram_kernel<4, false>),
                            reinterpret_cast<const void *>(gram_kernel<4, true>),
                            reinterpret_cast<const void *>(gram_kernel<4, false, 2>),
                            reinterpret_cast<const void *>(gram_kernel<4, true, 2>)})
        LBF_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
      return true;
    }();
    (void)attr_set;
  }
  const bool nt = hist_nt(a.h);
  const int vec = (a.ga || a.sa) && chunk % 4 == 0 && a.h.ld % 4 == 0 &&
                  aligned16(a.h.S, a.h.Y, a.sa, a.sb, a.ya, a.yb, a.ga, a.gb, a.gc, a.g_out); // null passes
  const int tr = transposed ? 1 : 0;
  // the split sweep (MODE 1 then 2) for the large-n history, where g is readable afterwards (ga, or g_out when formed)
  // (long histories only: at m = 10 the extra launch and the three staged reads cost what the split saves, two-loop
  // 56.9-57.5 % split against 57.1-58.1 % fused; m = 50 68.9-69.6 % against 67.2-67.3 %, profiles/r06/m/)
  if (vec && a.h.n >= (1LL << 21) && a.h.m >= 20 && !(a.has_g && (a.gb || a.gc) && !a.g_out)) {
    const dim3 g1{unsigned(nwg), 1, 1}, b1{unsigned(GRAM_THREADS), 1, 1};
    if (nt) {
      hipLaunchKernelGGL((gram_kernel<4, true, 1>), g1, b1, 0, s, a, chunk, partials, tr, vec);
      hipLaunchKernelGGL((gram_kernel<4, true, 2>), g1, b1, shmem, s, a, chunk, partials, tr, vec);
    } else {
      hipLaunchKernelGGL((gram_kernel<4, false, 1>), g1, b1, 0, s, a, chunk, partials, tr, vec);
      hipLaunchKernelGGL((gram_kernel<4, false, 2>), g1, b1, shmem, s, a, chunk, partials, tr, vec);
    }
    LBF_KERNEL_CHECK();
    return;
  }
  if (nt)
    hipLaunchKernelGGL((gram_kernel<4, true>), dim3(nwg), dim3(GRAM_THREADS), shmem, s, a, chunk, partials, tr, vec);
  else
    hipLaunchKernelGGL((gram_kernel<4, false>), dim3(nwg), dim3(GRAM_THREADS), shmem, s, a, chunk, partials, tr, vec);
  LBF_KERNEL_CHECK();
}

// ---------------------------------------------------------------------------------------------
// History step (one workgroup): (A) reduce the Gram sweep's per-workgroup partials, then the push and
// the two-loop recurrences of hist_core.hpp.
// ---------------------------------------------------------------------------------------------
static constexpr int HIST_STAGE_DOUBLES = 4096;   // up to 32 KB of partial rows staged per round
static constexpr int HIST_STATIC_LDS = 16 * 1024; // bound on the kernel's static LDS
static constexpr int HIST_PRE_UNROLL = 11;        // fused path: (m+1)^2 <= 256 * 11, i.e. m <= 52

__global__ __launch_bounds__(256) void hist_step_kernel(const CoefArgs a) {
  if (a.h.abort && *a.h.abort) return;
  KT(0);
  extern __shared__ double sy[]; // [k][k] live s_i . y_j after the push (logical order), then staging
  __shared__ HistSmem sm;
  const HistView &h = a.h;
  const int t = threadIdx.x;
  HistStep st;
  st.h = a.h;
  st.has_pair = a.has_pair;
  st.has_g = a.has_g;
  st.reset = a.reset;
  st.policy = a.policy;
  st.want_dir = a.want_dir;
  st.iter = a.iter;
  st.dsign = a.dsign;
  // fused: SY, YY and rho go to LDS (after the SY block and the staging area) with the prologue's
  // loads, one round trip for all of them; the recurrences then read LDS only
  constexpr int PU = HIST_PRE_UNROLL;
  const int S_ = h.slots, SS = S_ * S_;
  double *pre = sy + a.sy_cap + a.stage;
  double psy[PU], pyy[PU], prho = 0.0;
  if (a.fused) {
#pragma unroll
    for (int u = 0; u < PU; ++u) { // clamped, unconditional: no branch and wait per load
      const int i = min(t + 256 * u, SS - 1);
      psy[u] = h.SY[i];
      pyy[u] = h.YY[i];
    }
    prho = h.rho[min(t, S_ - 1)];
  }
  // Step A's partial rows in the same round trip when they fit one staging round (the folded table, History::
  // update): every column, the live ones picked after the prologue
  constexpr int AU = HIST_STAGE_DOUBLES / 256;
  const int ncols = 6 * h.m + 6, tot_all = a.nwg * ncols;
  const bool one_round = tot_all <= a.stage && tot_all <= 256 * AU;
  double pa[AU];
  if (one_round) {
#pragma unroll
    for (int u = 0; u < AU; ++u) pa[u] = a.partials[min(t + 256 * u, tot_all - 1)];
  }
  hist_prologue(st, sm, h.ist[IST_WSLOT]);
  if (a.fused) {
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      const int i = t + 256 * u;
      if (i < SS) {
        pre[i] = psy[u];
        pre[SS + i] = pyy[u];
      }
    }
    if (t < S_) pre[2 * SS + t] = prho;
  }
  KT(1);
  const int count0 = sm.count0;
  // ---- A: reduce the columns in use. Tiles of partial rows are staged into LDS with every load in
  // flight at once (one global round trip per tile), then thread q sums column q in row order. ----
  const int nneed = 6 * count0 + 6;
  double *stage = sy + a.sy_cap; // dynamic LDS after the SY block(s)
  const int rt = max(1, min(a.nwg, a.stage / nneed));
  double colacc[(6 * COEF_MAXK + 6 + 255) / 256];
#pragma unroll
  for (int i = 0; i < (6 * COEF_MAXK + 6 + 255) / 256; ++i) colacc[i] = 0.0;
  if (one_round) { // the same sums in the same row order as the rounds below
#pragma unroll
    for (int u = 0; u < AU; ++u)
      if (t + 256 * u < tot_all) stage[t + 256 * u] = pa[u];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < (6 * COEF_MAXK + 6 + 255) / 256; ++i) {
      const int q = t + 256 * i;
      if (q < nneed) {
        const int col = q < 6 * count0 ? q : 6 * h.m + (q - 6 * count0);
        for (int r = 0; r < a.nwg; ++r) colacc[i] += stage[r * ncols + col];
      }
    }
    __syncthreads();
  }
  for (int r0 = 0; !one_round && r0 < a.nwg; r0 += rt) {
    const int rows = min(rt, a.nwg - r0);
    const int tot = rows * nneed;
    for (int e0 = t; e0 < tot; e0 += 256 * 8) { // 8 independent loads in flight per thread
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { // unconditional (clamped) loads: no branch and wait per load
        const int e = min(e0 + 256 * u, tot - 1);
        const int r = e / nneed, q = e - r * nneed;
        const int col = q < 6 * count0 ? q : 6 * h.m + (q - 6 * count0);
        v[u] = a.partials[(long long)(r0 + r) * ncols + col];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (e0 + 256 * u < tot) stage[e0 + 256 * u] = v[u];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < (6 * COEF_MAXK + 6 + 255) / 256; ++i) {
      const int q = t + 256 * i;
      if (q < nneed)
        for (int r = 0; r < rows; ++r) colacc[i] += stage[r * nneed + q];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < (6 * COEF_MAXK + 6 + 255) / 256; ++i) {
    const int q = t + 256 * i;
    if (q < nneed) sm.dots[q < 6 * count0 ? q : 6 * h.m + (q - 6 * count0)] = colacc[i];
  }
  __syncthreads();
  KT(2);
  if (a.fused) {
    st.SY = pre;
    st.YY = pre + SS;
    st.rho = pre + 2 * SS;
    hist_core<true>(st, sm, sy, a.sy_cap, stage, a.stage);
  } else {
    hist_core<false>(st, sm, sy, a.sy_cap, stage, a.stage);
  }
}

// The history step's dynamic LDS for history size m with S slots, in doubles: [sy_cap | stage | pre]. fused: the step
// with LDS-prefetched sources and stores off wave 0, when the direction is wanted and SY (with its transpose), a full
// staging area and the prefetch (pre) all fit. sy_cap: SY and its transpose when they fit beside a full staging area;
// else (m = 100) hist_core's compact layout (SY with stride m + 1, YY's lower triangle): step A keeps many rows.
struct HistLds {
  bool fused;
  long long sy_cap, stage, pre;
};
static HistLds hist_lds(int m, long long S, bool want_dir) {
  const long long total = (160 * 1024 - HIST_STATIC_LDS) / 8, m2 = (long long)m * m;
  const long long need_stage = 6LL * m + 6, pre = 2 * S * S + S;
  const bool fused = want_dir && S * S <= 256LL * HIST_PRE_UNROLL && 2 * m2 + HIST_STAGE_DOUBLES + pre <= total;
  const long long avail = total - (fused ? pre : 0);
  const long long big = (long long)m * (m + 1) + ((long long)m * (m + 1)) / 2;
  long long sy_cap = big;
  if (2 * m2 + HIST_STAGE_DOUBLES <= avail || big + 4 * need_stage > avail)
    sy_cap = std::min(2 * m2, avail - need_stage);
  return {fused, sy_cap, std::min<long long>(HIST_STAGE_DOUBLES, avail - sy_cap), pre};
}

// Partial rows of the Gram table that one staging round of the history step holds (History::update
// folds taller tables to this many rows first, so step A is one round trip).
int hist_stage_rows(int m) { return int(std::max(1LL, hist_lds(m, m + 1, true).stage / (6LL * m + 6))); }

void hist_coef(hipStream_t s, const CoefArgs &a) {
  LBF_REQUIRE(a.h.m <= COEF_MAXK, "history size m must be <= 128");
  static const bool attr_set = [] { // once per process, thread-safe
    LBF_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(hist_step_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - HIST_STATIC_LDS));
    return true;
  }();
  (void)attr_set;
  CoefArgs c = a;
  const HistLds l = hist_lds(a.h.m, a.h.slots, a.want_dir == 1);
  c.fused = l.fused ? 1 : 0;
  c.sy_cap = int(l.sy_cap);
  LBF_REQUIRE(l.sy_cap >= (long long)a.h.m * a.h.m, "hist_step: LDS too small for the SY block");
  c.stage = int(l.stage);
  const size_t shmem = size_t(l.sy_cap + l.stage + (l.fused ? l.pre : 0)) * sizeof(double);
  hipLaunchKernelGGL(hist_step_kernel, dim3(1), dim3(256), shmem, s, c);
  LBF_KERNEL_CHECK();
}
// ---------------------------------------------------------------------------------------------
// History: linear-combination sweep  dir = sum_i cs_i S_i + cy_i Y_i + cg g  (fp64 per element),
// fused with the trial point x_out = x_in + alpha*dir (and an optional second copy).
// ---------------------------------------------------------------------------------------------

// Large-n combine with the Gram sweep's access pattern (round 6). A grid striding over the elements, one quad of
// every live vector per lane (1 KB of one vector per wave-instruction), has the chip touch every vector at the
// same few offsets at once, a pattern that streams at 5.45 TB/s against 6.7 TB/s for the Gram sweep's (each wave 4-16 KB contiguous of one vector; profiles/micro/ring_ld.hip, profiles/r06/d/, o/).
// Here a workgroup owns 4096-element chunks (grid-stride over the resident grid): wave w the 1024 elements
// c0 + 1024 w .., lane l the quads 256 u + 4 l (u < 4), so each vector is read as 4 KB contiguous per wave and
// 16 KB per workgroup, V vectors' quads (2 V x 4 loads) in flight per lane. Per element one fp64 sum in a fixed
// order: cg g, then cs_i S_i + cy_i Y_i for i = 0 .. k - 1.
template <int V, bool NT, int Q = 4>
__global__ __launch_bounds__(256) void combine_chunk_kernel(const CombineArgs a) {
  if (a.h.abort && *a.h.abort) return;
  __shared__ double cs[COEF_MAXK], cy[COEF_MAXK];
  __shared__ int L[COEF_MAXK];
  const HistView &h = a.h;
  const int S_ = h.slots;
  const int k = h.ist[IST_COUNT];
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    cs[i] = h.coef[i];
    cy[i] = h.coef[S_ + i];
    L[i] = h.ist[IST_ORDER + i];
  }
  __syncthreads();
  const double cg = h.coef[2 * S_];
  const double alpha = a.alpha_from_state ? h.scal[SC_ALPHA0] : a.alpha;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float *xsrc = a.x_out ? a.x_in : a.g;
  constexpr int CH = 1024 * Q; // elements per chunk: wave w the 256 Q contiguous elements c0 + 256 Q w ..
  for (long long c0 = (long long)blockIdx.x * CH; c0 < h.n; c0 += (long long)gridDim.x * CH) {
    long long e[Q], ec[Q];
    bool full[Q];
#pragma unroll
    for (int u = 0; u < Q; ++u) {
      e[u] = c0 + wave * 256 * Q + u * 256 + 4 * lane;
      full[u] = e[u] + 3 < h.n;
      ec[u] = full[u] ? e[u] : 0; // clamped: loads unconditional, results masked
    }
    double acc[Q][4];
#pragma unroll
    for (int u = 0; u < Q; ++u) {
      const f32x4 g4 = *reinterpret_cast<const f32x4 *>(a.g + ec[u]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[u][j] = cg * double(g4[j]);
    }
    int i = 0;
    for (; i + V <= k; i += V) {
      f32x4 s4[V][Q], y4[V][Q];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const long long sb = (long long)L[i + v] * h.ld;
#pragma unroll
        for (int u = 0; u < Q; ++u) {
          s4[v][u] = hist_load<NT>(h.S + sb + ec[u]);
          y4[v][u] = hist_load<NT>(h.Y + sb + ec[u]);
        }
      }
#pragma unroll
      for (int v = 0; v < V; ++v)
#pragma unroll
        for (int u = 0; u < Q; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[u][j] += cs[i + v] * double(s4[v][u][j]) + cy[i + v] * double(y4[v][u][j]);
    }
    for (; i < k; ++i) {
      const long long sb = (long long)L[i] * h.ld;
#pragma unroll
      for (int u = 0; u < Q; ++u) {
        const f32x4 s4 = hist_load<NT>(h.S + sb + ec[u]);
        const f32x4 y4 = hist_load<NT>(h.Y + sb + ec[u]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[u][j] += cs[i] * double(s4[j]) + cy[i] * double(y4[j]);
      }
    }
#pragma unroll
    for (int u = 0; u < Q; ++u) {
      if (full[u]) {
        f32x4 d4;
#pragma unroll
        for (int j = 0; j < 4; ++j) d4[j] = float(acc[u][j]);
        if (a.dir) *reinterpret_cast<f32x4 *>(a.dir + e[u]) = d4;
        if (a.x_out) {
          const f32x4 x4 = *reinterpret_cast<const f32x4 *>(xsrc + e[u]);
          const f32x4 o4 = x4 + float(alpha) * d4;
          *reinterpret_cast<f32x4 *>(a.x_out + e[u]) = o4;
          if (a.x_out2) *reinterpret_cast<f32x4 *>(a.x_out2 + e[u]) = o4;
        }
      } else {
        for (long long q = e[u]; q < h.n && q < e[u] + 4; ++q) { // the tail quad, element-wise (no read past n)
          double ac = cg * double(a.g[q]);
          for (int ii = 0; ii < k; ++ii)
            ac += cs[ii] * double(h.S[(long long)L[ii] * h.ld + q]) + cy[ii] * double(h.Y[(long long)L[ii] * h.ld + q]);
          const float d = float(ac);
          if (a.dir) a.dir[q] = d;
          if (a.x_out) {
            const float o = a.x_in[q] + float(alpha) * d;
            a.x_out[q] = o;
            if (a.x_out2) a.x_out2[q] = o;
          }
        }
      }
    }
  }
}

// Small-n form (the latency-bound regime: n up to a few million, k <= 32): one element per lane so
// the grid covers every CU, the ring header and coefficients read lane-distributed (no LDS, no
// barrier) and broadcast with v_readlane, and every history load of the lane issued at once: one
// round trip for the header, one for the data.
// WW: x_out's w.w partials (one word per block: 256 elements == ww_block_elems(n) for every n of this form).
template <int KMAX, bool WW = false>
__global__ __launch_bounds__(256) void combine_small_kernel(const CombineArgs a) {
  // the speculative chain's abort flag: requested with the header, g and x (one round trip for all) and
  // tested before the history loads, so an aborted launch exits after that round trip
  const int abf = abort_flag(a.h.abort);
  const HistView &h = a.h;
  const int S_ = h.slots, lane = threadIdx.x & 63;
  const long long e0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = e0 < h.n;
  const long long e = in ? e0 : h.n - 1; // loads are unconditional (clamped), results masked
  // independent of the header: in flight with it
  const float gv = a.g[e];
  const float xv = (a.x_out ? a.x_in : a.g)[e];
  const int lk = lane < h.m ? lane : 0; // header entries read without waiting for the count
  const int k = __builtin_amdgcn_readfirstlane(h.ist[IST_COUNT]);
  const int Lr = h.ist[IST_ORDER + lk];
  const double csr = h.coef[lk], cyr = h.coef[S_ + lk];
  const double cg = h.coef[2 * S_];
  const double alpha = a.alpha_from_state ? h.scal[SC_ALPHA0] : a.alpha;
  if (aborted(abf)) return; // uniform for the launch
  float sv[KMAX], yv[KMAX];
  if (k > 0) {
#pragma unroll
    for (int i = 0; i < KMAX; ++i) { // every load issued before the first use
      const long long off = (long long)__builtin_amdgcn_readlane(Lr, i < k ? i : k - 1) * h.ld + e;
      sv[i] = h.S[off];
      yv[i] = h.Y[off];
    }
  }
  double acc = cg * double(gv);
#pragma unroll
  for (int i = 0; i < KMAX; ++i)
    if (i < k) acc += lane_f64(csr, i) * double(sv[i]) + lane_f64(cyr, i) * double(yv[i]);
  if constexpr (WW) {
    const float d = float(acc), o = xv + float(alpha) * d;
    if (in) {
      if (a.dir) a.dir[e] = d;
      a.x_out[e] = o;
      if (a.x_out2) a.x_out2[e] = o;
    }
    ww_block_store(in ? double(o) * double(o) : 0.0, a.ww_part);
    return;
  }
  if (!in) return;
  const float d = float(acc);
  if (a.dir) a.dir[e] = d;
  if (a.x_out) {
    const float o = xv + float(alpha) * d;
    a.x_out[e] = o;
    if (a.x_out2) a.x_out2[e] = o;
  }
}

// The streaming regime with g, dir, x_in, x_out or x_out2 off a 16-B boundary (a caller's pointer, lbf_two_loop):
// one element per thread, grid-stride, every access 4 bytes; the fp64 sum in combine_chunk_kernel's order (bitwise
// its result).
__global__ __launch_bounds__(256) void combine_elem_kernel(const CombineArgs a) {
  if (a.h.abort && *a.h.abort) return;
  __shared__ double cs[COEF_MAXK], cy[COEF_MAXK];
  __shared__ int L[COEF_MAXK];
  const HistView &h = a.h;
  const int S_ = h.slots;
  const int k = h.ist[IST_COUNT];
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    cs[i] = h.coef[i];
    cy[i] = h.coef[S_ + i];
    L[i] = h.ist[IST_ORDER + i];
  }
  __syncthreads();
  const double cg = h.coef[2 * S_];
  const double alpha = a.alpha_from_state ? h.scal[SC_ALPHA0] : a.alpha;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < h.n; q += (long long)gridDim.x * blockDim.x) {
    double ac = cg * double(a.g[q]);
    for (int i = 0; i < k; ++i)
      ac += cs[i] * double(h.S[(long long)L[i] * h.ld + q]) + cy[i] * double(h.Y[(long long)L[i] * h.ld + q]);
    const float d = float(ac);
    if (a.dir) a.dir[q] = d;
    if (a.x_out) {
      const float o = a.x_in[q] + float(alpha) * d;
      a.x_out[q] = o;
      if (a.x_out2) a.x_out2[q] = o;
    }
  }
}

static void combine_stream(hipStream_t s, const CombineArgs &a); // n > 2^21 or m > 32

void hist_combine(hipStream_t s, const CombineArgs &ca) {
  LBF_REQUIRE(ca.h.ld % 4 == 0, "history slot stride must be a multiple of 4");
  LBF_REQUIRE(!ca.ww_part || ca.x_out, "hist_combine: w.w partials need x_out");
  if (ca.h.n <= (1LL << 21) && ca.h.m <= 32) {
    const dim3 g1(unsigned(cdiv(ca.h.n, 256)));
    if (ca.ww_part) {
      if (ca.h.m <= 16)
        hipLaunchKernelGGL((combine_small_kernel<16, true>), g1, dim3(256), 0, s, ca);
      else
        hipLaunchKernelGGL((combine_small_kernel<32, true>), g1, dim3(256), 0, s, ca);
    } else if (ca.h.m <= 16)
      hipLaunchKernelGGL((combine_small_kernel<16>), g1, dim3(256), 0, s, ca);
    else
      hipLaunchKernelGGL((combine_small_kernel<32>), g1, dim3(256), 0, s, ca);
    LBF_KERNEL_CHECK();
    return;
  }
  // the streaming forms: x_out's partials in a launch of their own behind the combine (abort-aware like it)
  combine_stream(s, ca);
  if (ca.ww_part) ww_partials(s, ca.h.n, ca.x_out, ca.ww_part, ca.h.abort);
}

static void combine_stream(hipStream_t s, const CombineArgs &a) {
  // 2 vectors x 4 quads in flight per lane: measured against 1 x 4, 2 x 2 and 4 x 2 (m = 50: 69.9-70.0 % against
  // 69.5-69.9, 67.3-67.6, 66.7-66.8 %; profiles/r06/o/)
  static const long long resident = [] { // workgroups of combine_chunk_kernel the chip holds at once, once
    int dev = 0, cus = 0, p1 = 0, p2 = 0;
    LBF_HIP(hipGetDevice(&dev));
    LBF_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    LBF_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&p1, combine_chunk_kernel<2, true>, 256, 0));
    LBF_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&p2, combine_chunk_kernel<2, false>, 256, 0));
    return (long long)std::max(1, cus) * std::max(1, std::min(p1, p2));
  }();
  const dim3 grid(unsigned(std::min(cdiv(a.h.n, 4096LL), resident)));
  if (!aligned16(a.g, a.dir, a.x_in, a.x_out, a.x_out2)) { // null passes; the ring is the engine's own
    hipLaunchKernelGGL(combine_elem_kernel, dim3(unsigned(std::min(cdiv(a.h.n, 256LL), 16 * resident))), dim3(256), 0, s, a);
    LBF_KERNEL_CHECK();
    return;
  }
  if (hist_nt(a.h))
    hipLaunchKernelGGL((combine_chunk_kernel<2, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((combine_chunk_kernel<2, false>), grid, dim3(256), 0, s, a);
  LBF_KERNEL_CHECK();
}

__global__ void hist_reset_kernel(HistView h) {
  h.ist[IST_COUNT] = 0;
  h.ist[IST_FREE] = 0;
  h.ist[IST_WSLOT] = 0;
  h.scal[SC_COUNT] = 0.0;
}
void hist_reset(hipStream_t s, const HistView &h) {
  hipLaunchKernelGGL(hist_reset_kernel, dim3(1), dim3(1), 0, s, h);
  LBF_KERNEL_CHECK();
}

} // namespace lbf

#ifdef LBF_KTRACE
extern "C" int lbf_dbg_ktrace(unsigned long long *host, int n) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(lbf::lbf_kt_buf), size_t(n) * 8) == hipSuccess ? 0 : 1;
}
#endif
