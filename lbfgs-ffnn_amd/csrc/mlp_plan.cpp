// Mlp: layers, the tile / split-K plan, the workspace and the layer GEMM descriptors (see runtime.hpp).
#include "runtime.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace lbf {

Mlp::Mlp(Ctx *ctx, int nl, const int *dims, const int *acts, const Switches &sw)
    : ctx_(ctx), group_dw_(sw.group_dw), fold_on_(sw.fold), show_plan_(sw.show_plan) {
  LBF_REQUIRE(nl >= 1 && nl <= 16, "1..16 layers");
  size_t off = 0;
  for (int l = 0; l < nl; ++l) {
    LBF_REQUIRE(dims[l] > 0 && dims[l + 1] > 0, "layer dims must be positive");
    LBF_REQUIRE(acts[l] >= 0 && acts[l] < ACT_COUNT, "activation id 0..6");
    Layer L;
    L.in = dims[l];
    L.out = dims[l + 1];
    L.act = acts[l];
    L.off = off;
    off += size_t(L.in + 1) * L.out;
    layers_.push_back(L);
  }
  nparams_ = off;
}

void Mlp::set_l2(double l2) {
  LBF_REQUIRE(std::isfinite(l2) && l2 >= 0.0, "l2 must be finite and >= 0");
  l2_ = l2;
}

void Mlp::set_loss(int loss) {
  LBF_REQUIRE(loss == LOSS_MSE || loss == LOSS_XENT, "unknown loss");
  if (loss == LOSS_XENT) {
    const Layer &Lo = layers_.back();
    LBF_REQUIRE(Lo.act == ACT_LINEAR, "softmax cross-entropy needs a linear last layer (the logits)");
    LBF_REQUIRE(Lo.out >= 2, "softmax cross-entropy needs at least two outputs");
  }
  loss_ = loss;
}

// Split-K factor for `tiles` output tiles over a K of `K` rows: the GEMM tiles run two workgroups per
// CU, so a launch is ceil(tiles * s / slots) waves of equal-length workgroups; choose s (chunks of at
// least min_chunk rows, slabs within a memory cap) to maximise tiles * s / (waves * slots), the
// smallest s within half a percent of the best. A count just past a multiple of the slots (e.g. 520
// workgroups on 512 slots) would otherwise cost a whole extra wave.
static long long split_factor(long long tiles, long long K, long long min_chunk, long long slots,
                              long long slab_elems_per_split) {
  const long long cap_elems = 1LL << 29; // 2 GiB of fp32 slabs
  long long smax = std::max(1LL, std::min(cdiv(K, min_chunk), 4 * slots));
  if (slab_elems_per_split > 0) smax = std::max(1LL, std::min(smax, cap_elems / slab_elems_per_split));
  long long best = 1;
  double best_eff = 0.0;
  for (long long s = 1; s <= smax; ++s) {
    const long long wg = tiles * s, waves = cdiv(wg, slots);
    const double eff = double(wg) / double(waves * slots);
    if (eff > best_eff + 0.005) {
      best_eff = eff;
      best = s;
    }
  }
  return best;
}

// Batches up to this many rows are "small" for the dW plan (64x64 tiles, k chunks of two k-tiles).
constexpr long long DW_SMALL_BATCH = 2048;

// Forward plan (split-K for few row tiles), the EPI_HEAD fold, then the split-K plan of every dW GEMM
// for batch B (workgroup-slot aware, split_factor), k chunks a multiple of the 32-deep LDS tile.
void Mlp::plan(long long B) {
  if (planned_ == B) return;
  size_t slab = 0, fslab = 0;
  const int nl = int(layers_.size());
  const bool fused = head_route();
  const long long slots = 2LL * ctx_->cus;
  for (auto &L : layers_) {
    // forward GEMM: with fewer row tiles than CUs (a data-parallel rank's shard), split K so the chip
    // fills; the partial slabs are summed in split order with the bias and activation afterwards
    int fBM, fBN;
    gemm_tile_for(L.out, TILE_AUTO, &fBM, &fBN);
    const long long ftiles = cdiv(B, 128) * cdiv(L.out, fBN);
    L.fsplits = 1;
    L.fk_chunk = L.in;
    L.ftile = TILE_AUTO;
    // Row-tile height for layers 65..128 wide (one column tile of 128, where the head can fuse). A small
    // tile is bound by its per-CU operand delivery (~22 GB/s per CU for the LDS-DMA stream,
    // profiles/r02/gemm_small_tiles.txt), a 128-row tile by the MFMA issue, so the plan takes the tile
    // with the shortest estimated launch: n = the most tiles any CU gets, each costing a measured time per
    // 32-deep k-tile, plus one epilogue per round of co-resident workgroups (one per CU for 32 x 128,
    // two otherwise). Constants: 784 -> 128 with the fused head on MI355X (profiles/r02/
    // gemm_fwd_tiles_by_shard.txt, tile64_*.json, tilemodel_*.json): 32 x 128 at 7500 rows (one round),
    // 64 x 128 at 15000-40000 rows (forward 63.5 -> 48.4 us at 15000, 120.4 -> 77.9 at 30000,
    // 132.4 -> 112.7 at 40000), 128 x 128 at 60000 (137 against 144.5 with 64-row tiles). Layers up to 64
    // wide keep the round-1 rule (32-row tiles below 256 row tiles of 128, else 128 x 64 / 128 x 32).
    const long long cus = ctx_->cus, nkt = cdiv(L.in, 32);
    auto est_us = [&](long long bm, double per_ktile, long long per_round, double epi) {
      const long long n = cdiv(cdiv(B, bm), cus);
      return double(n) * per_ktile * double(nkt) + double(cdiv(n, per_round)) * epi;
    };
    if (L.out > 64 && L.out <= 128) {
      const double t32 = est_us(32, 0.93, 1, 8.0), t64 = est_us(64, 1.25, 2, 12.0), t128 = est_us(128, 2.3, 2, 20.0);
      if (t32 <= t64 && t32 <= t128) L.ftile = TILE_32x128; // full rows (the head can still fuse), no split
      else if (t64 <= t128) L.ftile = TILE_64x128;
    } else if (L.out <= 64 && cdiv(B, 128) < 256) {
      L.ftile = TILE_32x128;
    }
    if (L.ftile != TILE_AUTO) {
      // no split: the fused head and the activation need the full K
    } else if (ftiles < 192 && L.in >= 256) {
      // Few rows of a wide layer (S-LBFGS minibatches: 256 x 784 -> 512 is 8 tiles of 128 x 128): split
      // K. With 32 x 128 tiles the rows make 4x the tiles, so fewer, longer splits fill the chip (one
      // workgroup per CU) and the slabs are a quarter of the bytes of 128 x 128 tiles at the same count.
      const long long tiles32 = cdiv(B, 32) * cdiv(L.out, 128);
      long long fs;
      if (2 * tiles32 <= cus) {
        L.ftile = TILE_32x128;
        fs = std::max(2LL, std::min(cus / tiles32, cdiv(L.in, 64))); // splits of >= 2 k-tiles
      } else {
        fs = std::min(cdiv(384, ftiles), (long long)L.in / 128);
      }
      long long fkc = cdiv(cdiv(L.in, fs), 32) * 32;
      fs = cdiv(L.in, fkc);
      if (fs > 1) {
        L.fsplits = int(fs);
        L.fk_chunk = int(fkc);
        fslab = std::max(fslab, size_t(fs) * size_t(B) * L.out);
      }
    }
    // dW: 64x64 tiles over narrow outputs -> fewer, longer K splits (a third of the slab traffic)
    // (only for short K: at long K the 128x128 tile's reuse wins over the slab savings). Small batches
    // (S-LBFGS minibatches, K = 128 / 256 rows) take 64x64 tiles at any width: four times the tiles of
    // 128x128 at the same K, where 128x128 tiles filled a fifth of the chip (784 -> 512: 56 workgroups).
    L.dtile = ((L.out <= 128 && L.in + 1 <= 1024 && B <= 16384) || B <= DW_SMALL_BATCH) ? TILE_64x64 : TILE_AUTO;
    // (128 x 128 tiles with two k-groups and one workgroup per CU, half the split-K slabs, measured slower at
    // cfg 2: dW 128.5 against 112.2 us, profiles/r04/a/bench_400{,_nok2}.json; not kept)
  }
  // The last hidden layer's dW GEMM has in + 1 rows; when they pass a multiple of its tile height by
  // at most 16 input columns + the bias row (784 + 1 = 6 x 128 + 17 at cfg 2), those rows go to the
  // EPI_HEAD epilogue, which holds delta in registers, instead of a last row tile that would be
  // mostly padding (a seventh of the dW GEMM's MFMA work at cfg 2).
  fold_ = -1;
  fold_c0_ = 0;
  if (fold_on_ && gemm_head_on()) {
    const Layer &L = layers_[size_t(nl - 2)];
    int BM, BN;
    gemm_tile_for(L.out, L.dtile, &BM, &BN);
    const int c0 = L.in / BM * BM;
    if (c0 > 0 && L.in - c0 <= 16 && L.in % 4 == 0 && L.out <= 128) {
      fold_ = L.in - c0;
      fold_c0_ = c0;
    }
  }
  // dW tiles and split-K, last layer first: layer l's launch also carries the side blocks that finish
  // layer l+1's slabs (side_reduced), and those take workgroup slots too
  for (int l = nl - 1; l >= 0; --l) {
    Layer &L = layers_[l];
    int BM, BN;
    const long long M = (fold_ >= 0 && l == nl - 2) ? fold_c0_ : L.in + 1;
    gemm_tile_for(L.out, L.dtile, &BM, &BN);
    const long long tiles = cdiv(M, BM) * cdiv(L.out, BN);
    const long long min_chunk = L.dtile == TILE_64x64 ? (B <= DW_SMALL_BATCH ? 64 : 256) : 128;
    long long side = 0;
    if (side_reduced(l + 1, fused)) {
      const Layer &N1 = layers_[l + 1];
      long long cols = (long long)(N1.in + 1) * N1.out;
      if (fold_ >= 0 && l == nl - 2) cols += (long long)(fold_ + 1) * L.out;
      side = cdiv(cdiv(cols, 256), tiles) * tiles; // gemm.hip SIDE_COLS per side block
    }
    long long splits = split_factor(tiles, B, min_chunk, std::max(slots - side, slots / 2), M * L.out);
    long long kc = cdiv(cdiv(B, splits), 32) * 32;
    if (kc <= 0) kc = 32;
    splits = std::max(1LL, cdiv(B, kc));
    L.splits = int(splits);
    L.k_chunk = int(kc);
  }
  for (auto &L : layers_) {
    L.slab_off = slab;
    if (L.splits > 1) slab += size_t(L.splits) * size_t(L.in + 1) * L.out; // every layer keeps its own slabs
  }
  if (show_plan_) {
    for (int l = 0; l < nl; ++l) {
      std::fprintf(stderr, "[lbf plan] B=%lld layer %d: dW tile %d splits %d k_chunk %d | fwd tile %d splits %d", B, l,
                   layers_[l].dtile, layers_[l].splits, layers_[l].k_chunk, layers_[l].ftile, layers_[l].fsplits);
      if (l >= 1) std::fprintf(stderr, " | dX tile %d", dx_tile(B, layers_[l].in)); // layer 0 has no dX GEMM
      std::fprintf(stderr, "\n");
    }
    std::fprintf(stderr, "[lbf plan] B=%lld fold %d from column %d\n", B, fold_, fold_c0_);
  }
  asum_shown_ = false;
  slab_.ensure(slab);
  fslab_.ensure(std::max<size_t>(fslab, 1));
  fslab2_.ensure(std::max<size_t>(fslab, 1)); // odd layers' slabs: the next layer may read the previous one's
  planned_ = B;
}

// dX GEMM tile: 128-row tiles unless they leave most CUs idle (a minibatch of a few hundred rows:
// S-LBFGS's b = 256 gives 8 tiles of 128 x 128 for a 512-wide layer), then 32 x 128 (four times the
// row tiles; the epilogue needs the full K, so no split-K here).
int Mlp::dx_tile(long long B, int N) const {
  if (N >= 128 && cdiv(B, 128) * cdiv((long long)N, 128) < ctx_->cus / 2) return TILE_32x128;
  return TILE_AUTO;
}

bool Mlp::head_route() const {
  const int nl = int(layers_.size());
  if (nl < 2) return false;
  const Layer &Lo = layers_[size_t(nl - 1)], &Lh = layers_[size_t(nl - 2)];
  return head_supported(Lo.in, Lo.out) && act_in_heads(Lo.act) && act_in_heads(Lh.act);
}

bool Mlp::rowhead_on(long long B) const {
  const int nl = int(layers_.size());
  if (nl < 2 || B <= 0) return false;
  const Layer &Lo = layers_[size_t(nl - 1)], &Lh = layers_[size_t(nl - 2)];
  return Lh.fsplits > 1 && rowhead_supported(Lo.in, Lo.out) && head_route();
}

bool Mlp::gemm_head_on() const {
  const int nl = int(layers_.size());
  if (nl < 2) return false;
  const Layer &Lo = layers_[size_t(nl - 1)];
  return head_route() && layers_[size_t(nl - 2)].fsplits == 1 && Lo.in <= 128;
}

void Mlp::ensure(long long B) {
  if (B > cap_) {
    A_.clear();
    D_.clear();
    for (auto &L : layers_) {
      A_.emplace_back(size_t(std::max(1LL, B)) * L.out);
      D_.emplace_back(size_t(std::max(1LL, B)) * L.out);
    }
    cap_ = B;
  }
  plan(plan_pin_ > 0 ? plan_pin_ : B);
  const int nl = int(layers_.size());
  const Layer &Lo = layers_[nl - 1];
  size_t nloss = size_t(loss_partials_wg(std::max(1LL, B), Lo.out));
  if (head_route()) {
    const size_t hw = size_t(std::max({head_nwg(B, Lo.in), gemm_row_tiles(int(std::max(1LL, B)), layers_[nl - 2].ftile),
                                       rowhead_nwg(B)}));
    nloss = std::max(nloss, hw);
    head_slab_.ensure(hw * (size_t(Lo.in + 1) * Lo.out + (fold_ >= 0 ? size_t(fold_ + 1) * Lo.in : 0)));
  }
  loss_part_.ensure(nloss);
  long long ncg = 0;
  for (auto &L : layers_) ncg += cdiv((long long)(L.in + 1) * L.out, RA_COLS);
  dots_part_.ensure(size_t(std::max<long long>(dots_partials_wg(nparams_), ncg)) * 3);
  colpart_.ensure(size_t(ncg) * RA_MAXPART * RA_COLS);
}

// Layer l's dW slabs are reduced by side blocks of layer l-1's dW launch: the fused head's always,
// other layers' when they have many split-K slabs over few columns.
bool Mlp::side_reduced(int l, bool fused) const {
  if (l <= 0 || l >= int(layers_.size())) return false;
  if (fused && l == int(layers_.size()) - 1) return true;
  return layers_[l].splits > 2 * RA_SPLITS_PER_PART;
}

GemmDesc Mlp::fwd_desc(size_t l, const float *P, const float *in, const int *idx, long long B) const {
  const Layer &L = layers_[l];
  GemmDesc d;
  d.M = int(B);
  d.N = L.out;
  d.K = L.in;
  d.A = in;
  d.lda = L.in;
  d.a_kc = true;
  d.a_idx = (l == 0) ? idx : nullptr;
  d.B = P + L.off; // W as [In][Out] row-major (column-major Out x In)
  d.ldb = L.out;
  d.b_kc = false;
  d.C = A_[l].get();
  d.ldc = L.out;
  d.epi = EPI_FWD;
  d.bias = P + L.off + size_t(L.in) * L.out;
  d.act = L.act;
  d.abort = ctx_->abort;
  d.tile = L.ftile;
  return d;
}

// Layer l's forward GEMM as forward() launches it (split-K slabs into fslab_buf(l) when split).
GemmDesc Mlp::fwd_launch_desc(size_t l, const float *P, const float *in, const int *idx, long long B) {
  const Layer &L = layers_[l];
  GemmDesc d = fwd_desc(l, P, in, idx, B);
  if (L.fsplits > 1) {
    d.epi = EPI_STORE;
    d.C = fslab_buf(l);
    d.splits = L.fsplits;
    d.k_chunk = L.fk_chunk;
    d.slab_stride = B * L.out;
  }
  return d;
}

// d (layer l + 1's GEMM) takes its A, layer l's activations, from layer l's split-K slabs
void Mlp::set_asum(GemmDesc &d, size_t l, const float *P, long long B) {
  const Layer &L = layers_[l];
  d.a_slab = fslab_buf(l);
  d.a_splits = L.fsplits;
  d.a_slab_stride = B * L.out;
  d.a_bias = P + L.off + size_t(L.in) * L.out;
  d.a_act = L.act;
  d.a_out = A_[l].get();
}

// [dW ; db] = [in | 1]^T dZ of layer l over B rows (layer.cuh:81-84 + sum_rows_kernel kernels.cuh:144-153) with
// the layer's dW plan; rows (nullable) gathers in's rows, ones = false leaves the bias row zero. The caller
// sets the destination (C, slab_stride).
GemmDesc Mlp::dw_desc(int l, const float *in, const int *rows, bool ones, const float *dZ, long long B) const {
  const Layer &L = layers_[size_t(l)];
  GemmDesc d;
  d.M = L.in + 1;
  d.N = L.out;
  d.K = int(B);
  d.A = in;
  d.lda = L.in;
  d.a_kc = false;
  d.a_idx = rows;
  d.a_mvalid = L.in;
  d.a_ones = ones ? L.in : -1;
  d.B = dZ;
  d.ldb = L.out;
  d.b_kc = false;
  d.epi = EPI_STORE;
  d.ldc = L.out;
  d.splits = L.splits;
  d.k_chunk = L.k_chunk;
  d.abort = ctx_->abort;
  d.tile = L.dtile;
  return d;
}

// out = (dZ W^T) .* act'(A_[l - 1]) of layer l over B rows (layer.cuh:89-103 fused with activation_deriv of
// layer l-1); W is Wsrc's layer block, aux_act linear gives the plain product.
GemmDesc Mlp::dx_desc(int l, const float *dZ, const float *Wsrc, int aux_act, float *out, long long B) const {
  const Layer &L = layers_[size_t(l)];
  GemmDesc x;
  x.M = int(B);
  x.N = L.in;
  x.K = L.out;
  x.A = dZ;
  x.lda = L.out;
  x.a_kc = true;
  x.B = Wsrc + L.off; // B[n=i][k=o] = W[i][o]
  x.ldb = L.out;
  x.b_kc = true;
  x.C = out;
  x.ldc = L.in;
  x.epi = EPI_DX;
  x.aux = A_[size_t(l - 1)].get();
  x.ldaux = L.in;
  x.aux_act = aux_act;
  x.abort = ctx_->abort;
  x.tile = dx_tile(B, L.in);
  return x;
}

} // namespace lbf
