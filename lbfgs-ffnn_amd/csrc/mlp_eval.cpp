// Mlp: the first-order evaluation routes, forward and backward phase (see runtime.hpp).
#include "runtime.hpp"
#include "eval_limbs.hpp"

#include <algorithm>
#include <cstdio>
#include <string>

namespace lbf {

const float *Mlp::forward(const float *P, const float *X, const int *idx, long long B, int nrun, bool raw_last) {
  ensure(B);
  hipStream_t s = ctx_->stream;
  const float *in = X;
  const size_t nr = nrun < 0 ? layers_.size() : size_t(nrun);
  bool pending = false; // layer l - 1's slabs are reduced by layer l's GEMM (its A prologue)
  std::string asum; // LBF_SHOW_PLAN: the layers whose GEMM takes its A from slabs
  for (size_t l = 0; l < nr; ++l) {
    const Layer &L = layers_[l];
    GemmDesc d = fwd_launch_desc(l, P, in, idx, B);
    if (pending) set_asum(d, l - 1, P, B);
    if (pending && show_plan_) asum += " " + std::to_string(l);
    {
      ProfScope ps(ctx_, PK_FWD, int(l), double(B));
      gemm(s, d);
    }
    pending = false;
    if (L.fsplits > 1 && !(raw_last && l + 1 == nr)) {
      // The split-K slabs summed in split order with the bias and activation: by the next layer's GEMM while
      // it loads its A (one launch fewer; the 32 x 128 split tile of S-LBFGS minibatches), else by
      // fwd_reduce_act. (An in-launch reduction by each tile's last split measured slower: the reducer's
      // serial slab read lengthened the GEMM more than the launch it saved, profiles/r03/bench_cfg4_*_fin.json.)
      if (l + 1 < nr) {
        GemmDesc dn = fwd_launch_desc(l + 1, P, A_[l].get(), nullptr, B);
        set_asum(dn, l, P, B);
        pending = gemm_asum_ok(dn);
      }
      if (!pending)
        fwd_reduce_act(s, fslab_buf(l), L.fsplits, B * L.out, int(B), L.out, d.bias, L.act, A_[l].get(), ctx_->abort);
    }
    in = A_[l].get();
  }
  if (show_plan_ && !asum_shown_) { // once per plan, by the first forward that runs it
    std::fprintf(stderr, "[lbf plan] B=%lld forward of %zu layers: A from slabs at layers%s\n", planned_, nr,
                 asum.empty() ? " none" : asum.c_str());
    asum_shown_ = true;
  }
  return in;
}

void Mlp::out_loss(const float *Y, const int *idx, long long B, double inv_scale) {
  const size_t nl = layers_.size();
  const Layer &Lo = layers_[nl - 1];
  if (loss_ == LOSS_XENT)
    loss_xent(ctx_->stream, A_[nl - 1].get(), Lo.out, Y, Lo.out, idx, B, Lo.out, inv_scale, D_[nl - 1].get(), Lo.out,
              loss_part_.get());
  else
    loss_diff(ctx_->stream, A_[nl - 1].get(), Lo.out, Y, Lo.out, idx, B, Lo.out, Lo.act, inv_scale, D_[nl - 1].get(),
              Lo.out, loss_part_.get());
}

// Forward phase of an evaluation: every forward GEMM, the output layer (fused head or loss_diff) with
// its SSE partials, delta of the last layer the head covers, and the head's [dW ; db] partial slabs.
// What the backward phase needs is kept in fs_.
void Mlp::forward_phase(const float *P, const float *X, const float *Y, const int *idx, long long B,
                        double inv_scale) {
  hipStream_t s = ctx_->stream;
  const int nl = int(layers_.size());
  const Layer &Lo = layers_[nl - 1];
  const bool fused = head_route();
  ensure(B);
  // the output layer inside the last hidden layer's forward GEMM (EPI_HEAD), when that GEMM is one
  // unsplit tile column: its activations then never reach HBM
  const bool gemm_head = gemm_head_on();
  // the fold reads the last hidden layer's input with 16-byte loads; an unaligned caller X (2-layer
  // nets) takes the unfolded route instead
  const float *head_in = nl >= 3 ? A_[nl - 3].get() : X;
  const int fold = (gemm_head && aligned16(head_in)) ? fold_ : -1;
  const bool row_head = fused && !gemm_head && rowhead_on(B);
  forward(P, X, idx, B, fused ? (gemm_head ? nl - 2 : nl - 1) : nl, row_head);
  int nloss, lstart;
  if (row_head) {
    // last layer straight from the last hidden layer's split-K slabs: its fwd_reduce_act and the tile head
    // in one launch (head.hip rowhead)
    const Layer &Lh = layers_[nl - 2];
    RowHeadArgs r;
    r.fslab = fslab_buf(size_t(nl - 2));
    r.splits = Lh.fsplits;
    r.stride = B * Lh.out;
    r.hbias = P + Lh.off + size_t(Lh.in) * Lh.out;
    r.act_prev = Lh.act;
    r.P = P + Lo.off;
    r.H = Lo.in;
    r.Out = Lo.out;
    r.act_out = Lo.act;
    r.Y = Y;
    r.idx = idx;
    r.B = B;
    r.rpw = rowhead_rpw(B);
    r.inv_scale = inv_scale;
    r.delta = D_[nl - 2].get();
    r.slab = head_slab_.get();
    r.sse_part = loss_part_.get();
    r.abort = ctx_->abort;
    r.loss = loss_;
    nloss = rowhead_nwg(B);
    {
      ProfScope ps(ctx_, PK_LOSS);
      rowhead(s, r);
    }
    lstart = nl - 2;
  } else if (gemm_head) {
    nloss = gemm_row_tiles(int(B), layers_[nl - 2].ftile);
    GemmDesc d = fwd_desc(size_t(nl - 2), P, head_in, idx, B);
    d.epi = EPI_HEAD;
    d.C = nullptr;
    d.head_P = P + Lo.off;
    d.head_out = Lo.out;
    d.head_act = Lo.act;
    d.head_loss = loss_;
    d.head_Y = Y;
    d.head_idx = idx;
    d.head_inv_scale = inv_scale;
    d.head_delta = D_[nl - 2].get();
    d.head_slab = head_slab_.get();
    d.head_sse = loss_part_.get();
    d.head_fold = fold;
    d.head_fold_c0 = fold_c0_;
    ProfScope ps(ctx_, PK_FWD, nl - 2, double(B));
    gemm(s, d);
    lstart = nl - 2;
  } else if (fused) {
    // last layer: forward + loss + dZ + delta + [dW ; db] partials in one kernel (head.hip)
    nloss = head_nwg(B, Lo.in);
    {
      ProfScope ps(ctx_, PK_LOSS);
      head_fused(s, A_[nl - 2].get(), Lo.in, P + Lo.off, Lo.out, Y, idx, B, Lo.act, layers_[nl - 2].act, inv_scale,
                 D_[nl - 2].get(), head_slab_.get(), loss_part_.get(), ctx_->abort, loss_);
    }
    lstart = nl - 2;
  } else {
    nloss = loss_partials_wg(std::max(1LL, B), Lo.out);
    ProfScope ps(ctx_, PK_LOSS);
    out_loss(Y, idx, B, inv_scale);
    lstart = nl - 1;
  }
  fs_.B = B;
  fs_.fused = fused;
  fs_.fold = fold;
  fs_.nloss = nloss;
  fs_.lstart = lstart;
}

// Loss only (forward phase + the SSE reduction; the reference's f(x) of a line-search trial,
// full_batch_minimizer.hpp:136): SC_SSE / SC_LOSS of scal, bitwise the values a full evaluation of
// the same point writes (same partials, same reduction order). The forward state stays for
// grad_after_loss. lambda != 0: the penalty 0.5 lambda w.w from the point's w.w partials (no w.w of the trial
// point exists otherwise before the backward), which the following grad_after_loss must be given too.
void Mlp::loss_only(const float *P, const float *X, const float *Y, const int *idx, long long B, double inv_scale,
                    double *scal, double lambda, WwPart ww) {
  LBF_REQUIRE(B >= 0, "negative batch");
  LBF_REQUIRE(lambda == 0.0 || ww.part, "loss_only: a penalised loss needs the point's w.w partials");
  hipStream_t s = ctx_->stream;
  const float *hilo = nullptr;
  if (B > 0) forward_phase(P, X, Y, idx, B, inv_scale);
  if (ctx_->dp() || B == 0) {
    hilo_.ensure(4);
    if (B > 0) sse_pack(s, loss_part_.get(), fs_.nloss, hilo_.get(), ctx_->abort);
    else zero_fill(s, 2, hilo_.get(), ctx_->abort);
    if (ctx_->dp()) {
      ProfScope ps(ctx_, PK_ALLREDUCE);
      ctx_->allreduce(hilo_.get(), 2);
    }
    hilo = hilo_.get();
  }
  ProfScope ps(ctx_, PK_FINAL, 2);
  sse_loss(s, loss_part_.get(), B > 0 ? fs_.nloss : 0, hilo, inv_scale, scal, ctx_->abort, lambda, ww);
  ++loss_only_;
}

void Mlp::loss_grad(const float *P, float *G, const float *X, const float *Y, const int *idx, long long B,
                    double inv_scale, double lambda, const float *pdir, double *scal, const TailFuse *tf,
                    WwPart ww) {
  LBF_REQUIRE(B >= 0, "negative batch");
  if (B > 0) forward_phase(P, X, Y, idx, B, inv_scale);
  backward_phase(P, G, X, idx, B, inv_scale, lambda, BwdRoute{pdir, scal, tf, ww});
}

void Mlp::loss_grad_deferred(const float *P, float *G, const float *X, const float *Y, const int *idx, long long B,
                             double inv_scale, double lambda, RedAllArgs *red) {
  LBF_REQUIRE(B >= 0 && red, "loss_grad_deferred: batch / output");
  LBF_REQUIRE(!ctx_->dp(), "loss_grad_deferred: single rank (or replicated) only");
  red->nseg = 0;
  if (B > 0) forward_phase(P, X, Y, idx, B, inv_scale);
  BwdRoute r;
  r.defer = red;
  backward_phase(P, G, X, idx, B, inv_scale, lambda, r);
}

void Mlp::loss_grad_local(const float *P, float *G, const float *X, const float *Y, const int *idx, long long B,
                          double inv_scale) {
  LBF_REQUIRE(B >= 0, "negative batch");
  if (B > 0) forward_phase(P, X, Y, idx, B, inv_scale);
  BwdRoute r;
  r.local = true;
  backward_phase(P, G, X, idx, B, inv_scale, 0.0, r);
}

void Mlp::grad_after_loss(const float *P, float *G, const float *X, const int *idx, long long B, double inv_scale,
                          double lambda, const float *pdir, double *scal, const TailFuse *tf, WwPart ww) {
  LBF_REQUIRE(B == 0 || fs_.B == B, "grad_after_loss: no forward phase of this batch");
  ++gal_;
  BwdRoute r{pdir, scal, tf, ww};
  // the reduced route reports the loss of the loss-only trial's own all-reduced words, so the Armijo
  // decision and the recorded loss are one value whatever order the collective sums the two buffers in
  if (ctx_->dp() || B == 0) r.hilo_in = hilo_.get();
  backward_phase(P, G, X, idx, B, inv_scale, lambda, r);
}

// Backward phase: the dW / dX GEMMs below the head, every layer's slab reduction, the gradient
// finish (+ all-reduce, dots, status block) or the fused optimizer tail.
void Mlp::backward_phase(const float *P, float *G, const float *X, const int *idx, long long B, double inv_scale,
                         double lambda, const BwdRoute &route) {
  hipStream_t s = ctx_->stream;
  const int nl = int(layers_.size());
  BwdPass b{P, X, idx, B, inv_scale, lambda, route}; // the steps below read b alone
  if (lambda == 0.0) b.r.ww = {}; // no penalty: the lambda = 0 kernels
  b.empty = B == 0; // a data-parallel rank whose share of a small batch is empty
  b.reduced = ctx_->dp() || b.empty || b.r.local;
  b.fused = fs_.fused;
  b.fold = b.empty ? -1 : fs_.fold;
  b.nloss = b.empty ? 0 : fs_.nloss;
  b.lstart = b.empty ? -1 : fs_.lstart;
  b.nfold = b.fold >= 0 ? (long long)(b.fold + 1) * layers_[nl - 1].in : 0; // fold rows in the head slab
  // Where this rank's gradient lands before the collective: G itself on a single rank and for a packed
  // local evaluation (its caller reduces the block), else the private words buffer. The collective of a
  // speculative iteration that was aborted still runs (RCCL cannot skip it; every rank aborts alike), and
  // G of a queued iteration can be the buffer of the live gradient: only abort-aware kernels (the tail,
  // finalize) may write G from the reduced words.
  b.G = G;
  b.Gl = G;
  if (b.reduced && !b.r.local) {
    words_.ensure(size_t(cdiv((long long)nparams_ + 2, 4) * 4));
    b.Gl = words_.get();
  }
  if (b.empty) zero_fill(s, (long long)nparams_ + 2, b.Gl, ctx_->abort);
  EarlyLs early;
  bwd_launch(b, bwd_early(b, &early) ? &early : nullptr);
  RedAllArgs ra;
  bwd_segments(b, ra);
  ++evals_;
  rows_ += B;
  bool one_pass = true; // no segment needs the multi-part reduction
  for (int l = 0; l < nl; ++l) one_pass = one_pass && ra.seg[l].parts == 1;
  if (b.r.tf && !b.r.local && one_pass) {
    bwd_tail(b, ra);
  } else if (b.reduced) {
    bwd_finish_reduced(b, ra);
  } else if (b.r.defer && !ra.dots && one_pass) {
    *b.r.defer = ra; // the consumer finishes the gradient from the slabs (Mlp::loss_grad_deferred)
  } else {
    ProfScope ps(ctx_, PK_SLAB, 0);
    reduce_all(s, ra);
  }
}

// A speculative first trial (tf->early, set by the solver: single rank, Switches::early; lambda != 0 with the
// point's w.w partials) takes its Armijo test in the first backward launch (EarlyLs, gemm.hip gemm_early_exit):
// on a failure that launch, the rest of the backward and the tail exit at entry, and the host finishes the
// search as after the tail's own rejection. Returns whether the request applies (*e filled).
bool Mlp::bwd_early(const BwdPass &b, EarlyLs *e) const {
  const TailFuse *tf = b.r.tf;
  if (!(tf && tf->early && !b.reduced && (b.lambda == 0.0 || b.r.ww.part) && b.nloss > 0)) return false;
  e->sse_part = loss_part_.get();
  e->nsse = b.nloss;
  e->inv_scale = b.inv_scale;
  e->ww_part = b.r.ww.part;
  e->nww = b.r.ww.n;
  e->lambda = b.lambda;
  e->ls = tf->ls;
  return true;
}

// Layer l's dW GEMM in a backward phase: without the folded rows, with the side blocks that finish layer
// l+1's slabs, into its slabs or straight into the gradient.
GemmDesc Mlp::bwd_dw_desc(const BwdPass &b, int l) const {
  const int nl = int(layers_.size());
  const Layer &L = layers_[l];
  GemmDesc d = dw_desc(l, l == 0 ? b.X : A_[l - 1].get(), l == 0 ? b.idx : nullptr, true, D_[l].get(), b.B);
  if (b.fold >= 0 && l == nl - 2) { // rows >= fold_c0_ come from the EPI_HEAD epilogue
    d.M = fold_c0_;
    d.a_mvalid = fold_c0_;
    d.a_ones = -1;
  }
  if (l + 1 < nl && side_reduced(l + 1, b.fused)) {
    // finish layer l+1's [dW ; db] slabs (the fused head's, or many split-K slabs) in side blocks
    // of this launch, while its GEMM runs; the head's slab starts with this layer's folded rows
    const Layer &N1 = layers_[l + 1];
    const bool head = b.fused && l + 1 == nl - 1;
    // the segment exactly as layer l+1's launch wrote its slabs: a folded layer's GEMM has fold_c0_
    // rows (its remaining rows live in the head's segment)
    const long long n1rows = (b.fold >= 0 && l + 1 == nl - 2) ? fold_c0_ : N1.in + 1;
    const long long nseg = head ? (long long)(N1.in + 1) * N1.out + b.nfold : n1rows * N1.out;
    d.side_slab = head ? head_slab_.get() : slab_.get() + N1.slab_off;
    d.side_splits = head ? b.nloss : N1.splits;
    d.side_stride = nseg;
    d.side_count = nseg;
    d.side_dst = b.Gl + N1.off - (head ? b.nfold : 0);
  }
  if (L.splits > 1) {
    d.C = slab_.get() + L.slab_off;
    d.slab_stride = (long long)d.M * L.out;
  } else {
    d.C = b.Gl + L.off;
  }
  return d;
}

// The dW / dX launches from layer lstart down; the early test rides on the first launch only.
void Mlp::bwd_launch(const BwdPass &b, const EarlyLs *early) {
  hipStream_t s = ctx_->stream;
  auto first_launch = [&](GemmDesc d) {
    d.early = early;
    early = nullptr;
    return d;
  };
  auto dx = [&](int l) { return dx_desc(l, D_[l].get(), b.P, layers_[l - 1].act, D_[l - 1].get(), b.B); };
  for (int l = b.lstart; l >= 0; --l) {
    if (l == 1 && group_dw_ && !side_reduced(1, b.fused)) {
      // the last two dW GEMMs in one launch (S-LBFGS minibatches: two small split-K grids that each
      // leave most of the chip idle at its tail): dX of layer 1 first, since dW of layer 0 reads it
      const GemmDesc d1 = bwd_dw_desc(b, 1), d0 = bwd_dw_desc(b, 0);
      if (gemm_group_ok(d1, d0)) {
        {
          ProfScope ps(ctx_, PK_DX, 1, double(b.B));
          gemm(s, first_launch(dx(1)));
        }
        ProfScope ps(ctx_, PK_DW, 1, double(b.B));
        gemm_group(s, first_launch(d1), d0);
        break;
      }
    }
    {
      ProfScope ps(ctx_, PK_DW, l, double(b.B));
      gemm(s, first_launch(bwd_dw_desc(b, l)));
    }
    if (l > 0) {
      ProfScope ps(ctx_, PK_DX, l, double(b.B));
      gemm(s, first_launch(dx(l)));
    }
  }
}

// every layer's partial slabs -> gradient (+ dots and the status block on a single rank)
void Mlp::bwd_segments(const BwdPass &b, RedAllArgs &ra) const {
  const int nl = int(layers_.size());
  ra.G = b.Gl;
  ra.w = b.P;
  ra.p = b.r.pdir;
  ra.lambda = b.lambda;
  // scal == nullptr (S-LBFGS minibatch / Hessian-batch gradients, whose status nobody reads): the
  // gradient only, no dot partials and no finishing launch. The reduced route (data parallel, an empty
  // share, or a packed local evaluation) finishes the gradient from [G | hi | lo] after the all-reduce.
  ra.dots = (b.reduced || !b.r.scal) ? 0 : 1;
  ra.l2 = b.reduced ? 0 : 1;
  ra.partials = dots_part_.get();
  ra.colpart = colpart_.get();
  ra.sse_part = loss_part_.get();
  ra.nsse = b.nloss;
  ra.inv_scale = b.inv_scale;
  ra.scal = b.r.scal;
  ra.abort = ctx_->abort;
  ra.ww_part = b.r.ww.part;
  ra.nww = b.r.ww.n;
  for (int l = 0; l < nl; ++l) {
    const Layer &L = layers_[l];
    RedSeg &g = ra.seg[l];
    g.count = (long long)(L.in + 1) * L.out;
    g.goff = (long long)L.off;
    if (b.fold >= 0 && l == nl - 2) g.count = (long long)fold_c0_ * L.out; // the rest is the head's segment
    if (b.fold >= 0 && l == nl - 1) {
      g.count += b.nfold;
      g.goff -= b.nfold;
    }
    g.stride = g.count;
    if (b.empty || side_reduced(l, b.fused)) {
      // zero-filled (an empty share) / finished by the side blocks of the next dW launch: as written
    } else if (L.splits > 1) {
      g.slab = slab_.get() + L.slab_off;
      g.splits = L.splits;
    }
    const int ncols = int(cdiv(g.count, RA_COLS));
    // many slabs over few columns (the head's): split ranges over blocks, finished by one block
    if (g.splits > 2 * RA_SPLITS_PER_PART && ra.nfin + ncols <= RA_MAXFIN)
      g.parts = int(std::min<long long>(RA_MAXPART, cdiv(g.splits, RA_SPLITS_PER_PART)));
    g.wg0 = ra.nwg;
    g.cg0 = ra.ncg;
    if (g.parts > 1) {
      g.fin0 = ra.nfin;
      ra.nfin += ncols;
    }
    // few splits: RA_GPB groups per block (a block's loads are few, blocks the cost); many: one group per
    // block, so the splits' loads spread over four times the blocks (the 20-slab shard gradient)
    g.gpb = g.parts == 1 && g.splits <= 8 ? RA_GPB : 1;
    ra.nwg += g.parts > 1 ? ncols * g.parts : int(cdiv(ncols, g.gpb));
    ra.ncg += ncols;
  }
  ra.nseg = nl;
}

// this rank's gradient (no lambda w) and its SSE as an fp32 (hi, lo) pair, [G | hi | lo], then one all-reduce
// of those words, unless the caller reduces the block itself (local)
void Mlp::bwd_words(const BwdPass &b, const RedAllArgs &ra) {
  if (!b.empty) { // an empty share's words were zero-filled at entry
    RedAllArgs loc = ra;
    loc.dots = 0;
    loc.sse_part = loss_part_.get(); // the SSE words in an extra block of the same launch
    loc.nsse = b.nloss;
    loc.sse_hilo = b.Gl + nparams_;
    ProfScope ps(ctx_, PK_SLAB, 0);
    reduce_all(ctx_->stream, loc);
  }
  if (ctx_->dp() && !b.r.local) {
    ProfScope ps(ctx_, PK_ALLREDUCE);
    ctx_->allreduce(b.Gl, nparams_ + 2);
  }
}

// fused optimizer tail (tail.hip); data parallel: local reduce -> all-reduce -> tail over G
void Mlp::bwd_tail(const BwdPass &b, RedAllArgs &ra) {
  hipStream_t s = ctx_->stream;
  const TailFuse *tf = b.r.tf;
  const int nl = int(layers_.size());
  TailArgs ta;
  const float *hilo = nullptr;
  if (b.reduced) {
    bwd_words(b, ra);
    hilo = b.r.hilo_in ? b.r.hilo_in : b.Gl + nparams_;
    for (int l = 0; l < nl; ++l) {
      ra.seg[l].slab = nullptr;
      ra.seg[l].splits = 0;
    }
  }
  ta.ra = ra;
  ta.ra.G = b.G;
  ta.g_src = b.Gl != b.G ? b.Gl : nullptr;
  ta.hilo = hilo;
  ta.h = tf->h;
  ta.h.abort = ctx_->abort;
  ta.has_pair = tf->has_pair;
  ta.x_prev = tf->x_prev;
  ta.g_prev = tf->g_prev;
  ta.policy = tf->policy;
  ta.iter_next = tf->iter_next;
  ta.ls = tf->ls;
  ta.nc = 6 * tf->h.m + 8;
  ta.nb = 0; // one TAIL_COLS column group per block: latency-bound work wants every CU busy
  for (int l = 0; l < nl; ++l) {
    ta.tcg0[l] = ta.nb;
    ta.nb += int(cdiv(ra.seg[l].count, (long long)TAIL_COLS));
  }
  trows_.ensure(size_t(ta.nb) * ta.nc);
  tdots_.ensure(size_t(ta.nc));
  ta.rows = trows_.get();
  ta.dots = tdots_.get();
  if (!cols_done_.get()) {
    cols_done_.resize(1);
    LBF_HIP(hipMemsetAsync(cols_done_.get(), 0, sizeof(unsigned), s));
  }
  ta.cols_done = cols_done_.get();
  ProfScope ps(ctx_, PK_GRAM, 1);
  tail_reduce(s, ta); // + the fin in the last tail_cols block (cols_done)
}

// The reduced route without the tail: the all-reduced [G | hi | lo], then finish_reduced.
void Mlp::bwd_finish_reduced(const BwdPass &b, const RedAllArgs &ra) {
  bwd_words(b, ra);
  if (b.r.local) return; // the caller all-reduces [G | hi | lo] (with other blocks) and calls finish_reduced
  finish_reduced(b.P, b.G, b.inv_scale, b.lambda, b.r.pdir, b.r.scal, b.r.hilo_in, b.Gl != b.G ? b.Gl : nullptr,
                 b.r.ww);
}

void Mlp::batch_grads(const float *P, const float *X, const float *Y, int nmb, long long cnt, double inv_scale,
                      double lambda, float *G, long long ldg, bool local) {
  LBF_REQUIRE(nmb > 0 && cnt > 0 && cnt % 32 == 0, "batch_grads: minibatches of a multiple of 32 rows");
  LBF_REQUIRE(ldg >= (long long)nparams_, "batch_grads: gradient stride below the parameter count");
  hipStream_t s = ctx_->stream;
  const int nl = int(layers_.size());
  const long long R = (long long)nmb * cnt;
  ensure(R);
  // forward over every row (no fused head: its [dW ; db] partials are per 64-row tile, not per minibatch)
  forward(P, X, nullptr, R, nl);
  {
    ProfScope ps(ctx_, PK_LOSS);
    out_loss(Y, nullptr, R, inv_scale);
  }
  for (int l = nl - 1; l >= 0; --l) {
    const Layer &L = layers_[l];
    // [dW ; db] of minibatch t = split t of [A_in | 1]^T dZ
    GemmDesc d = dw_desc(l, l == 0 ? X : A_[l - 1].get(), nullptr, true, D_[l].get(), R);
    d.splits = nmb;
    d.k_chunk = int(cnt);
    d.C = G + L.off;
    d.slab_stride = ldg;
    d.tile = TILE_64x64;
    {
      ProfScope ps(ctx_, PK_DW, l, double(R));
      gemm(s, d);
    }
    if (l > 0) {
      ProfScope ps(ctx_, PK_DX, l, double(R));
      gemm(s, dx_desc(l, D_[l].get(), P, layers_[l - 1].act, D_[l - 1].get(), R));
    }
  }
  if (!local) {
    ProfScope ps(ctx_, PK_FINAL, 0);
    add_l2_rows(s, (long long)nparams_, nmb, ldg, G, P, lambda);
  }
  evals_ += nmb;
  rows_ += R;
}

// The gradient and status of an all-reduced [G | hi | lo] block: G += lambda w, the dots of the status
// block, and the loss from the (hi, lo) words (or from hilo_in: a loss-only trial's reduced words).
void Mlp::finish_reduced(const float *P, float *G, double inv_scale, double lambda, const float *pdir, double *scal,
                         const float *hilo_in, const float *g_src, WwPart ww) {
  hipStream_t s = ctx_->stream;
  ProfScope ps(ctx_, PK_FINAL, 1);
  const int nd = dots_partials_wg(nparams_);
  dots_part_.ensure(size_t(nd) * 3);
  finalize_grad_dots(s, nparams_, G, P, lambda, pdir, dots_part_.get(), ctx_->abort, g_src);
  if (scal)
    eval_tail(s, dots_part_.get(), nd, loss_part_.get(), 0, hilo_in ? hilo_in : (g_src ? g_src : G) + nparams_,
              inv_scale, lambda, scal, ctx_->abort, ww);
}

Mlp::EvalTotals Mlp::evaluate(const float *P, const float *X, const float *Y, const int *idx, long long B, int k,
                              long long chunk_rows, long long *h_conf, int *d_pred, float *d_proba) {
  const Layer &Lo = layers_.back();
  const int Out = Lo.out, In = layers_.front().in;
  LBF_REQUIRE(B >= 0 && chunk_rows >= 0, "evaluate: negative batch or chunk");
  LBF_REQUIRE(P && (B == 0 || X), "evaluate: null argument");
  LBF_REQUIRE(k >= 1 && k <= Out, "evaluate: k outside 1..Out");
  LBF_REQUIRE(!h_conf || Y || B == 0, "evaluate: a confusion matrix needs targets");
  LBF_REQUIRE(!d_proba || loss_ == LOSS_XENT, "evaluate: probabilities need the softmax cross-entropy loss");
  LBF_REQUIRE(!ctx_->dp() || ctx_->nranks <= kEvalMaxRanks, "evaluate: at most 256 ranks");
  LBF_REQUIRE(B <= kEvalMaxCount, "evaluate: batch too large");
  hipStream_t s = ctx_->stream;
  const long long chunk = std::max(1LL, std::min(chunk_rows > 0 ? chunk_rows : 65536LL, std::max(1LL, B)));
  const long long nchunks = cdiv(B, chunk);
  const int ncounts = 3 + (h_conf ? Out * Out : 0);
  const size_t nwords = 2 + size_t(kEvalLimbs) * size_t(ncounts);
  const size_t part_cap = size_t(std::max(1LL, nchunks)) * size_t(metrics_nwg(chunk, Out));
  const int nconf = h_conf ? Out * Out : 0;
  ev_part_.ensure(part_cap);
  ev_cpart_.ensure(3 * part_cap);
  ev_cnt_.ensure(size_t(std::max(1, nconf)));
  ev_words_.ensure(nwords);
  ev_sum_.ensure(1);
  ev_hwords_.ensure(nwords);
  ev_hsum_.ensure(1);
  if (nconf) LBF_HIP(hipMemsetAsync(ev_cnt_.get(), 0, size_t(nconf) * sizeof(unsigned long long), s));
  int npart = 0;
  {
    // every chunk under the whole batch's forward plan: the outputs do not depend on the chunking
    struct Pin {
      long long &p;
      ~Pin() { p = -1; }
    } pin{plan_pin_};
    plan_pin_ = B;
    for (long long r0 = 0; r0 < B; r0 += chunk) {
      const long long b = std::min(chunk, B - r0);
      const float *Z = forward(P, idx ? X : X + r0 * In, idx ? idx + r0 : nullptr, b);
      MetricsArgs a;
      a.Z = Z;
      a.Y = Y ? (idx ? Y : Y + r0 * Out) : nullptr;
      a.idx = idx ? idx + r0 : nullptr;
      a.B = b;
      a.Out = Out;
      a.loss = loss_;
      a.k = k;
      a.conf_mode = metrics_conf_mode(Out, h_conf != nullptr);
      a.partials = ev_part_.get() + npart;
      a.cpart = ev_cpart_.get() + 3 * size_t(npart);
      a.conf = h_conf ? ev_cnt_.get() : nullptr;
      a.pred = d_pred ? d_pred + r0 : nullptr;
      a.proba = d_proba ? d_proba + r0 * Out : nullptr;
      {
        ProfScope ps(ctx_, PK_METRICS, 0, double(b));
        metrics(s, a);
      }
      npart += metrics_nwg(b, Out);
    }
  }
  metrics_finish(s, ev_part_.get(), ev_cpart_.get(), npart, ev_cnt_.get(), nconf, ev_sum_.get(), ev_words_.get());
  if (ctx_->dp()) ctx_->allreduce(ev_words_.get(), nwords);
  LBF_HIP(hipMemcpyAsync(ev_hwords_.get(), ev_words_.get(), nwords * sizeof(float), hipMemcpyDeviceToHost, s));
  LBF_HIP(hipMemcpyAsync(ev_hsum_.get(), ev_sum_.get(), sizeof(double), hipMemcpyDeviceToHost, s));
  LBF_HIP(hipStreamSynchronize(s));
  const float *w = ev_hwords_.get();
  EvalTotals r;
  // a single rank keeps the fp64 sum; across ranks the loss is what the (hi, lo) words carried
  r.sse = ctx_->dp() ? double(w[0]) + double(w[1]) : ev_hsum_[0];
  r.rows = eval_limbs_merge(w + 2);
  r.correct = eval_limbs_merge(w + 2 + kEvalLimbs);
  r.topk = eval_limbs_merge(w + 2 + 2 * kEvalLimbs);
  if (h_conf)
    for (int c = 0; c < Out * Out; ++c) h_conf[c] = eval_limbs_merge(w + 2 + kEvalLimbs * (3 + c));
  return r;
}

} // namespace lbf
