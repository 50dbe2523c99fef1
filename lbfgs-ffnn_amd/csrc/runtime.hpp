// Host runtime of liblbfgs_amd_abi3.so: context (device, stream, RCCL communicator) and profiler (ctx.cpp), the
// MLP's plan and layer GEMMs (mlp_plan.cpp), its evaluation routes (mlp_eval.cpp) and curvature products
// (mlp_curvature.cpp), and the device-resident L-BFGS history (history.cpp). The solver drivers: solvers.hpp.
#pragma once

#include "internal.hpp"
#include "comm.hpp"
#include "kernels.hpp"

#include <memory>
#include <vector>

namespace lbf {

// Per-kernel-class timing with HIP events on the launch stream (enabled by the benchmark only).
enum ProfKind : int { PK_FWD = 0, PK_DW = 1, PK_DX = 2, PK_LOSS = 3, PK_SLAB = 4, PK_FINAL = 5, PK_GRAM = 6,
                      PK_COEF = 7, PK_COMBINE = 8, PK_AXPY = 9, PK_ALLREDUCE = 10, PK_METRICS = 11,
                      PK_OWL_PSEUDO = 12, PK_OWL_TRIAL = 13 };
struct ProfRec { int id; size_t a, b; double work; };
struct Profiler {
  bool on = false;
  int only = -1; // section filter (-1: all)
  int every = 1;  // sample every k-th launch of a wanted section
  long long seen = 0;
  bool want(int id) {
    if (!on || (only >= 0 && only != id)) return false;
    return every <= 1 || (seen++ % every) == 0;
  }
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  using Rec = ProfRec;
  std::vector<Rec> recs;
  std::vector<double> ms;      // by section id
  std::vector<long long> cnt;  // by section id
  std::vector<double> work;    // by section id: the caller's work units of the timed launches (GEMMs: rows)
  ~Profiler();
  size_t mark(hipStream_t s);
  void resolve();
  void merge_into(Profiler &dst); // resolve this one and add its totals to dst's
  void add(const Rec &r, float t);
};

struct Ctx {
  int device = 0;
  int cus = 256; // compute units (workgroup slots = 2 per CU for the GEMM tiles, see Mlp::plan)
  Profiler prof;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::unique_ptr<Comm> comm; // RCCL (lbf_comm_init) or an in-process rank group (lbf_comm_init_local)
  int rank = 0, nranks = 1;
  const int *abort = nullptr; // set by a solver while it runs speculatively (see LbfgsSolver)
  // evaluate as a single rank although a communicator exists (replicated S-LBFGS inner steps, LocalOnly)
  bool local_only = false;
  // scratch for the BLAS-1 ABI helpers
  DevBuf<double> part, red;
  PinnedBuf<double> host;
  ~Ctx();
  void set_device() const;
  // data-parallel evaluation path: taken whenever a communicator exists, including a 1-rank one
  // (lbf_comm_init(ctx, 1, 0, id)), which is how the RCCL path is exercised on a single GPU
  bool dp() const { return comm != nullptr && !local_only; }
  void allreduce(float *buf, size_t count);
};

// Scoped Ctx::local_only (when `on`).
struct LocalOnly {
  Ctx *c;
  bool prev;
  LocalOnly(Ctx *ctx, bool on) : c(ctx), prev(ctx->local_only) {
    if (on) c->local_only = true;
  }
  ~LocalOnly() { c->local_only = prev; }
};

// Fused optimizer tail request (speculative L-BFGS fast path, tail.hip): the pair inputs, the
// history and the line-search decision taken after the evaluation.
struct TailFuse {
  HistView h;
  int has_pair = 0;
  const float *x_prev = nullptr, *g_prev = nullptr;
  int policy = POL_CPU;
  int iter_next = 1;
  LsCtlArgs ls;
  int early = 0; // a speculative first trial: its Armijo test in the first backward launch (EarlyLs)
};

struct Layer {
  int in, out, act;
  size_t off;      // flat offset of the [(in+1) x out] segment
  int splits = 1;  // split-K factor of the dW GEMM at the planned batch
  int k_chunk = 0;
  size_t slab_off = 0; // this layer's partial slabs inside the shared slab buffer
  int fsplits = 1;     // split-K factor of the forward GEMM (few row tiles: small per-rank batches)
  int fk_chunk = 0;
  int ftile = 0;       // forward GEMM tile (GemmTile)
  int dtile = 0;       // dW GEMM tile (GemmTile)
};

// RAII section: records an event pair around the enclosed launches when profiling is on.
struct ProfScope {
  Ctx *c;
  int id;
  size_t a = 0;
  bool on;
  double work;
  ProfScope(Ctx *ctx, int kind, int layer = 0, double w = 0.0)
      : c(ctx), id(kind * 16 + layer), on(ctx->prof.want(id)), work(w) {
    if (on) a = c->prof.mark(c->stream);
  }
  ~ProfScope() {
    if (on) c->prof.recs.push_back({id, a, c->prof.mark(c->stream), work});
  }
};

// Dense MLP (the reference's CudaNetwork, src/cuda/network.cuh:21-158) with a cached workspace.
class Mlp {
public:
  Mlp(Ctx *ctx, int nl, const int *dims, const int *acts, const Switches &sw);
  size_t nparams() const { return nparams_; }
  const std::vector<Layer> &layers() const { return layers_; }
  Ctx *ctx() const { return ctx_; }
  // The loss every evaluation below minimises (kernels.hpp Loss); LOSS_XENT needs a linear last layer with
  // at least two outputs. Takes effect from the next evaluation; the workspace and the plan do not depend on it.
  void set_loss(int loss);
  int loss() const { return loss_; }
  // L2 weight decay of the solvers that take no lambda of their own (full-batch L-BFGS, GD, SGD): they minimise
  // data loss + 0.5 l2 |w|^2. A property of the network like the loss; read when a solve begins. The evaluations
  // below take their lambda as an argument and do not read it.
  void set_l2(double l2);
  double l2() const { return l2_; }

  // Forward only: activations of every layer into the workspace; returns the output buffer.
  // raw_last: the last layer run stays as its split-K slabs in fslab_buf(l) (no fwd_reduce_act; rowhead reads them)
  const float *forward(const float *P, const float *X, const int *idx, long long B, int nrun = -1,
                       bool raw_last = false);
  // Fused loss + gradient (+ all-reduce over the communicator) + line-search dots.
  //   G    : gradient output, must hold nparams()+2 floats (two extra words carry the loss for the
  //          all-reduce).
  //   pdir : optional direction for the g.p dot.
  //   scal : device fp64 status block (SC_LOSS, SC_TGG, SC_TGP, SC_WW, SC_SSE written).
  void loss_grad(const float *P, float *G, const float *X, const float *Y, const int *idx, long long B,
                 double inv_scale, double lambda, const float *pdir, double *scal, const TailFuse *tf = nullptr,
                 WwPart ww = {});
  // loss_grad without the last launch (a single rank's gradient only: scal == nullptr): the split-K slabs
  // are left for the consumer, which finishes each gradient value with reduce_all's arithmetic (the S-LBFGS
  // direction sweep, dir.hip). *red describes the slabs; red->nseg == 0 when a segment needs the multi-part
  // reduction (then G is complete as with loss_grad). When red->nseg > 0, G is left INCOMPLETE: the split
  // segments of G keep whatever they held (the consumer forms those values in registers and does not store
  // them back; the S-LBFGS sweep writes only v = g - gb + mu). No reader of G exists on that route.
  void loss_grad_deferred(const float *P, float *G, const float *X, const float *Y, const int *idx, long long B,
                          double inv_scale, double lambda, RedAllArgs *red);
  // The same evaluation in two steps (a line-search trial needs f first and the gradient only once
  // Armijo holds, full_batch_minimizer.hpp:136-146): loss_only runs the forward phase and writes
  // SC_SSE / SC_LOSS; grad_after_loss then runs the backward phase of that same forward state. loss_only
  // followed by grad_after_loss == loss_grad, bit for bit. ww: the w.w partials of P (kernels.hpp WwPart), from
  // which every evaluation of P takes SC_WW and the penalty when lambda != 0 (loss_only requires them then: it
  // has no sweep over P of its own); without them a full evaluation uses its own sweep's w.w.
  void loss_only(const float *P, const float *X, const float *Y, const int *idx, long long B, double inv_scale,
                 double *scal, double lambda = 0.0, WwPart ww = {});
  void grad_after_loss(const float *P, float *G, const float *X, const int *idx, long long B, double inv_scale,
                       double lambda, const float *pdir, double *scal, const TailFuse *tf = nullptr, WwPart ww = {});
  // Packed data-parallel evaluation in two halves: loss_grad_local stops before the all-reduce, leaving
  // this rank's gradient (no lambda w) and its SSE as fp32 (hi, lo) words in G[0 .. n+2); the caller
  // all-reduces one or more such blocks in a single collective and then finishes each with
  // finish_reduced (+ lambda w, status block). Together bitwise equal to loss_grad on the same rank.
  void loss_grad_local(const float *P, float *G, const float *X, const float *Y, const int *idx, long long B,
                       double inv_scale);
  // g_src (nullable): the reduced words are there and the finished gradient is written to G
  void finish_reduced(const float *P, float *G, double inv_scale, double lambda, const float *pdir, double *scal,
                      const float *hilo_in = nullptr, const float *g_src = nullptr, WwPart ww = {});
  // Per-minibatch gradients at one point P (S-LBFGS's anchor gradients: w is fixed for an epoch): rows
  // [t cnt, (t+1) cnt) of the gathered X / Y are minibatch t (t < nmb); its gradient, scaled by inv_scale,
  // goes to G + t ldg (+ lambda P unless local: a data-parallel rank's partial sums). One evaluation over
  // the nmb cnt rows (full-batch GEMM tiles), whose dW GEMMs split K exactly at the minibatch boundaries
  // and write split t in place as minibatch t's [dW ; db]: no slab reduction. cnt % 32 == 0.
  void batch_grads(const float *P, const float *X, const float *Y, int nmb, long long cnt, double inv_scale,
                   double lambda, float *G, long long ldg, bool local);
  long long loss_only_evals() const { return loss_only_; }
  long long grad_after_loss_evals() const { return gal_; } // backward phases run after a loss_only
  // Exact Hessian-vector product Hv = H(P) V of the same batch loss (+ lambda V), Pearlmutter's
  // R-operator (hvp.hip); with a communicator the shards' products are all-reduced. Hv: nparams().
  void hvp(const float *P, const float *V, const float *X, const float *Y, const int *idx, long long B,
           double inv_scale, double lambda, float *Hv);
  // Gauss-Newton vector product Gv = J^T H_L J V (+ lambda V) of the same batch loss (hvp.hip): positive
  // semi-definite, no second-order terms. The loss is split from the network at the outputs A_L for the squared
  // error (H_L = inv_scale I) and at the logits for the cross-entropy. Arguments, empty batch and all-reduce as
  // hvp; it shares hvp's workspace, and the two may be called in any order with any batch sizes.
  void gnvp(const float *P, const float *V, const float *X, const float *Y, const int *idx, long long B,
            double inv_scale, double lambda, float *Gv);
  // Conjugate gradients on (G(P) + damping I) x = bscale b, G the Gauss-Newton matrix of gnvp on the given batch
  // (cg.hip), from x = 0. The forward pass runs once (gn_prepare); an iteration is gn_apply on the
  // direction and three sweeps. The host enqueues `check` iterations, reads the status block and goes on while the
  // solve is running; the solver's abort word, which ctx->abort points at meanwhile, freezes what was enqueued
  // past the stopping iteration. x: nparams() floats, any 4-byte aligned pointer. Synchronous.
  struct CgInfo {
    int iterations = 0, status = 0; // CG_CONVERGED / CG_MAXITER / CG_BREAKDOWN
    double rr0 = 0.0, rr = 0.0, xb = 0.0, xr = 0.0, xx = 0.0; // xb = x.(bscale b)
  };
  // minv (nullable; nparams() floats, entries > 0, any 4-byte aligned pointer): preconditioned CG with the diagonal
  // inverse preconditioner minv (kernels.hpp CgArgs): two more reads of n floats per iteration, no extra launch.
  void gn_cg(const float *P, const float *b, float bscale, const float *X, const float *Y, const int *idx,
             long long B, double inv_scale, double damping, int max_iters, double rtol, int check, float *x,
             CgInfo *info, const float *minv = nullptr);
  // out[i] = scale * sum_b (d l_b / d w_i)^2 over the batch rows, l_b row b's data loss at inv_scale = 1
  // (0.5 |a_b - y_b|^2, or sum_o y_bo (lse_b - z_bo)); flat parameter layout, no l2 term: the diagonal of the
  // empirical Fisher matrix (fisher.hip). gn_prepare's unfused forward, out_loss at inv_scale = 1,
  // then per layer from the top the squared product on (A_{l-1}, D_l) and the EPI_DX GEMM to D_{l-1}; scale is
  // applied where the row chunks' slabs are summed. With a communicator every rank sums its rows, scales, and the
  // scaled vectors are all-reduced once; B == 0 contributes zeros and joins. Overwrites the activation workspace
  // like forward(). Bitwise reproducible.
  void grad_sq(const float *P, const float *X, const float *Y, const int *idx, long long B, double scale, float *out);
  const float *cg_residual() const { return cg_r_.get(); } // r of the last gn_cg (null before the first)
  // `steps` steps of Lanczos on A = H(P) + l2 I (exact) or G(P) + l2 I from q_0 = v0 / |v0| (lanczos.hip; DESIGN
  // §23): the tridiagonal's alpha and beta into h_alpha / h_beta (steps doubles each, zeros from info->steps on).
  // G: one gn_prepare, then gn_apply per step; H: hvp per step. reorth: every step orthogonalises twice against
  // all earlier rows (steps + 1 rows are kept: in basis when given, else in a workspace); otherwise once against
  // q_{j-1} and q_j, three rows in a ring, and basis is only written. The host enqueues `check` steps per status
  // read; what is enqueued behind a stop is frozen by the run's abort word. Synchronous.
  struct LanczosInfo {
    int steps = 0, status = 0; // LZ_DONE / LZ_EXHAUSTED / LZ_FAILED
    double v0_norm = 0.0;
  };
  void lanczos(const float *P, const float *v0, const float *X, const float *Y, const int *idx, long long B,
               double inv_scale, double l2, bool exact, int steps, bool reorth, int check, double breakdown_rtol,
               double *h_alpha, double *h_beta, float *basis, long long ld, LanczosInfo *info);
  // Device-side evaluation (metrics.hip; replaces the host scan of unified_launcher.hpp:154-199): forward() and
  // the metrics kernel per chunk of chunk_rows rows (0: 65536, or the batch if smaller), so the activation
  // workspace is bounded by the chunk. Every chunk runs the forward plan of the whole batch, so the outputs, and
  // with them every count, do not depend on the chunking. The chunks' loss partials fill one table in row order,
  // summed once at the end; counts accumulate on the device; one read-back and one synchronisation per call.
  // With a communicator each rank passes its B local rows (B == 0: an empty share) and one float all-reduce
  // carries the loss as (hi, lo) words and every count as three 16-bit limbs (eval_limbs.hpp: exact up to 256
  // ranks and counts below 2^48); d_pred / d_proba stay local. Y null: predictions only (sse = correct = topk = 0).
  // h_conf (nullable, needs Y): Out x Out counts [tgt][pred]. All buffers are this Mlp's own: nothing a solver on
  // another Mlp of the context reads is touched (not the context's status block, its gradient scratch or any
  // history). Intended use during a stateful solve: a second Mlp of the same shape (parameters are external to
  // the net, so that costs only workspace); on the solver's own Mlp it overwrites the activations like forward().
  struct EvalTotals {
    double sse = 0.0; // sum of the loss partials: data loss = 0.5 * inv_scale * sse
    long long rows = 0, correct = 0, topk = 0;
  };
  EvalTotals evaluate(const float *P, const float *X, const float *Y, const int *idx, long long B, int k,
                      long long chunk_rows, long long *h_conf, int *d_pred, float *d_proba);
  long long evals() const { return evals_; }
  long long rows() const { return rows_; } // batch rows evaluated (sum of B over loss_grad calls)
  void discard_evals(long long k, long long B) { // speculative evaluations (B rows each) that were aborted
    evals_ -= k;
    rows_ -= k * B;
  }
  void backward_skipped() { // a trial rejected by EarlyLs ran its forward only: a loss-only trial
    --evals_;
    ++loss_only_;
  }

private:
  // ---- layers and plan state (mlp_plan.cpp) ----
  Ctx *ctx_;
  std::vector<Layer> layers_;
  size_t nparams_ = 0;
  int loss_ = LOSS_MSE;
  double l2_ = 0.0;
  const bool group_dw_;  // dW of layers 1 and 0 in one launch (Switches::group_dw)
  const bool fold_on_;   // fold into the EPI_HEAD epilogue (Switches::fold; off: the unfolded route, tests)
  const bool show_plan_; // plan() reports each plan on stderr
  bool asum_shown_ = false; // forward() has reported the current plan's A-from-slabs layers
  long long cap_ = -1, planned_ = -1;
  long long plan_pin_ = -1; // > 0: ensure() plans for this many rows whatever the batch (evaluate's chunks)
  // Planned fold: the last hidden layer's [dW ; db] rows fold_c0_ .. in (fold_ input columns and the
  // bias row) are computed in the forward GEMM's EPI_HEAD epilogue instead of a mostly empty last
  // row tile of its dW GEMM; fold_ = -1: none.
  int fold_ = -1, fold_c0_ = 0;
  void plan(long long B);
  void ensure(long long B);
  bool side_reduced(int l, bool fused) const;
  bool head_route() const; // the last layer runs in a fused head kernel: its shape and both activations fit one
  bool rowhead_on(long long B) const; // the standalone head fed by the last hidden layer's slabs
  bool gemm_head_on() const; // the output layer runs inside the last hidden layer's forward GEMM
  int dx_tile(long long B, int N) const;
  // the layer GEMMs as the operands and the plan determine them; callers add their destination and route
  GemmDesc fwd_desc(size_t l, const float *P, const float *in, const int *idx, long long B) const;
  GemmDesc fwd_launch_desc(size_t l, const float *P, const float *in, const int *idx, long long B);
  void set_asum(GemmDesc &d, size_t l, const float *P, long long B);
  GemmDesc dw_desc(int l, const float *in, const int *rows, bool ones, const float *dZ, long long B) const;
  GemmDesc dx_desc(int l, const float *dZ, const float *Wsrc, int aux_act, float *out, long long B) const;
  // ---- activation workspace and slabs ----
  std::vector<DevBuf<float>> A_, D_;
  DevBuf<float> slab_, head_slab_, fslab_, fslab2_;
  float *fslab_buf(size_t l) const { return (l & 1) ? fslab2_.get() : fslab_.get(); } // forward slabs of layer l
  // ---- forward state and the two phases (mlp_eval.cpp) ----
  struct FwdState {
    long long B = -1;
    bool fused = false;
    int fold = -1, nloss = 0, lstart = 0;
  } fs_;
  void forward_phase(const float *P, const float *X, const float *Y, const int *idx, long long B, double inv_scale);
  // the output layer on the generic route: loss_diff or loss_xent on A_[nl - 1] -> D_[nl - 1], loss_part_
  void out_loss(const float *Y, const int *idx, long long B, double inv_scale);
  // What a backward phase writes besides the gradient, and the route it takes after its GEMMs. Default: the
  // gradient alone, by reduce_all on a single rank, by the reduced route under a communicator or with no rows.
  struct BwdRoute {
    const float *pdir = nullptr;    // direction of the g.p dot
    double *scal = nullptr;         // status block (null: no dots, no finishing launch)
    const TailFuse *tf = nullptr;   // fused optimizer tail, when every segment reduces in one pass
    WwPart ww = {};                 // the point's w.w partials
    bool local = false;             // stop before the all-reduce: [G | hi | lo] left for finish_reduced
    const float *hilo_in = nullptr; // reduced route: the loss words of the loss-only trial
    RedAllArgs *defer = nullptr;    // single rank, no status: leave the slabs to the consumer
  };
  struct BwdPass { // one backward phase: its arguments, and what it derives from them and from fs_
    const float *P = nullptr, *X = nullptr;
    const int *idx = nullptr;
    long long B = 0;
    double inv_scale = 0.0, lambda = 0.0;
    BwdRoute r; // the caller's, with ww cleared when lambda == 0
    float *G = nullptr, *Gl = nullptr; // Gl: where this rank's gradient lands before the collective
    bool empty = false, reduced = false, fused = false;
    int fold = -1, nloss = 0, lstart = -1;
    long long nfold = 0; // fold rows in the head slab
  };
  void backward_phase(const float *P, float *G, const float *X, const int *idx, long long B, double inv_scale,
                      double lambda, const BwdRoute &route);
  bool bwd_early(const BwdPass &b, EarlyLs *e) const;
  GemmDesc bwd_dw_desc(const BwdPass &b, int l) const;
  void bwd_launch(const BwdPass &b, const EarlyLs *early);
  void bwd_segments(const BwdPass &b, RedAllArgs &ra) const;
  void bwd_words(const BwdPass &b, const RedAllArgs &ra);
  void bwd_tail(const BwdPass &b, RedAllArgs &ra);
  void bwd_finish_reduced(const BwdPass &b, const RedAllArgs &ra);
  // ---- reduction and tail buffers ----
  DevBuf<float> hilo_, words_; // loss-only (hi, lo); data parallel: this rank's [grad | hi | lo] for the collective
  DevBuf<double> loss_part_, dots_part_, colpart_, trows_, tdots_;
  DevBuf<unsigned> cols_done_; // tail_cols arrival counter (zero between launches)
  // ---- R-pass workspace (mlp_curvature.cpp): R{Z}, R{A}, R{dZ} and delta per layer, two products, one segment ----
  std::vector<DevBuf<float>> RZ_, RA_, RD_, DL_;
  DevBuf<float> T1_, T2_, seg_;
  DevBuf<float> gsq_slab_; // grad_sq: the row chunks' partial slabs of one layer
  long long rcap_ = -1;
  void rpass_ensure(long long B); // grows the workspace to B rows
  // the R-pass products of layer l on B rows, with the forward, dW and dX plans of ensure(B)
  void rpass_linear_fwd(long long B, int l, const float *Wsrc, const float *in, const int *rows, bool with_bias,
                        float *out);
  void rpass_weight_grad(long long B, int l, const float *in, const int *rows, bool ones, const float *dZ,
                         float *dst);
  void rpass_back_prod(long long B, int l, const float *dZ, const float *Wsrc, int aux_act, float *out);
  void curv_finish(float *out, double lambda, const float *V, const int *abort); // all-reduce, + lambda V
  void curv_empty(float *out, double lambda, const float *V, const int *abort);  // an empty share: zeros that join
  // gnvp in two steps. gn_prepare: the workspaces and the unfused forward pass of the batch. gn_apply: the
  // R-forward, the loss's Hessian, the backward pass, the all-reduce and + lambda V, on the activations
  // gn_prepare left. The prepared state holds until the next call that writes the activation workspace (forward,
  // loss_grad, loss_only, evaluate, hvp, gnvp, grad_sq); P, X, idx and B must be gn_prepare's.
  void gn_prepare(const float *P, const float *X, const int *idx, long long B);
  void gn_apply(const float *P, const float *V, const float *X, const float *Y, const int *idx, long long B,
                double inv_scale, double lambda, float *Gv);
  // ---- CG state (gn_cg) ----
  // r, p, Ap, the partial tables [pap | rr x 2 | xdots x 3 | rz x 2], the status block, the abort word
  DevBuf<float> cg_r_, cg_p_, cg_ap_;
  DevBuf<double> cg_part_, cg_st_;
  DevBuf<int> cg_abort_;
  PinnedBuf<double> cg_hst_;
  // ---- Lanczos state (lanczos) ----
  // the basis rows (a ring of three, or steps + 1 without a caller's basis), w, the tables [dots x 2 passes | w.w],
  // the status block, the abort word
  DevBuf<float> lz_q_, lz_w_;
  DevBuf<double> lz_part_, lz_st_;
  DevBuf<int> lz_abort_;
  PinnedBuf<double> lz_hst_;
  // ---- evaluate buffers ----
  // per-workgroup loss partials and counts [rows, correct, topk] of every chunk, the confusion cells,
  // the partials' sum, the all-reduce words
  DevBuf<double> ev_part_, ev_sum_;
  DevBuf<unsigned> ev_cpart_;
  DevBuf<unsigned long long> ev_cnt_;
  DevBuf<float> ev_words_;
  PinnedBuf<float> ev_hwords_;
  PinnedBuf<double> ev_hsum_;
  // ---- counters ----
  long long evals_ = 0, rows_ = 0, loss_only_ = 0, gal_ = 0;
};

// Device-resident history of (s, y) pairs and its fp64 Gram state.
// Row groups the Gram sweep's partial table is folded into before the history step (large n).
constexpr int kGramFold = 32;

class History {
public:
  // gram_fin: Switches::gram_fin (1 / 0 forces the history route, -1: by history length)
  History(Ctx *ctx, int m, long long n, int gram_fin);
  HistView view() const { return v_; }
  void reset();
  // Gram sweep + bookkeeping (+ direction coefficients when want_dir > 0).
  // gred (nullable, nseg > 0): g.ga's values are still split-K slabs (Mlp::loss_grad_deferred); the fused
  // S-LBFGS sweep finishes them in place of reduce_all, other routes launch reduce_all first.
  void update(const GramArgs &g, int want_dir, int iter, double dsign, const RedAllArgs *gred = nullptr) {
    (void)update_impl(g, want_dir, iter, dsign, gred, nullptr);
  }
  // ww_part (nullable): also x_out's w.w partials (kernels.hpp WwPart)
  void combine(const float *g, float *dir, const float *x_in, float *x_out, float *x_out2, bool alpha_from_state,
               double alpha, double *ww_part = nullptr);
  // update(g, 1, iter, dsign) then combine(g.g_out, nullptr, x_in, x_out, x_out2, false, alpha)
  bool update_combine(const GramArgs &g, int iter, double dsign, const float *x_in, float *x_out, float *x_out2,
                      double alpha, const RedAllArgs *gred = nullptr);
  double *scal() const { return v_.scal; }
  int m() const { return v_.m; }

private:
  // cmb: the combine to fuse into the update when the S-LBFGS direction path can (dir_cols_combine);
  // returns whether it did
  bool update_impl(const GramArgs &g, int want_dir, int iter, double dsign, const RedAllArgs *gred,
                   const CombineArgs *cmb);

  Ctx *ctx_;
  HistView v_;
  DevBuf<float> S_, Y_;
  DevBuf<int> ist_;
  DevBuf<double> dstate_, part_, red_;
  // two-launch S-LBFGS update (dir.hip): partial rows, column sums, arrival counter
  DevBuf<double> drows_, ddots_, dkmat_;
  DevBuf<unsigned> dcount_;
  bool dir_on_ = false;
  // unfused path: Gram sweep (transposed partials in part_) + column sums whose last block runs the step
  DevBuf<double> gdots_;
  DevBuf<unsigned> gcount_;
  bool gfin_on_ = false;
};

} // namespace lbf
