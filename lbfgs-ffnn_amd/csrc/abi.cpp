// extern "C" surface of liblbfgs_amd_abi3.so (declared in include/lbfgs_amd.h). Every call converts
// internal exceptions into a status code + thread-local message (the reference aborts instead:
// src/cuda/common.cuh:18-23, cublas_handle.cuh:14-19).
#include "../../include/lbfgs_amd.h"
#include "host_rng.hpp"
#include "runtime.hpp"
#include "solvers.hpp"
#include "tridiag.hpp"

#include <rccl/rccl.h>

#include <cstring>
#include <memory>
#include <string>

using namespace lbf;

struct lbf_ctx {
  Ctx c;
  DevBuf<double> scal;
  DevBuf<float> gscratch;
};
struct lbf_mlp {
  lbf_ctx *ctx;
  std::unique_ptr<Mlp> net;
};
struct lbf_lbfgs {
  std::unique_ptr<Objective> obj;
  std::unique_ptr<LbfgsSolver> s;
};

namespace {
thread_local std::string g_err;

template <class F> int guard(F &&f) {
  try {
    f();
    return LBF_OK;
  } catch (const Error &e) {
    g_err = e.what();
    return e.code;
  } catch (const std::exception &e) {
    g_err = e.what();
    return LBF_ERR_INVALID;
  } catch (...) {
    g_err = "unknown error";
    return LBF_ERR_INVALID;
  }
}

void check_comm(ncclResult_t r, const char *what) {
  if (r != ncclSuccess) throw Error(LBF_ERR_COMM, std::string(what) + ": " + ncclGetErrorString(r));
}

void check_memory(const lbf_lbfgs_params &prm) { LBF_REQUIRE(prm.m >= 0 && prm.m <= 128, "m in [0, 128]"); }

// lbf_mlp_gn_cg (d_minv null) and lbf_mlp_gn_pcg
void gn_cg(lbf_mlp *net, const float *d_params, const float *d_b, const float *d_minv, const float *d_X,
           const float *d_Y, const int *d_idx, long long batch, double inv_scale, const lbf_cg_params *prm, float *d_x,
           lbf_cg_info *info) {
  net->ctx->c.set_device();
  Mlp::CgInfo ci;
  net->net->gn_cg(d_params, d_b, 1.0f, d_X, d_Y, d_idx, batch, inv_scale, prm->damping, prm->max_iters, prm->rtol,
                  prm->check, d_x, &ci, d_minv);
  if (info) *info = lbf_cg_info{ci.iterations, ci.status, ci.rr0, ci.rr, ci.xb, ci.xr, ci.xx};
}

// lbf_prof_read (values: total ms, counts) and lbf_prof_read_work (values: work units, no counts): the sections
// that were timed, the first `cap` of them written, all of them counted
void prof_read(lbf_ctx *ctx, const std::vector<double> &src, int cap, int *ids, double *values, long long *counts,
               int *n_out) {
  int k = 0;
  for (size_t i = 0; i < ctx->c.prof.cnt.size(); ++i) {
    if (ctx->c.prof.cnt[i] == 0) continue;
    if (k < cap) {
      if (ids) ids[k] = int(i);
      if (values) values[k] = i < src.size() ? src[i] : 0.0;
      if (counts) counts[k] = ctx->c.prof.cnt[i];
    }
    ++k;
  }
  *n_out = k;
}
} // namespace

extern "C" {

const char *lbf_last_error(void) { return g_err.c_str(); }
const char *lbf_version(void) { return "lbfgs_amd 0.4 (gfx950, abi 3)"; }
int lbf_abi_version(void) { return LBF_ABI_VERSION; }

int lbf_ctx_create(int device, void *stream, lbf_ctx **out) {
  return guard([&] {
    LBF_REQUIRE(out, "out");
    auto c = std::make_unique<lbf_ctx>();
    c->c.device = device;
    c->c.set_device();
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
      c->c.cus = cus;
    if (stream) {
      c->c.stream = static_cast<hipStream_t>(stream);
    } else {
      // blocking: ordered with the legacy stream torch uses; the highest priority, so that a solver's
      // critical chain is dispatched ahead of its own off-path work (the S-LBFGS twin, lowest priority)
      int least = 0, greatest = 0;
      if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest < least)
        LBF_HIP(hipStreamCreateWithPriority(&c->c.stream, hipStreamDefault, greatest));
      else
        LBF_HIP(hipStreamCreateWithFlags(&c->c.stream, hipStreamDefault));
      c->c.own_stream = true;
    }
    c->scal.resize(SC_N);
    LBF_HIP(hipMemset(c->scal.get(), 0, SC_N * sizeof(double)));
    *out = c.release();
  });
}

int lbf_ctx_destroy(lbf_ctx *ctx) {
  return guard([&] { delete ctx; });
}

int lbf_ctx_sync(lbf_ctx *ctx) {
  return guard([&] {
    LBF_REQUIRE(ctx, "ctx");
    LBF_HIP(hipStreamSynchronize(ctx->c.stream));
  });
}

void *lbf_ctx_stream(lbf_ctx *ctx) { return ctx ? static_cast<void *>(ctx->c.stream) : nullptr; }

int lbf_comm_unique_id(char out[128]) {
  return guard([&] {
    ncclUniqueId id;
    check_comm(ncclGetUniqueId(&id), "ncclGetUniqueId");
    static_assert(sizeof(id) <= 128, "unique id size");
    std::memset(out, 0, 128);
    std::memcpy(out, &id, sizeof(id));
  });
}

int lbf_comm_init(lbf_ctx *ctx, int nranks, int rank, const char id[128]) {
  return guard([&] {
    LBF_REQUIRE(ctx && nranks >= 1 && rank >= 0 && rank < nranks, "comm args");
    LBF_REQUIRE(id, "unique id");
    ctx->c.set_device();
    ctx->c.comm.reset();
    // a 1-rank communicator is created too: it routes evaluations through the data-parallel path
    // (local reduce -> ncclAllReduce -> tail), the single-GPU test of that path
    ctx->c.comm = make_rccl_comm(nranks, rank, id);
    ctx->c.rank = rank;
    ctx->c.nranks = nranks;
  });
}

int lbf_comm_init_local(lbf_ctx **ctxs, int nranks) {
  return guard([&] {
    LBF_REQUIRE(ctxs && nranks >= 1 && nranks <= kMaxLocalRanks, "comm_init_local: 1..16 contexts");
    for (int r = 0; r < nranks; ++r) {
      LBF_REQUIRE(ctxs[r], "comm_init_local: null context");
      LBF_REQUIRE(ctxs[r]->c.device == ctxs[0]->c.device, "comm_init_local: every context on one device");
      for (int q = 0; q < r; ++q) LBF_REQUIRE(ctxs[q] != ctxs[r], "comm_init_local: a context twice");
    }
    auto group = make_local_group(nranks, ctxs[0]->c.device);
    for (int r = 0; r < nranks; ++r) {
      ctxs[r]->c.comm = std::move(group[size_t(r)]);
      ctxs[r]->c.rank = r;
      ctxs[r]->c.nranks = nranks;
    }
  });
}

int lbf_comm_rank(lbf_ctx *ctx, int *rank, int *nranks) {
  return guard([&] {
    LBF_REQUIRE(ctx, "ctx");
    if (rank) *rank = ctx->c.rank;
    if (nranks) *nranks = ctx->c.nranks;
  });
}

int lbf_allreduce_sum(lbf_ctx *ctx, float *d_buf, size_t count) {
  return guard([&] {
    LBF_REQUIRE(ctx, "ctx");
    ctx->c.set_device();
    ctx->c.allreduce(d_buf, count);
  });
}

int lbf_mlp_create(lbf_ctx *ctx, int nlayers, const int *dims, const int *acts, lbf_mlp **out) {
  return guard([&] {
    LBF_REQUIRE(ctx && dims && acts && out, "null argument");
    static_assert(LBF_ACT_LINEAR == ACT_LINEAR && LBF_ACT_TANH == ACT_TANH && LBF_ACT_RELU == ACT_RELU &&
                      LBF_ACT_SIGMOID == ACT_SIGMOID && LBF_ACT_LEAKY_RELU == ACT_LEAKY_RELU &&
                      LBF_ACT_ELU == ACT_ELU && LBF_ACT_SOFTPLUS == ACT_SOFTPLUS && ACT_COUNT == 7,
                  "activation codes");
    ctx->c.set_device();
    auto m = std::make_unique<lbf_mlp>();
    m->ctx = ctx;
    m->net.reset(new Mlp(&ctx->c, nlayers, dims, acts, read_switches()));
    *out = m.release();
  });
}

int lbf_mlp_destroy(lbf_mlp *net) {
  return guard([&] { delete net; });
}

long long lbf_mlp_param_count(const lbf_mlp *net) { return net ? (long long)net->net->nparams() : -1; }

int lbf_mlp_init_params(lbf_mlp *net, unsigned seed, int init_mode, float *d_params) {
  return guard([&] {
    LBF_REQUIRE(net && d_params, "null argument");
    LBF_REQUIRE(init_mode == LBF_INIT_CPU || init_mode == LBF_INIT_CUDA, "init_mode");
    std::vector<float> h;
    init_params_host(net->net->layers(), seed, init_mode, h);
    net->ctx->c.set_device();
    LBF_HIP(hipMemcpyAsync(d_params, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice,
                           net->ctx->c.stream));
    LBF_HIP(hipStreamSynchronize(net->ctx->c.stream));
  });
}

int lbf_init_params_host(int nlayers, const int *dims, const int *acts, unsigned seed, int init_mode, float *h_out) {
  return guard([&] {
    LBF_REQUIRE(dims && acts && h_out && nlayers >= 1, "bad argument");
    LBF_REQUIRE(init_mode == LBF_INIT_CPU || init_mode == LBF_INIT_CUDA, "init_mode");
    std::vector<Layer> layers;
    size_t off = 0;
    for (int l = 0; l < nlayers; ++l) {
      Layer L;
      L.in = dims[l];
      L.out = dims[l + 1];
      L.act = acts[l];
      L.off = off;
      off += size_t(L.in + 1) * L.out;
      layers.push_back(L);
    }
    std::vector<float> h;
    init_params_host(layers, seed, init_mode, h);
    std::copy(h.begin(), h.end(), h_out);
  });
}

int lbf_mlp_forward(lbf_mlp *net, const float *d_params, const float *d_X, long long batch, float *d_out) {
  return guard([&] {
    LBF_REQUIRE(net && d_params && d_X && d_out && batch >= 0, "bad argument");
    net->ctx->c.set_device();
    const float *o = net->net->forward(d_params, d_X, nullptr, batch);
    const int Out = net->net->layers().back().out;
    LBF_HIP(hipMemcpyAsync(d_out, o, size_t(batch) * Out * sizeof(float), hipMemcpyDeviceToDevice,
                           net->ctx->c.stream));
  });
}

int lbf_mlp_loss_grad(lbf_mlp *net, const float *d_params, float *d_grad, const float *d_X, const float *d_Y,
                      const int *d_idx, long long batch, double inv_scale, double l2, double *h_loss) {
  return guard([&] {
    LBF_REQUIRE(net && d_params && d_grad && d_X && d_Y && batch >= 0, "bad argument");
    lbf_ctx *c = net->ctx;
    c->c.set_device();
    const size_t n = net->net->nparams();
    c->gscratch.ensure(n + 4);
    net->net->loss_grad(d_params, c->gscratch.get(), d_X, d_Y, d_idx, batch, inv_scale, l2, nullptr, c->scal.get());
    LBF_HIP(hipMemcpyAsync(d_grad, c->gscratch.get(), n * sizeof(float), hipMemcpyDeviceToDevice, c->c.stream));
    if (h_loss) {
      double tmp[SC_N];
      LBF_HIP(hipMemcpyAsync(tmp, c->scal.get(), SC_N * sizeof(double), hipMemcpyDeviceToHost, c->c.stream));
      LBF_HIP(hipStreamSynchronize(c->c.stream));
      *h_loss = tmp[SC_LOSS];
    }
  });
}

int lbf_mlp_batch_grads(lbf_mlp *net, const float *d_params, const float *d_X, const float *d_Y, int nmb,
                        long long cnt, double inv_scale, double l2, float *d_grads, long long ld) {
  return guard([&] {
    LBF_REQUIRE(net && d_params && d_X && d_Y && d_grads && nmb > 0 && cnt > 0, "bad argument");
    lbf_ctx *c = net->ctx;
    LBF_REQUIRE(!c->c.dp(), "lbf_mlp_batch_grads: single rank only");
    c->c.set_device();
    net->net->batch_grads(d_params, d_X, d_Y, nmb, cnt, inv_scale, l2, d_grads, ld, false);
    LBF_HIP(hipStreamSynchronize(c->c.stream));
  });
}

int lbf_mlp_loss(lbf_mlp *net, const float *d_params, const float *d_X, const float *d_Y, const int *d_idx,
                 long long batch, double inv_scale, double *h_loss) {
  return guard([&] {
    LBF_REQUIRE(net && d_params && d_X && d_Y && h_loss && batch > 0, "bad argument");
    lbf_ctx *c = net->ctx;
    c->c.set_device();
    net->net->loss_only(d_params, d_X, d_Y, d_idx, batch, inv_scale, c->scal.get());
    double tmp[SC_N];
    LBF_HIP(hipMemcpyAsync(tmp, c->scal.get(), SC_N * sizeof(double), hipMemcpyDeviceToHost, c->c.stream));
    LBF_HIP(hipStreamSynchronize(c->c.stream));
    *h_loss = tmp[SC_LOSS];
  });
}

int lbf_mlp_hvp(lbf_mlp *net, const float *d_params, const float *d_v, const float *d_X, const float *d_Y,
                const int *d_idx, long long batch, double inv_scale, double l2, float *d_hv) {
  return guard([&] {
    LBF_REQUIRE(net && d_params && d_v && d_hv && batch >= 0 && (batch == 0 || (d_X && d_Y)), "bad argument");
    net->ctx->c.set_device();
    net->net->hvp(d_params, d_v, d_X, d_Y, d_idx, batch, inv_scale, l2, d_hv);
    LBF_HIP(hipStreamSynchronize(net->ctx->c.stream));
  });
}

int lbf_mlp_gnvp(lbf_mlp *net, const float *d_params, const float *d_v, const float *d_X, const float *d_Y,
                 const int *d_idx, long long batch, double inv_scale, double l2, float *d_gv) {
  return guard([&] {
    LBF_REQUIRE(net && d_params && d_v && d_gv && batch >= 0 && (batch == 0 || (d_X && d_Y)), "bad argument");
    net->ctx->c.set_device();
    net->net->gnvp(d_params, d_v, d_X, d_Y, d_idx, batch, inv_scale, l2, d_gv);
    LBF_HIP(hipStreamSynchronize(net->ctx->c.stream));
  });
}

int lbf_mlp_set_loss(lbf_mlp *net, int loss) {
  return guard([&] {
    LBF_REQUIRE(net, "null argument");
    static_assert(LBF_LOSS_MSE == LOSS_MSE && LBF_LOSS_SOFTMAX_XENT == LOSS_XENT, "loss codes");
    net->net->set_loss(loss);
  });
}

int lbf_mlp_get_loss(const lbf_mlp *net, int *loss) {
  return guard([&] {
    LBF_REQUIRE(net && loss, "null argument");
    *loss = net->net->loss();
  });
}

int lbf_mlp_set_l2(lbf_mlp *net, double l2) {
  return guard([&] {
    LBF_REQUIRE(net, "null argument");
    net->net->set_l2(l2);
  });
}

int lbf_mlp_get_l2(const lbf_mlp *net, double *l2) {
  return guard([&] {
    LBF_REQUIRE(net && l2, "null argument");
    *l2 = net->net->l2();
  });
}

int lbf_mlp_evaluate(lbf_mlp *net, const float *d_params, const float *d_X, const float *d_Y, const int *d_idx,
                     long long batch, double inv_scale, int k, long long chunk_rows, lbf_eval_result *h_res,
                     long long *h_confusion, int *d_pred, float *d_proba) {
  return guard([&] {
    LBF_REQUIRE(net && d_params && h_res && batch >= 0 && (batch == 0 || d_X) && chunk_rows >= 0, "bad argument");
    net->ctx->c.set_device();
    const Mlp::EvalTotals t =
        net->net->evaluate(d_params, d_X, d_Y, d_idx, batch, k, chunk_rows, h_confusion, d_pred, d_proba);
    h_res->loss = 0.5 * t.sse * inv_scale;
    h_res->rows = t.rows;
    h_res->correct = t.correct;
    h_res->topk = t.topk;
    h_res->k = k;
    h_res->reserved = 0;
  });
}

int lbf_mlp_fd_hvp(lbf_mlp *net, const float *d_params, const float *d_v, const float *d_X, const float *d_Y,
                   const int *d_idx, long long batch, double inv_scale, double l2, double eps, float *d_y) {
  return guard([&] {
    LBF_REQUIRE(net && d_params && d_v && d_y && batch >= 0 && (batch == 0 || (d_X && d_Y)) && eps > 0.0,
                "bad argument");
    lbf_ctx *c = net->ctx;
    c->c.set_device();
    const size_t n = net->net->nparams(), ld = (n + 3) / 4 * 4, lg = (n + 2 + 3) / 4 * 4;
    DevBuf<float> w(2 * ld), g(2 * lg);
    fd_hvp_grads(net->net.get(), d_params, d_v, d_X, d_Y, d_idx, batch, inv_scale, l2, eps, w.get(), w.get() + ld,
                 g.get(), g.get() + lg, c->scal.get());
    diff_scale(c->c.stream, (long long)n, g.get(), g.get() + lg, float(1.0 / (2.0 * eps)), d_y);
    LBF_HIP(hipStreamSynchronize(c->c.stream));
  });
}

int lbf_two_loop(lbf_ctx *ctx, long long n, int k, const float *d_S, const float *d_Y, const double *h_rho,
                 const float *d_g, float *d_dir, int mode) {
  return guard([&] {
    LBF_REQUIRE(ctx && d_g && d_dir && n > 0 && k >= 0 && k <= 128, "bad argument");
    LBF_REQUIRE(k == 0 || (d_S && d_Y && h_rho), "history pointers");
    LBF_REQUIRE(mode >= 0 && mode <= 3, "mode");
    ctx->c.set_device();
    hipStream_t s = ctx->c.stream;
    const int policy = mode == 0 ? POL_CPU : (mode == 1 || mode == 3 ? POL_SLBFGS : POL_CUDA);
    const double dsign = mode == 1 || mode == 3 ? 1.0 : -1.0;
    History h(&ctx->c, k, n, read_switches().gram_fin);
    DevBuf<float> zero{size_t(n)};
    LBF_HIP(hipMemsetAsync(zero.get(), 0, size_t(n) * sizeof(float), s));
    if (mode == 3) { // the S-LBFGS solver's own route (SlbfgsSolver::epoch_steps)
      LBF_REQUIRE(k <= DIR_MAXM && n % 4 == 0 && dir_supported(k, n) &&
                      aligned16(d_g, d_dir) && (k == 0 || aligned16(d_S, d_Y)),
                  "mode 3: k <= 16, n % 4 == 0, 16-B aligned vectors");
      for (int i = 0; i < k; ++i) { // pair updates: |y.s| > 1e-10, rho = 1 / y.s and the map K on the device
        GramArgs ga;
        ga.policy = policy;
        ga.has_pair = 1;
        ga.sa = d_S + size_t(i) * n;
        ga.sb = zero.get();
        ga.ya = d_Y + size_t(i) * n;
        ga.yb = zero.get();
        h.update(ga, 0, 1, dsign);
      }
      DevBuf<float> v{size_t(n)};
      GramArgs gg; // a direction-only step: dir_cols_combine, x_out = 0 + 1 * (+H g)
      gg.policy = policy;
      gg.has_g = 1;
      gg.ga = d_g;
      gg.g_out = v.get();
      LBF_REQUIRE(h.update_combine(gg, 1, dsign, zero.get(), d_dir, nullptr, 1.0),
                  "mode 3: the direction-only step did not take the coefficient-map route");
      ctx->c.host.ensure(1);
      LBF_HIP(hipMemcpyAsync(ctx->c.host.get(), h.view().scal + SC_KERR, sizeof(double), hipMemcpyDeviceToHost, s));
      LBF_HIP(hipStreamSynchronize(s));
      LBF_REQUIRE(ctx->c.host[0] == 0.0, "mode 3: the coefficient map K is out of step with the ring");
      return;
    }
    for (int i = 0; i < k; ++i) {
      GramArgs ga;
      ga.policy = policy;
      ga.has_pair = 1;
      ga.sa = d_S + size_t(i) * n;
      ga.sb = zero.get();
      ga.ya = d_Y + size_t(i) * n;
      ga.yb = zero.get();
      h.update(ga, -1, 1, dsign); // -1: push unconditionally
    }
    if (k > 0)
      LBF_HIP(hipMemcpyAsync(h.view().rho, h_rho, size_t(k) * sizeof(double), hipMemcpyHostToDevice, s));
    GramArgs gg;
    gg.policy = policy;
    gg.has_g = 1;
    gg.ga = d_g;
    h.update(gg, 2, 1, dsign); // 2: direction without the solver's descent fallback
    h.combine(d_g, d_dir, nullptr, nullptr, nullptr, false, 0.0);
    LBF_HIP(hipStreamSynchronize(s));
  });
}

int lbf_dot(lbf_ctx *ctx, long long n, const float *d_x, const float *d_y, double *h_out) {
  return guard([&] {
    LBF_REQUIRE(ctx && d_x && d_y && h_out && n >= 0, "bad argument");
    ctx->c.set_device();
    hipStream_t s = ctx->c.stream;
    const int nw = dots_partials_wg(n);
    ctx->c.part.ensure(size_t(nw));
    ctx->c.red.ensure(1);
    ctx->c.host.ensure(1);
    dot_partials(s, n, d_x, d_y, ctx->c.part.get());
    reduce_rows(s, ctx->c.part.get(), nw, 1, ctx->c.red.get());
    LBF_HIP(hipMemcpyAsync(ctx->c.host.get(), ctx->c.red.get(), sizeof(double), hipMemcpyDeviceToHost, s));
    LBF_HIP(hipStreamSynchronize(s));
    *h_out = ctx->c.host[0];
  });
}

int lbf_nrm2(lbf_ctx *ctx, long long n, const float *d_x, double *h_out) {
  double d = 0;
  int r = lbf_dot(ctx, n, d_x, d_x, &d);
  if (r == LBF_OK && h_out) *h_out = std::sqrt(d);
  return r;
}

int lbf_axpy(lbf_ctx *ctx, long long n, float alpha, const float *d_x, float *d_y) {
  return guard([&] {
    LBF_REQUIRE(ctx && d_x && d_y && n >= 0, "bad argument");
    ctx->c.set_device();
    axpy(ctx->c.stream, n, alpha, d_x, d_y);
  });
}

int lbf_scal(lbf_ctx *ctx, long long n, float alpha, float *d_x) {
  return guard([&] {
    LBF_REQUIRE(ctx && d_x && n >= 0, "bad argument");
    ctx->c.set_device();
    scal(ctx->c.stream, n, alpha, d_x);
  });
}

void lbf_lbfgs_default_params(lbf_lbfgs_params *p, int line_search) {
  if (!p) return;
  p->line_search = line_search;
  if (line_search == LBF_LS_ARMIJO) { // minimizer_base.cuh:63-64, lbfgs.cuh:118 (m_ = 16)
    p->m = 16;
    p->max_iters = 200;
    p->tol = 1e-6;
    p->max_line_iters = 20;
    p->c1 = 1e-4;
    p->c2 = 0.9;
    p->rho = 0.5;
  } else { // full_batch_minimizer.hpp:107-116, lbfgs.hpp:142 (m = 16)
    p->m = 16;
    p->max_iters = 1000;
    p->tol = 1e-10;
    p->max_line_iters = 50;
    p->c1 = 1e-4;
    p->c2 = 0.9;
    p->rho = 0.5;
  }
}

void lbf_gd_default_params(lbf_gd_params *p) { // gd.cuh:103-104, minimizer_base.cuh:62-63
  if (!p) return;
  p->lr = 0.01;
  p->momentum = 0.9;
  p->max_iters = 200;
  p->tol = 1e-6;
}

void lbf_sgd_default_params(lbf_sgd_params *p) { // sgd.cuh:156-161, minimizer_base.cuh:62-63
  if (!p) return;
  p->lr = 0.01;
  p->momentum = 0.9;
  p->batch = 64;
  p->decay_rate = 1.0;
  p->decay_step = 0;
  p->max_epochs = 200;
  p->tol = 1e-6;
}

int lbf_gd_solve(lbf_mlp *net, const lbf_gd_params *prm, float *d_params, const float *d_X, const float *d_Y,
                 long long n_local, long long n_global, lbf_record *rec, lbf_solve_info *info) {
  return guard([&] {
    LBF_REQUIRE(net && prm, "null argument");
    run_gd(net->net.get(), *prm, d_params, d_X, d_Y, n_local, n_global, rec, info);
  });
}

int lbf_sgd_solve(lbf_mlp *net, const lbf_sgd_params *prm, float *d_params, const float *d_X, const float *d_Y,
                  long long N, lbf_record *rec, lbf_solve_info *info) {
  return guard([&] {
    LBF_REQUIRE(net && prm, "null argument");
    run_sgd(net->net.get(), *prm, d_params, d_X, d_Y, N, rec, info);
  });
}

void lbf_cg_default_params(lbf_cg_params *p) {
  if (!p) return;
  p->max_iters = 50;
  p->rtol = 0.1;
  p->damping = 0.0;
  p->check = 10;
}

int lbf_mlp_gn_cg(lbf_mlp *net, const float *d_params, const float *d_b, const float *d_X, const float *d_Y,
                  const int *d_idx, long long batch, double inv_scale, const lbf_cg_params *prm, float *d_x,
                  lbf_cg_info *info) {
  return guard([&] {
    LBF_REQUIRE(net && prm && d_params && d_b && d_x && batch >= 0 && (batch == 0 || (d_X && d_Y)), "bad argument");
    gn_cg(net, d_params, d_b, nullptr, d_X, d_Y, d_idx, batch, inv_scale, prm, d_x, info);
  });
}

int lbf_mlp_gn_pcg(lbf_mlp *net, const float *d_params, const float *d_b, const float *d_minv, const float *d_X,
                   const float *d_Y, const int *d_idx, long long batch, double inv_scale, const lbf_cg_params *prm,
                   float *d_x, lbf_cg_info *info) {
  return guard([&] {
    LBF_REQUIRE(net && prm && d_params && d_b && d_minv && d_x && batch >= 0 && (batch == 0 || (d_X && d_Y)),
                "bad argument");
    gn_cg(net, d_params, d_b, d_minv, d_X, d_Y, d_idx, batch, inv_scale, prm, d_x, info);
  });
}

int lbf_mlp_grad_sq(lbf_mlp *net, const float *d_params, const float *d_X, const float *d_Y, const int *d_idx,
                    long long batch, double scale, float *d_out) {
  return guard([&] {
    LBF_REQUIRE(net && d_params && d_out && batch >= 0 && (batch == 0 || (d_X && d_Y)), "bad argument");
    LBF_REQUIRE(std::isfinite(scale) && scale >= 0.0, "scale must be finite and >= 0");
    net->ctx->c.set_device();
    net->net->grad_sq(d_params, d_X, d_Y, d_idx, batch, scale, d_out);
    LBF_HIP(hipStreamSynchronize(net->ctx->c.stream));
  });
}

int lbf_mlp_gn_cg_residual(lbf_mlp *net, float *d_r) {
  return guard([&] {
    LBF_REQUIRE(net && d_r, "null argument");
    LBF_REQUIRE(net->net->cg_residual(), "no conjugate-gradient solve has run on this network");
    net->ctx->c.set_device();
    hipStream_t s = net->ctx->c.stream;
    LBF_HIP(hipMemcpyAsync(d_r, net->net->cg_residual(), net->net->nparams() * sizeof(float), hipMemcpyDeviceToDevice,
                           s));
    LBF_HIP(hipStreamSynchronize(s));
  });
}

void lbf_lanczos_default_params(lbf_lanczos_params *p) {
  if (!p) return;
  p->steps = 32;
  p->matrix = LBF_HVP_GAUSS_NEWTON;
  p->reorth = 1;
  p->check = 8;
  p->l2 = 0.0;
  p->breakdown_rtol = 1.1e-3;
}

int lbf_mlp_lanczos(lbf_mlp *net, const float *d_params, const float *d_v0, const float *d_X, const float *d_Y,
                    const int *d_idx, long long batch, double inv_scale, const lbf_lanczos_params *prm,
                    double *h_alpha, double *h_beta, float *d_basis, long long ld, lbf_lanczos_info *info) {
  return guard([&] {
    // the parameters first, so that a caller without a device still learns which of them is wrong
    LBF_REQUIRE(prm, "null parameters");
    LBF_REQUIRE(prm->steps >= 1 && prm->steps <= LZ_MAX_STEPS, "steps must be in 1..128");
    LBF_REQUIRE(prm->matrix == LBF_HVP_EXACT || prm->matrix == LBF_HVP_GAUSS_NEWTON,
                "matrix must be LBF_HVP_EXACT or LBF_HVP_GAUSS_NEWTON");
    LBF_REQUIRE(prm->reorth == 0 || prm->reorth == 1, "reorth must be 0 or 1");
    LBF_REQUIRE(prm->check >= 1, "check must be >= 1");
    LBF_REQUIRE(std::isfinite(prm->l2) && prm->l2 >= 0.0, "l2 must be finite and >= 0");
    LBF_REQUIRE(std::isfinite(prm->breakdown_rtol) && prm->breakdown_rtol >= 0.0,
                "breakdown_rtol must be finite and >= 0");
    LBF_REQUIRE(net && d_params && d_v0 && h_alpha && h_beta && batch >= 0 && (batch == 0 || (d_X && d_Y)),
                "null handle or bad batch");
    net->ctx->c.set_device();
    Mlp::LanczosInfo li;
    net->net->lanczos(d_params, d_v0, d_X, d_Y, d_idx, batch, inv_scale, prm->l2, prm->matrix == LBF_HVP_EXACT,
                      prm->steps, prm->reorth != 0, prm->check, prm->breakdown_rtol, h_alpha, h_beta, d_basis, ld, &li);
    if (info) *info = lbf_lanczos_info{li.steps, li.status, li.v0_norm};
  });
}

int lbf_tridiag_eig(int m, const double *alpha, const double *beta, double *theta, double *first_sq, double *vecs) {
  return guard([&] {
    LBF_REQUIRE(m >= 1 && alpha && theta && (m == 1 || beta), "m >= 1, alpha, theta and (m > 1) beta");
    LBF_REQUIRE(tridiag_eig(m, alpha, beta, theta, first_sq, vecs), "the QL iteration did not converge");
  });
}

void lbf_hf_default_params(lbf_hf_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->max_iters = 100;
  p->tol = 1e-6;
  p->cg_iters = 50;
  p->cg_rtol = 0.1;
  p->cg_check = 10;
  p->damping0 = 1.0;
  p->damp_up = 1.5;
  p->damp_down = 2.0 / 3.0;
  p->ratio_lo = 0.25;
  p->ratio_hi = 0.75;
  p->c1 = 1e-4;
  p->rho = 0.5;
  p->max_line_iters = 20;
}

int lbf_hf_solve(lbf_mlp *net, const lbf_hf_params *prm, float *d_params, const float *d_X, const float *d_Y,
                 long long n_local, long long n_global, lbf_record *rec, lbf_solve_info *info) {
  return guard([&] {
    LBF_REQUIRE(net && prm, "null argument");
    run_hf(net->net.get(), *prm, d_params, d_X, d_Y, n_local, n_global, rec, info);
  });
}

void lbf_hf_precond_default(lbf_hf_precond *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->mode = LBF_PRECOND_NONE;
  p->exponent = 0.75;
  p->refresh = 1;
}

int lbf_hf_solve_pc(lbf_mlp *net, const lbf_hf_params *prm, const lbf_hf_precond *pc, float *d_params,
                    const float *d_X, const float *d_Y, long long n_local, long long n_global, lbf_record *rec,
                    lbf_solve_info *info) {
  return guard([&] {
    LBF_REQUIRE(net && prm, "null argument");
    run_hf(net->net.get(), *prm, d_params, d_X, d_Y, n_local, n_global, rec, info, pc);
  });
}

void lbf_owlqn_default_params(lbf_owlqn_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->m = 10;
  p->max_iters = 100;
  p->tol = 1e-6;
  p->c1 = 1e-4;
  p->rho = 0.5;
  p->max_line_iters = 20;
}

int lbf_owlqn_solve(lbf_mlp *net, const lbf_owlqn_params *prm, float *d_params, const float *d_X, const float *d_Y,
                    long long n_local, long long n_global, lbf_record *rec, lbf_solve_info *info,
                    lbf_owlqn_stats *stats) {
  return guard([&] {
    LBF_REQUIRE(net && prm, "null argument");
    run_owlqn(net->net.get(), *prm, d_params, d_X, d_Y, n_local, n_global, rec, info, stats);
  });
}

namespace {
// The sweeps' scratch is the context's BLAS-1 scratch: [tables | status block] on the device, the block on the host.
void owl_sweep_args(lbf_mlp *net, double l1, int l1_bias, OwlArgs &a) {
  LBF_REQUIRE(std::isfinite(l1) && l1 >= 0.0, "l1 must be finite and >= 0");
  Ctx &c = net->ctx->c;
  c.set_device();
  a.n = (long long)net->net->nparams();
  a.coef = owl_coef(*net->net, l1, l1_bias);
  a.l1 = l1;
  const size_t words = size_t(owl_table_words(a.n));
  c.part.ensure(words + OWL_N);
  c.host.ensure(OWL_N);
  a.tab = c.part.get();
  a.st = c.part.get() + words;
}
void owl_sweep_read(lbf_mlp *net, const OwlArgs &a) {
  Ctx &c = net->ctx->c;
  LBF_HIP(hipMemcpyAsync(c.host.get(), a.st, OWL_N * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  LBF_HIP(hipStreamSynchronize(c.stream));
}
} // namespace

int lbf_mlp_l1_pseudo_grad(lbf_mlp *net, const float *d_x, const float *d_g, double l1, int l1_bias, float *d_pg,
                           lbf_owlqn_stats *h_stats) {
  return guard([&] {
    LBF_REQUIRE(net && d_x && d_g && d_pg, "null argument");
    OwlArgs a;
    owl_sweep_args(net, l1, l1_bias, a);
    a.x = d_x;
    a.g = d_g;
    a.out = d_pg;
    owl_pseudo(net->ctx->c.stream, a);
    owl_pseudo_finish(net->ctx->c.stream, a);
    owl_sweep_read(net, a);
    if (h_stats) {
      const double *h = net->ctx->c.host.get();
      h_stats->zeros = (long long)h[OWL_ZEROS];
      h_stats->penalised = owl_penalised_count(*net->net, l1_bias);
      h_stats->l1_term = h[OWL_L1];
      h_stats->pg_norm = std::sqrt(h[OWL_PGPG]);
    }
  });
}

int lbf_mlp_l1_trial(lbf_mlp *net, const float *d_x, const float *d_d, const float *d_pg, double l1, int l1_bias,
                     float alpha, float *d_xnew, double *h_l1_term, double *h_ww, double *h_dec, long long *h_zeros) {
  return guard([&] {
    LBF_REQUIRE(net && d_x && d_d && d_pg && d_xnew, "null argument");
    OwlArgs a;
    owl_sweep_args(net, l1, l1_bias, a);
    a.x = d_x;
    a.d = d_d;
    a.pg = d_pg;
    a.alpha = alpha;
    a.out = d_xnew;
    owl_trial(net->ctx->c.stream, a);
    owl_trial_finish(net->ctx->c.stream, a);
    owl_sweep_read(net, a);
    const double *h = net->ctx->c.host.get();
    if (h_l1_term) *h_l1_term = h[OWL_L1];
    if (h_ww) *h_ww = h[OWL_WW];
    if (h_dec) *h_dec = h[OWL_DEC];
    if (h_zeros) *h_zeros = (long long)h[OWL_ZEROS];
  });
}

void lbf_adam_default_params(lbf_adam_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->lr = 1e-3;
  p->beta1 = 0.9;
  p->beta2 = 0.999;
  p->eps = 1e-8;
  p->batch = 128;
  p->shuffle = 1;
  p->seed = 123;
  p->decay_rate = 1.0; // lbf_sgd_default_params
  p->max_epochs = 200;
  p->tol = 1e-6;
}

int lbf_adam_coefs(const lbf_adam_params *prm, double lr_now, long long t, lbf_adam_coef *h_out) {
  return guard([&] {
    LBF_REQUIRE(prm && h_out, "null argument");
    adam_check(*prm);
    LBF_REQUIRE(t >= 1 && std::isfinite(lr_now) && lr_now > 0.0, "t >= 1, lr_now finite and > 0");
    double p1 = 1.0, p2 = 1.0; // the solver's running products: one multiplication per step
    for (long long i = 0; i < t; ++i) {
      p1 *= prm->beta1;
      p2 *= prm->beta2;
    }
    const AdamCoef k = adam_coefs(*prm, lr_now, p1, p2);
    std::memcpy(h_out, &k, sizeof(k));
  });
}

int lbf_adam_epoch_orders(long long N, unsigned seed, int epochs, int *h_out) {
  return guard([&] {
    LBF_REQUIRE(N >= 1 && N < (1LL << 31) && epochs >= 0 && h_out, "bad argument");
    std::mt19937 rng(seed);
    for (int e = 0; e < epochs; ++e) epoch_order(rng, N, h_out + size_t(e) * size_t(N));
  });
}

int lbf_adam_step(lbf_ctx *ctx, long long n, const lbf_adam_coef *coef, float *d_w, float *d_m, float *d_v,
                  const float *d_g, const double *d_gg) {
  return guard([&] {
    LBF_REQUIRE(ctx && coef && d_w && d_m && d_v && d_g && n >= 0, "bad argument");
    ctx->c.set_device();
    AdamCoef k;
    std::memcpy(&k, coef, sizeof(k));
    adam_step(ctx->c.stream, n, k, d_g, d_m, d_v, d_w, d_gg);
  });
}

struct lbf_adam {
  std::unique_ptr<AdamSolver> s;
};

int lbf_adam_begin(lbf_mlp *net, const lbf_adam_params *prm, float *d_params, const float *d_X, const float *d_Y,
                   long long N, lbf_adam **out) {
  return guard([&] {
    LBF_REQUIRE(prm && out, "null argument");
    adam_check(*prm);
    LBF_REQUIRE(N >= 1 && N < (1LL << 31), "N must lie in [1, 2^31)");
    LBF_REQUIRE(net && d_params && d_X && d_Y, "null argument");
    net->ctx->c.set_device();
    auto h = std::make_unique<lbf_adam>();
    h->s.reset(new AdamSolver(net->net.get(), *prm, d_params, d_X, d_Y, N));
    *out = h.release();
  });
}

int lbf_adam_iterate(lbf_adam *s, int epochs, lbf_record *rec, lbf_solve_info *info, int *h_epochs) {
  return guard([&] {
    LBF_REQUIRE(s && epochs >= 0, "bad argument");
    s->s->iterate(epochs, rec);
    s->s->info(info);
    if (h_epochs) *h_epochs = s->s->epochs();
  });
}

int lbf_adam_end(lbf_adam *s) {
  return guard([&] { delete s; });
}

int lbf_adam_solve(lbf_mlp *net, const lbf_adam_params *prm, float *d_params, const float *d_X, const float *d_Y,
                   long long N, lbf_record *rec, lbf_solve_info *info) {
  lbf_adam *s = nullptr;
  int r = lbf_adam_begin(net, prm, d_params, d_X, d_Y, N, &s);
  if (r != LBF_OK) return r;
  r = lbf_adam_iterate(s, prm->max_epochs, rec, info, nullptr);
  lbf_adam_end(s);
  return r;
}

void lbf_slbfgs_default_params(lbf_slbfgs_params *p) {
  if (!p) return;
  p->max_epochs = 1000; // stochastic_minimizer.hpp:44-47
  p->tol = 1e-4;
  p->M = 10;
  p->L = 10;
  p->b = 128;
  p->b_H = 64;
  p->step = 0.01;
  p->lambda = 1e-4;
  p->seed = 123;
  p->fd_eps = 1e-4;
  p->hvp_exact = 0;
  p->pair_trace = nullptr;
  p->pair_trace_cap = 0;
  p->dp_mode = LBF_SLBFGS_DP_REPLICATED;
}

int lbf_lbfgs_begin(lbf_mlp *net, const lbf_lbfgs_params *prm, float *d_params, const float *d_X,
                    const float *d_Y, long long n_local, long long n_global, lbf_lbfgs **out) {
  return guard([&] {
    LBF_REQUIRE(net && prm && out, "null argument");
    check_memory(*prm);
    net->ctx->c.set_device();
    // a data-parallel rank with an empty shard (n_local == 0) has no data pointers
    LBF_REQUIRE(d_params && (n_local == 0 || (d_X && d_Y)), "null pointer");
    LBF_REQUIRE(n_local >= 0 && n_global > 0, "batch sizes");
    auto s = std::make_unique<lbf_lbfgs>();
    s->obj.reset(new MlpObjective(net->net.get(), d_X, d_Y, n_local, n_global));
    s->s.reset(new LbfgsSolver(s->obj.get(), *prm, d_params, read_switches()));
    *out = s.release();
  });
}

int lbf_lbfgs_iterate(lbf_lbfgs *s, int iters, lbf_record *rec, lbf_solve_info *info) {
  return guard([&] {
    LBF_REQUIRE(s && iters >= 0, "bad argument");
    s->s->iterate(iters, rec);
    s->s->info(info);
  });
}

int lbf_lbfgs_end(lbf_lbfgs *s) {
  return guard([&] { delete s; });
}

int lbf_lbfgs_solve(lbf_mlp *net, const lbf_lbfgs_params *prm, float *d_params, const float *d_X,
                    const float *d_Y, long long n_local, long long n_global, lbf_record *rec,
                    lbf_solve_info *info) {
  // CudaMinimizerBase::solve contract (minimizer_base.cuh:54-59): n <= 0 or params == nullptr is a
  // no-op with iterations() == 0 (lbfgs.cuh:45-48).
  if (!net || !d_params || net->net->nparams() == 0) {
    if (info) std::memset(info, 0, sizeof(*info));
    return LBF_OK;
  }
  lbf_lbfgs *s = nullptr;
  int r = lbf_lbfgs_begin(net, prm, d_params, d_X, d_Y, n_local, n_global, &s);
  if (r != LBF_OK) return r;
  r = lbf_lbfgs_iterate(s, prm->max_iters, rec, info);
  lbf_lbfgs_end(s);
  return r;
}

int lbf_lbfgs_solve_fn(lbf_ctx *ctx, const lbf_lbfgs_params *prm, long long n, float *d_params,
                       lbf_loss_grad_fn fn, void *user, lbf_record *rec, lbf_solve_info *info) {
  if (!d_params || n <= 0) { // lbfgs.cuh:45-48
    if (info) std::memset(info, 0, sizeof(*info));
    return LBF_OK;
  }
  return guard([&] {
    LBF_REQUIRE(ctx && prm && fn, "null argument");
    check_memory(*prm);
    ctx->c.set_device();
    CallbackObjective obj(&ctx->c, n, fn, user);
    LbfgsSolver s(&obj, *prm, d_params, read_switches());
    s.iterate(prm->max_iters, rec);
    s.info(info);
  });
}

int lbf_device_alloc(lbf_ctx *ctx, size_t bytes, void **out) {
  return guard([&] {
    LBF_REQUIRE(ctx && out, "null argument");
    ctx->c.set_device();
    *out = nullptr;
    if (bytes) LBF_HIP(hipMalloc(out, bytes));
  });
}

int lbf_device_free(lbf_ctx *ctx, void *p) {
  return guard([&] {
    LBF_REQUIRE(ctx, "ctx");
    ctx->c.set_device();
    if (p) LBF_HIP(hipFree(p));
  });
}

int lbf_memcpy(lbf_ctx *ctx, void *dst, const void *src, size_t bytes, int kind) {
  return guard([&] {
    LBF_REQUIRE(ctx && (bytes == 0 || (dst && src)) && kind >= 0 && kind <= 2, "bad argument");
    ctx->c.set_device();
    const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : (kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
    if (bytes) LBF_HIP(hipMemcpyAsync(dst, src, bytes, k, ctx->c.stream));
    LBF_HIP(hipStreamSynchronize(ctx->c.stream));
  });
}

int lbf_slbfgs_solve(lbf_mlp *net, const lbf_slbfgs_params *prm, float *d_params, const float *d_X,
                     const float *d_Y, long long N, lbf_record *rec, lbf_solve_info *info) {
  return guard([&] {
    LBF_REQUIRE(net && prm, "null argument");
    net->ctx->c.set_device();
    SlbfgsSolver s(net->net.get(), *prm, d_params, d_X, d_Y, N, read_switches());
    s.run(rec);
    s.info(info);
  });
}

struct lbf_slbfgs {
  std::unique_ptr<SlbfgsSolver> s;
};

int lbf_slbfgs_begin(lbf_mlp *net, const lbf_slbfgs_params *prm, float *d_params, const float *d_X,
                     const float *d_Y, long long N, lbf_slbfgs **out) {
  return guard([&] {
    LBF_REQUIRE(net && prm && out, "null argument");
    net->ctx->c.set_device();
    auto h = std::make_unique<lbf_slbfgs>();
    h->s.reset(new SlbfgsSolver(net->net.get(), *prm, d_params, d_X, d_Y, N, read_switches()));
    *out = h.release();
  });
}

int lbf_slbfgs_iterate(lbf_slbfgs *s, int epochs, lbf_record *rec, lbf_solve_info *info) {
  return guard([&] {
    LBF_REQUIRE(s && epochs >= 0, "bad argument");
    s->s->iterate(epochs, rec);
    s->s->info(info);
  });
}

int lbf_slbfgs_pair0(lbf_slbfgs *s, float *d_wt, float *d_u, float *d_s, float *d_y) {
  return guard([&] {
    LBF_REQUIRE(s, "null argument");
    LBF_REQUIRE(s->s->pair0(d_wt, d_u, d_s, d_y), "no curvature-pair candidate traced (pair_trace off, or none yet)");
  });
}

int lbf_slbfgs_pair_io(lbf_slbfgs *s, int cap, float *d_rec, const float *d_force) {
  return guard([&] {
    LBF_REQUIRE(s && cap >= 0, "bad argument");
    s->s->pair_io(cap, d_rec, d_force);
  });
}

int lbf_slbfgs_end(lbf_slbfgs *s) {
  return guard([&] { delete s; });
}

int lbf_prof_enable(lbf_ctx *ctx, int on) {
  return guard([&] {
    LBF_REQUIRE(ctx, "ctx");
    ctx->c.prof.resolve();
    ctx->c.prof.on = on != 0;
    if (on) {
      ctx->c.prof.ms.clear();
      ctx->c.prof.cnt.clear();
      ctx->c.prof.work.clear();
    }
  });
}

int lbf_prof_select(lbf_ctx *ctx, int section_id) {
  return guard([&] {
    LBF_REQUIRE(ctx, "ctx");
    ctx->c.prof.only = section_id < 0 ? -1 : section_id;
  });
}

int lbf_prof_sample(lbf_ctx *ctx, int every) {
  return guard([&] {
    LBF_REQUIRE(ctx && every >= 1, "ctx / every >= 1");
    ctx->c.prof.every = every;
    ctx->c.prof.seen = 0;
  });
}

int lbf_prof_read(lbf_ctx *ctx, int cap, int *ids, double *ms, long long *counts, int *n_out) {
  return guard([&] {
    LBF_REQUIRE(ctx && n_out, "null argument");
    ctx->c.set_device();
    ctx->c.prof.resolve();
    prof_read(ctx, ctx->c.prof.ms, cap, ids, ms, counts, n_out);
  });
}

int lbf_prof_read_work(lbf_ctx *ctx, int cap, int *ids, double *work, int *n_out) {
  return guard([&] {
    LBF_REQUIRE(ctx && n_out, "null argument");
    ctx->c.set_device();
    ctx->c.prof.resolve();
    prof_read(ctx, ctx->c.prof.work, cap, ids, work, nullptr, n_out);
  });
}

int lbf_synth_mnist(long long N, int In, int classes, unsigned seed, float *h_X, float *h_Y) {
  return guard([&] {
    LBF_REQUIRE(N >= 0 && In > 0 && classes > 0 && h_X && h_Y, "bad argument");
    synth_mnist_host(N, In, classes, seed, h_X, h_Y);
  });
}

int lbf_synth_regression(lbf_ctx *ctx, long long row0, long long N, int In, unsigned seed_x, unsigned seed_t,
                         float *d_X, float *d_Y) {
  return guard([&] {
    LBF_REQUIRE(ctx && row0 >= 0 && N >= 0 && In > 0 && d_X && d_Y, "bad argument");
    ctx->c.set_device();
    synth_regression(ctx->c.stream, row0, N, In, seed_x, seed_t, d_X, d_Y);
    LBF_HIP(hipStreamSynchronize(ctx->c.stream));
  });
}

int lbf_idx_read_images(const char *path, long long max_images, float *h_out, long long *count, int *rows,
                        int *cols) {
  return guard([&] { idx_read_images(path, max_images, h_out, count, rows, cols); });
}

int lbf_idx_read_labels(const char *path, long long max_labels, int classes, float *h_onehot, long long *count) {
  return guard([&] { idx_read_labels(path, max_labels, classes, h_onehot, count); });
}

int lbf_sample_indices(long long N, int b, unsigned seed, int calls, long long *h_out) {
  return guard([&] {
    LBF_REQUIRE(N >= 0 && b >= 0 && calls >= 0 && h_out, "bad argument");
    std::mt19937 rng(seed);
    MinibatchSampler smp{size_t(N)}; // one permutation for every call, like the solver's
    std::vector<int> v;
    for (int c = 0; c < calls; ++c) {
      v.clear();
      smp.draw(size_t(b), rng, v);
      for (size_t i = 0; i < v.size(); ++i) h_out[size_t(c) * b + i] = (long long)v[i];
    }
  });
}

} // extern "C"
