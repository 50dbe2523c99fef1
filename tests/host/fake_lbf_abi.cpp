// tests/host/fake_lbf_abi.cpp — a host-only, recording implementation of exactly the lbf_* functions that
// include/lbfgs_amd/hip_backend.hpp calls, so the header runs on a CPU (tests/test_dropin_host.py). "Device"
// memory is host memory; every solver logs what it was given (fake_lbf_abi.hpp), writes a known number of
// rows into the record and returns. The *_default_params write the defaults that lbfgs_amd.h documents.
// lbf_idx_read_* forward to the engine's own reader (lbfgs-ffnn_amd/csrc/idx.cpp, host code, linked in).
#include "fake_lbf_abi.hpp"

#include <cstdlib>
#include <cstring>
#include <stdexcept>

struct lbf_ctx {
  int device;
};
struct lbf_mlp {
  lbf_ctx *ctx;
  std::vector<int> dims, acts;
  int loss = LBF_LOSS_MSE;
  double l2 = 0.0;
  long long nparams = 0;
};

namespace lbf { // lbfgs-ffnn_amd/csrc/host_rng.hpp; they throw lbf::Error, a std::runtime_error
void idx_read_images(const char *path, long long max_images, float *h_out, long long *count, int *rows, int *cols);
void idx_read_labels(const char *path, long long max_labels, int classes, float *h_onehot, long long *count);
} // namespace lbf

namespace fake {
State &state() {
  static State s;
  return s;
}
const Call *last(const std::string &fn) {
  auto &l = state().log;
  for (auto it = l.rbegin(); it != l.rend(); ++it)
    if (it->fn == fn) return &*it;
  return nullptr;
}
int count(const std::string &fn) {
  int c = 0;
  for (auto &e : state().log) c += e.fn == fn;
  return c;
}
} // namespace fake

namespace {
thread_local std::string g_err = "";

fake::Call &log_call(const char *fn, const lbf_mlp *net) {
  auto &s = fake::state();
  s.log.emplace_back();
  fake::Call &c = s.log.back();
  c.fn = fn;
  c.net = net;
  if (net) {
    c.ctx = net->ctx;
    c.net_loss = net->loss;
    c.net_l2 = net->l2;
  }
  return c;
}

void log_rec(fake::Call &c, const lbf_record *rec, const lbf_solve_info *info) {
  c.rec = rec;
  c.info = info;
  if (rec) {
    c.rec_loss = rec->loss;
    c.rec_grad_norm = rec->grad_norm;
    c.rec_time_ms = rec->time_ms;
    c.rec_alpha = rec->alpha;
    c.rec_ls_trials = rec->ls_trials;
    c.rec_accepted = rec->accepted;
    c.rec_cap = rec->cap;
    c.rec_size_in = rec->size;
  }
}

// What every solver does after logging: rows into the record (never past cap), the iteration count.
void finish(lbf_record *rec, lbf_solve_info *info) {
  auto &s = fake::state();
  if (rec) {
    const int rows = s.rows_to_write < rec->cap ? s.rows_to_write : rec->cap;
    for (int i = 0; i < rows; ++i) {
      if (rec->loss) rec->loss[i] = 100.0 + i;
      if (rec->grad_norm) rec->grad_norm[i] = 200.0 + i;
      if (rec->time_ms) rec->time_ms[i] = 300.0 + i;
    }
    rec->size = rows;
  }
  if (info) {
    *info = lbf_solve_info{};
    info->iterations = s.iterations;
  }
}

int fail(const char *msg) {
  g_err = msg;
  return LBF_ERR_INVALID;
}
} // namespace

extern "C" {

const char *lbf_last_error(void) { return g_err.c_str(); }

int lbf_ctx_create(int device, void *, lbf_ctx **out) {
  *out = new lbf_ctx{device};
  ++fake::state().live_ctxs;
  return LBF_OK;
}
int lbf_ctx_destroy(lbf_ctx *ctx) {
  if (ctx) --fake::state().live_ctxs;
  delete ctx;
  return LBF_OK;
}
int lbf_ctx_sync(lbf_ctx *ctx) {
  log_call("ctx_sync", nullptr).ctx = ctx;
  return LBF_OK;
}
int lbf_comm_unique_id(char out[128]) {
  for (int i = 0; i < 128; ++i) out[i] = char(i);
  return LBF_OK;
}
int lbf_comm_init(lbf_ctx *, int, int, const char *) { return fail("the fake has no communicator"); }

int lbf_device_alloc(lbf_ctx *ctx, size_t bytes, void **out) {
  if (!ctx || !out) return fail("lbf_device_alloc: null argument");
  *out = std::malloc(bytes ? bytes : 1);
  ++fake::state().live_allocs;
  ++fake::state().total_allocs;
  return LBF_OK;
}
int lbf_device_free(lbf_ctx *, void *p) {
  if (p) --fake::state().live_allocs;
  std::free(p);
  return LBF_OK;
}
int lbf_memcpy(lbf_ctx *ctx, void *dst, const void *src, size_t bytes, int kind) {
  if (!ctx || kind < 0 || kind > 2) return fail("lbf_memcpy: bad argument");
  if (bytes) std::memcpy(dst, src, bytes);
  return LBF_OK;
}

int lbf_mlp_create(lbf_ctx *ctx, int nlayers, const int *dims, const int *acts, lbf_mlp **out) {
  if (!ctx || nlayers < 1 || !dims || !acts || !out) return fail("lbf_mlp_create: bad argument");
  auto *n = new lbf_mlp();
  n->ctx = ctx;
  n->dims.assign(dims, dims + nlayers + 1);
  n->acts.assign(acts, acts + nlayers);
  for (int l = 0; l < nlayers; ++l) n->nparams += (long long)(dims[l] + 1) * dims[l + 1];
  fake::Call &c = log_call("mlp_create", n);
  c.dims = n->dims;
  c.acts = n->acts;
  ++fake::state().live_nets;
  *out = n;
  return LBF_OK;
}
int lbf_mlp_destroy(lbf_mlp *net) {
  if (net) --fake::state().live_nets;
  delete net;
  return LBF_OK;
}
long long lbf_mlp_param_count(const lbf_mlp *net) { return net ? net->nparams : 0; }
int lbf_mlp_init_params(lbf_mlp *net, unsigned seed, int init_mode, float *d_params) {
  if (!net || !d_params) return fail("lbf_mlp_init_params: null argument");
  fake::Call &c = log_call("mlp_init_params", net);
  c.seed = seed;
  c.init_mode = init_mode;
  c.params = d_params;
  for (long long i = 0; i < net->nparams; ++i) d_params[i] = float(seed) + float(i); // every element is written
  return LBF_OK;
}
int lbf_mlp_set_loss(lbf_mlp *net, int loss) {
  if (!net || (loss != LBF_LOSS_MSE && loss != LBF_LOSS_SOFTMAX_XENT)) return fail("lbf_mlp_set_loss: bad argument");
  log_call("mlp_set_loss", net).ivalue = loss;
  net->loss = loss;
  return LBF_OK;
}
int lbf_mlp_set_l2(lbf_mlp *net, double l2) {
  if (!net || !(l2 >= 0.0) || l2 > 1.7976931348623157e308) return fail("lbf_mlp_set_l2: l2 < 0 or non-finite");
  log_call("mlp_set_l2", net).value = l2;
  net->l2 = l2;
  return LBF_OK;
}
int lbf_mlp_forward(lbf_mlp *net, const float *d_params, const float *d_X, long long batch, float *d_out) {
  if (!net || !d_params || !d_out) return fail("lbf_mlp_forward: null argument");
  fake::Call &c = log_call("mlp_forward", net);
  c.params = d_params;
  c.X = d_X;
  c.batch = batch;
  c.out = d_out;
  const size_t want = size_t(batch) * size_t(net->dims.back());
  auto it = fake::state().forward_tables.find(batch);
  if (it == fake::state().forward_tables.end() || it->second.size() != want)
    return fail("lbf_mlp_forward: the harness installed no output table for this batch");
  std::memcpy(d_out, it->second.data(), want * sizeof(float));
  return LBF_OK;
}
int lbf_mlp_loss_grad(lbf_mlp *net, const float *d_params, float *d_grad, const float *d_X, const float *d_Y,
                      const int *d_idx, long long batch, double inv_scale, double l2, double *h_loss) {
  if (!net || !d_params || !d_grad || !h_loss) return fail("lbf_mlp_loss_grad: null argument");
  fake::Call &c = log_call("mlp_loss_grad", net);
  c.params = d_params;
  c.grad = d_grad;
  c.X = d_X;
  c.Y = d_Y;
  c.idx = d_idx;
  c.batch = batch;
  c.inv_scale = inv_scale;
  c.l2_arg = l2;
  for (long long i = 0; i < net->nparams; ++i) d_grad[i] = float(i) * 0.5f;
  *h_loss = fake::state().loss_grad_value;
  return LBF_OK;
}
int lbf_mlp_evaluate(lbf_mlp *net, const float *d_params, const float *d_X, const float *d_Y, const int *d_idx,
                     long long batch, double inv_scale, int k, long long chunk_rows, lbf_eval_result *h_res,
                     long long *h_confusion, int *d_pred, float *d_proba) {
  if (!net || !d_params || !h_res) return fail("lbf_mlp_evaluate: null argument");
  const int out = net->dims.back();
  if (k < 1 || k > out) return fail("lbf_mlp_evaluate: k outside 1..Out");
  fake::Call &c = log_call("mlp_evaluate", net);
  c.params = d_params;
  c.X = d_X;
  c.Y = d_Y;
  c.idx = d_idx;
  c.batch = batch;
  c.inv_scale = inv_scale;
  c.k = k;
  c.chunk_rows = chunk_rows;
  c.h_res = h_res;
  c.confusion = h_confusion;
  c.pred = d_pred;
  c.proba = d_proba;
  if (h_confusion) { // all Out * Out entries are read, then written: a short buffer shows under AddressSanitizer
    c.confusion_zeroed = true;
    for (int i = 0; i < out * out; ++i) {
      if (h_confusion[i] != 0) c.confusion_zeroed = false;
      h_confusion[i] = i + 1;
    }
  }
  if (d_pred)
    for (long long i = 0; i < batch; ++i) d_pred[i] = int(i % out);
  *h_res = fake::state().eval;
  h_res->k = k;
  return LBF_OK;
}

/* ---- defaults: the values lbfgs_amd.h documents next to each field ---- */
void lbf_lbfgs_default_params(lbf_lbfgs_params *p, int line_search) {
  const bool armijo = line_search == LBF_LS_ARMIJO;
  p->m = 16;
  p->max_iters = armijo ? 200 : 1000;
  p->tol = armijo ? 1e-6 : 1e-10;
  p->line_search = line_search;
  p->max_line_iters = armijo ? 20 : 50;
  p->c1 = 1e-4;
  p->c2 = 0.9;
  p->rho = 0.5;
}
void lbf_slbfgs_default_params(lbf_slbfgs_params *p) {
  std::memset(p, 0, sizeof(*p));
  p->max_epochs = 1000;
  p->tol = 1e-4;
  p->M = 10;
  p->L = 10;
  p->b = 128;
  p->b_H = 64;
  p->step = 0.01;
  p->lambda = 1e-4;
  p->seed = 123;
  p->fd_eps = 1e-4;
  p->hvp_exact = LBF_HVP_FD;
  p->dp_mode = LBF_SLBFGS_DP_REPLICATED;
}
void lbf_gd_default_params(lbf_gd_params *p) {
  p->lr = 0.01;
  p->momentum = 0.9;
  p->max_iters = 200;
  p->tol = 1e-6;
}
void lbf_sgd_default_params(lbf_sgd_params *p) {
  p->lr = 0.01;
  p->momentum = 0.9;
  p->batch = 64;
  p->decay_rate = 1.0;
  p->decay_step = 0;
  p->max_epochs = 200;
  p->tol = 1e-6;
}
void lbf_hf_default_params(lbf_hf_params *p) {
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
void lbf_owlqn_default_params(lbf_owlqn_params *p) {
  std::memset(p, 0, sizeof(*p));
  p->m = 10;
  p->max_iters = 100;
  p->tol = 1e-6;
  p->c1 = 1e-4;
  p->rho = 0.5;
  p->max_line_iters = 20;
}

/* ---- solvers: log, write rows, return ---- */
static void log_net_solve(fake::Call &c, const float *d_params, const float *d_X, const float *d_Y,
                          long long n_local, long long n_global, const lbf_record *rec, const lbf_solve_info *info) {
  c.params = d_params;
  c.X = d_X;
  c.Y = d_Y;
  c.n_local = n_local;
  c.n_global = n_global;
  log_rec(c, rec, info);
}

int lbf_lbfgs_solve(lbf_mlp *net, const lbf_lbfgs_params *prm, float *d_params, const float *d_X, const float *d_Y,
                    long long n_local, long long n_global, lbf_record *rec, lbf_solve_info *info) {
  if (!net || !prm) return fail("lbf_lbfgs_solve: null argument");
  fake::Call &c = log_call("lbfgs_solve", net);
  c.lbfgs = *prm;
  log_net_solve(c, d_params, d_X, d_Y, n_local, n_global, rec, info);
  finish(rec, info);
  return LBF_OK;
}
int lbf_lbfgs_solve_fn(lbf_ctx *ctx, const lbf_lbfgs_params *prm, long long n, float *d_params, lbf_loss_grad_fn fn,
                       void *user, lbf_record *rec, lbf_solve_info *info) {
  if (!ctx || !prm || !fn) return fail("lbf_lbfgs_solve_fn: null argument");
  std::vector<float> grad(size_t(n > 0 ? n : 0));
  const double v = fn(user, d_params, grad.data()); // one trial, at the caller's own point
  fake::Call &c = log_call("lbfgs_solve_fn", nullptr);
  c.ctx = ctx;
  c.lbfgs = *prm;
  c.n = n;
  c.params = d_params;
  c.user = user;
  c.value = v;
  log_rec(c, rec, info);
  finish(rec, info);
  return LBF_OK;
}
int lbf_slbfgs_solve(lbf_mlp *net, const lbf_slbfgs_params *prm, float *d_params, const float *d_X, const float *d_Y,
                     long long N, lbf_record *rec, lbf_solve_info *info) {
  if (!net || !prm) return fail("lbf_slbfgs_solve: null argument");
  fake::Call &c = log_call("slbfgs_solve", net);
  c.slbfgs = *prm;
  log_net_solve(c, d_params, d_X, d_Y, N, N, rec, info);
  finish(rec, info);
  return LBF_OK;
}
int lbf_gd_solve(lbf_mlp *net, const lbf_gd_params *prm, float *d_params, const float *d_X, const float *d_Y,
                 long long n_local, long long n_global, lbf_record *rec, lbf_solve_info *info) {
  if (!net || !prm) return fail("lbf_gd_solve: null argument");
  fake::Call &c = log_call("gd_solve", net);
  c.gd = *prm;
  log_net_solve(c, d_params, d_X, d_Y, n_local, n_global, rec, info);
  finish(rec, info);
  return LBF_OK;
}
int lbf_sgd_solve(lbf_mlp *net, const lbf_sgd_params *prm, float *d_params, const float *d_X, const float *d_Y,
                  long long N, lbf_record *rec, lbf_solve_info *info) {
  if (!net || !prm) return fail("lbf_sgd_solve: null argument");
  fake::Call &c = log_call("sgd_solve", net);
  c.sgd = *prm;
  log_net_solve(c, d_params, d_X, d_Y, N, N, rec, info);
  finish(rec, info);
  return LBF_OK;
}
int lbf_hf_solve(lbf_mlp *net, const lbf_hf_params *prm, float *d_params, const float *d_X, const float *d_Y,
                 long long n_local, long long n_global, lbf_record *rec, lbf_solve_info *info) {
  if (!net || !prm) return fail("lbf_hf_solve: null argument");
  fake::Call &c = log_call("hf_solve", net);
  c.hf = *prm;
  log_net_solve(c, d_params, d_X, d_Y, n_local, n_global, rec, info);
  finish(rec, info);
  return LBF_OK;
}
int lbf_owlqn_solve(lbf_mlp *net, const lbf_owlqn_params *prm, float *d_params, const float *d_X, const float *d_Y,
                    long long n_local, long long n_global, lbf_record *rec, lbf_solve_info *info,
                    lbf_owlqn_stats *stats) {
  if (!net || !prm) return fail("lbf_owlqn_solve: null argument");
  fake::Call &c = log_call("owlqn_solve", net);
  c.owlqn = *prm;
  c.stats = stats;
  log_net_solve(c, d_params, d_X, d_Y, n_local, n_global, rec, info);
  if (stats) *stats = fake::state().owl;
  finish(rec, info);
  return LBF_OK;
}

int lbf_idx_read_images(const char *path, long long max_images, float *h_out, long long *count, int *rows,
                        int *cols) {
  try {
    lbf::idx_read_images(path, max_images, h_out, count, rows, cols);
  } catch (const std::runtime_error &e) {
    return fail(e.what());
  }
  return LBF_OK;
}
int lbf_idx_read_labels(const char *path, long long max_labels, int classes, float *h_onehot, long long *count) {
  try {
    lbf::idx_read_labels(path, max_labels, classes, h_onehot, count);
  } catch (const std::runtime_error &e) {
    return fail(e.what());
  }
  return LBF_OK;
}

} // extern "C"
