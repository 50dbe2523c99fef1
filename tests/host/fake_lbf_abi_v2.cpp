// tests/host/fake_lbf_abi_v2.cpp — recording fakes of only the entry points that fake_lbf_abi.cpp leaves out:
// lbf_hf_precond_default, lbf_hf_solve_pc, lbf_mlp_grad_sq, lbf_adam_default_params and lbf_adam_solve. Linked next
// to fake_lbf_abi.cpp into dropin_harness_v2 only, so dropin_harness keeps proving that the classes of the earlier
// ABI link without them. Same conventions: log the call, copy the structs, write min(rows_to_write, cap) record
// rows (fake::state()) and min(trace_to_write, trace_cap) trace entries, return.
#include "fake_lbf_abi_v2.hpp"

#include <cmath>
#include <cstring>

namespace fake2 {
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
} // namespace fake2

namespace {
fake2::Call &log_solve(const char *fn, const lbf_mlp *net, const float *d_params, const float *d_X, const float *d_Y,
                       long long n_local, long long n_global, const lbf_record *rec, const lbf_solve_info *info) {
  auto &l = fake2::state().log;
  l.emplace_back();
  fake2::Call &c = l.back();
  c.fn = fn;
  c.net = net;
  c.params = d_params;
  c.X = d_X;
  c.Y = d_Y;
  c.n_local = n_local;
  c.n_global = n_global;
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
  return c;
}

// as fake_lbf_abi.cpp's: rows into the record (never past cap), the iteration count
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
} // namespace

extern "C" {

void lbf_hf_precond_default(lbf_hf_precond *p) {
  std::memset(p, 0, sizeof(*p));
  p->mode = LBF_PRECOND_NONE;
  p->exponent = 0.75;
  p->refresh = 1;
}

void lbf_adam_default_params(lbf_adam_params *p) {
  std::memset(p, 0, sizeof(*p));
  p->lr = 1e-3;
  p->beta1 = 0.9;
  p->beta2 = 0.999;
  p->eps = 1e-8;
  p->batch = 128;
  p->shuffle = 1;
  p->seed = 123;
  p->decay_rate = 1.0;
  p->max_epochs = 200;
  p->tol = 1e-6;
}

int lbf_hf_solve_pc(lbf_mlp *net, const lbf_hf_params *prm, const lbf_hf_precond *pc, float *d_params,
                    const float *d_X, const float *d_Y, long long n_local, long long n_global, lbf_record *rec,
                    lbf_solve_info *info) {
  if (!net || !prm) return LBF_ERR_INVALID;
  fake2::Call &c = log_solve("hf_solve_pc", net, d_params, d_X, d_Y, n_local, n_global, rec, info);
  c.hf = *prm;
  c.has_precond = pc != nullptr;
  if (pc) c.precond = *pc;
  finish(rec, info);
  return LBF_OK;
}

int lbf_mlp_grad_sq(lbf_mlp *net, const float *d_params, const float *d_X, const float *d_Y, const int *d_idx,
                    long long batch, double scale, float *d_out) {
  if (!net || !d_params || !d_out) return LBF_ERR_INVALID;
  fake2::Call &c = log_solve("mlp_grad_sq", net, d_params, d_X, d_Y, -1, -1, nullptr, nullptr);
  c.idx = d_idx;
  c.batch = batch;
  c.scale = scale;
  c.out = d_out;
  const long long n = lbf_mlp_param_count(net); // every element is written
  for (long long i = 0; i < n; ++i) d_out[i] = float(i) * 0.25f;
  return LBF_OK;
}

int lbf_adam_solve(lbf_mlp *net, const lbf_adam_params *prm, float *d_params, const float *d_X, const float *d_Y,
                   long long N, lbf_record *rec, lbf_solve_info *info) {
  if (!net || !prm) return LBF_ERR_INVALID;
  fake2::Call &c = log_solve("adam_solve", net, d_params, d_X, d_Y, N, N, rec, info);
  c.adam = *prm;
  if (prm->loss_trace) { // all trace_cap entries are read, then the first ones written: a short buffer shows
    c.trace_nan_on_entry = true;
    for (int i = 0; i < prm->trace_cap; ++i)
      if (!std::isnan(prm->loss_trace[i])) c.trace_nan_on_entry = false;
    const int w = fake2::state().trace_to_write;
    for (int i = 0; i < (w < prm->trace_cap ? w : prm->trace_cap); ++i) prm->loss_trace[i] = 400.0 + i;
  }
  finish(rec, info);
  return LBF_OK;
}

} // extern "C"
