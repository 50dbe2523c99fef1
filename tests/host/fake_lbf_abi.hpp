// tests/host/fake_lbf_abi.hpp — what the recording fake of the C ABI (fake_lbf_abi.cpp) shows the harness.
#pragma once

#include "lbfgs_amd.h"

#include <map>
#include <string>
#include <vector>

namespace fake {

/// One logged call. `fn` is the ABI function without its lbf_ prefix; only the fields that function has are set.
struct Call {
  std::string fn;
  // the parameter struct of a solver, copied whole
  lbf_lbfgs_params lbfgs{};
  lbf_slbfgs_params slbfgs{};
  lbf_gd_params gd{};
  lbf_sgd_params sgd{};
  lbf_hf_params hf{};
  lbf_owlqn_params owlqn{};
  // handles and pointers, as given
  const void *ctx = nullptr, *net = nullptr, *params = nullptr, *grad = nullptr, *X = nullptr, *Y = nullptr,
             *idx = nullptr, *out = nullptr, *rec = nullptr, *info = nullptr, *stats = nullptr, *user = nullptr,
             *confusion = nullptr, *pred = nullptr, *proba = nullptr, *h_res = nullptr;
  const double *rec_loss = nullptr, *rec_grad_norm = nullptr, *rec_time_ms = nullptr;
  const void *rec_alpha = nullptr, *rec_ls_trials = nullptr, *rec_accepted = nullptr;
  int rec_cap = -1, rec_size_in = -1;
  long long n = -1, n_local = -1, n_global = -1, batch = -1, chunk_rows = -1;
  double inv_scale = -1.0, l2_arg = -1.0, value = 0.0; // value: set_l2's argument / what the callback returned
  int k = -1, ivalue = -1, init_mode = -1;             // ivalue: set_loss's argument
  unsigned seed = 0;
  bool confusion_zeroed = false; // every one of the Out * Out entries was 0 on entry
  // the network's state when the call was made
  int net_loss = -1;
  double net_l2 = -1.0;
  std::vector<int> dims, acts; // mlp_create
};

struct State {
  std::vector<Call> log;
  long long live_allocs = 0, total_allocs = 0, live_nets = 0, live_ctxs = 0;
  std::map<long long, std::vector<float>> forward_tables; // batch -> batch * Out outputs that lbf_mlp_forward writes
  int rows_to_write = 0;  // a solver writes min(rows_to_write, rec->cap) rows: loss 100 + i, gnorm 200 + i, ms 300 + i
  int iterations = 0;     // info->iterations of every solver
  lbf_eval_result eval{}; // what lbf_mlp_evaluate returns (k is the caller's)
  lbf_owlqn_stats owl{};  // what lbf_owlqn_solve writes into stats
  double loss_grad_value = 0.0;
};

State &state();

/// The last logged call of that function, or nullptr.
const Call *last(const std::string &fn);
/// How many calls of that function are logged.
int count(const std::string &fn);

} // namespace fake
