// tests/host/fake_lbf_abi_v2.hpp — what the second recording fake (fake_lbf_abi_v2.cpp) shows its harness: the calls
// of the entry points that fake_lbf_abi.cpp deliberately leaves out, in a log of their own.
#pragma once

#include "fake_lbf_abi.hpp"

namespace fake2 {

/// One logged call: fake::Call (fn without its lbf_ prefix; hf, the pointers, the row counts and the record as
/// there) and what only these entry points have.
struct Call : fake::Call {
  lbf_hf_precond precond{};
  bool has_precond = false; // lbf_hf_solve_pc got a non-null lbf_hf_precond
  lbf_adam_params adam{};
  double scale = -1.0;             // lbf_mlp_grad_sq's
  bool trace_nan_on_entry = false; // every one of the trace_cap entries of loss_trace was NaN on entry
};

struct State {
  std::vector<Call> log;
  int trace_to_write = 0; // lbf_adam_solve writes min(trace_to_write, trace_cap) entries: 400 + i
};

State &state();
const Call *last(const std::string &fn);
int count(const std::string &fn);

} // namespace fake2
