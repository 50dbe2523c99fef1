// Host plumbing every solver driver (solve_*.cpp) shares: the lbf_record writer, the solve's evaluation counters
// for lbf_solve_info, the wall clock of a record row and the pinned mirror of the device status block.
// RecordWriter, SolveCounters and ms_since need lbfgs_amd.h and the standard library only, like host_sync.hpp, so
// the sanitizer harness (tests/host/sanitize_harness.cpp, g++) runs RecordWriter on the CPU. StatusMirror is the
// one piece that touches HIP: it exists in the library's translation units, which include internal.hpp first.
#pragma once

#include "../../include/lbfgs_amd.h"

#include <algorithm>
#include <chrono>
#include <cstring>

namespace lbf {

inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Appends rows to a caller's lbf_record (nullable) from its current size on. The row index keeps counting past the
// record's capacity: rows beyond it are dropped, and patch_prev_accepted then finds no row to patch instead of
// patching row cap - 1 for ever after.
class RecordWriter {
public:
  RecordWriter() = default;
  explicit RecordWriter(lbf_record *rec) : rec_(rec), i_(rec ? rec->size : 0) {}
  void retarget(lbf_record *rec) { rec_ = rec; } // go on at the same row index in the record of a later call
  void put(double loss, double gnorm, double ms, double alpha, int trials, int accepted) {
    const int i = i_++;
    if (!rec_ || i >= rec_->cap) return;
    if (rec_->loss) rec_->loss[i] = loss;
    if (rec_->grad_norm) rec_->grad_norm[i] = gnorm;
    if (rec_->time_ms) rec_->time_ms[i] = ms;
    if (rec_->alpha) rec_->alpha[i] = alpha;
    if (rec_->ls_trials) rec_->ls_trials[i] = trials;
    if (rec_->accepted) rec_->accepted[i] = accepted;
    rec_->size = std::max(rec_->size, i + 1);
  }
  // L-BFGS: whether the ring took the last row's pair is only known once the next iteration's history step ran.
  void patch_prev_accepted(int flag) {
    if (rec_ && rec_->accepted && i_ > 0 && i_ - 1 < rec_->cap) rec_->accepted[i_ - 1] = flag;
  }

private:
  lbf_record *rec_ = nullptr;
  int i_ = 0;
};

// The evaluation counters of a network (Mlp) or an Objective when a solve begins; fill() writes a whole
// lbf_solve_info (nullable) with what the solve itself added to them.
template <class Src> class SolveCounters {
public:
  explicit SolveCounters(const Src *src)
      : src_(src), evals_(src->evals()), rows_(src->rows()), lonly_(src->loss_only_evals()),
        gal_(src->grad_after_loss_evals()) {}
  void fill(lbf_solve_info *info, int iterations, double final_loss, double final_grad_norm) const {
    if (!info) return;
    std::memset(info, 0, sizeof(*info));
    info->iterations = iterations;
    info->n_evals = src_->evals() - evals_;
    info->n_rows = src_->rows() - rows_;
    info->n_loss_only = src_->loss_only_evals() - lonly_;
    info->n_grad_after_loss = src_->grad_after_loss_evals() - gal_;
    info->final_loss = final_loss;
    info->final_grad_norm = final_grad_norm;
  }

private:
  const Src *src_;
  long long evals_, rows_, lonly_, gal_;
};

#ifdef LBF_HIP // internal.hpp
// The SC_N doubles of a device status block (kernels.hpp SC_*) in pinned host memory.
class StatusMirror {
public:
  StatusMirror() { h_.ensure(SC_N); }
  void enqueue(hipStream_t s, const double *dev) { // the copy only: valid after the caller's next wait on s
    LBF_HIP(hipMemcpyAsync(h_.get(), dev, SC_N * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  void read(hipStream_t s, const double *dev) {
    enqueue(s, dev);
    LBF_HIP(hipStreamSynchronize(s));
  }
  double operator[](int i) const { return h_.get()[i]; }

private:
  PinnedBuf<double> h_;
};
#endif

} // namespace lbf
