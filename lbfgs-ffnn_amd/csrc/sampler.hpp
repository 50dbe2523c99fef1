// Minibatch index sampling of S-LBFGS (host only, no HIP: the sanitizer harness links it with g++).
#pragma once

#include <cstddef>
#include <random>
#include <vector>

namespace lbf {

// libstdc++ partial Fisher-Yates (s_lbfgs.hpp:141-160) over a reusable identity permutation of N: a draw
// swaps b positions, reads them, and swaps them back (O(b) per minibatch instead of the reference's iota(N),
// which cost ~15 ms of host time per cfg-4 epoch); the draws and results are the reference's.
class MinibatchSampler {
 public:
  explicit MinibatchSampler(size_t N);
  // appends the minibatch (min(b, N) indices) to out; returns how many
  size_t draw(size_t b, std::mt19937 &rng, std::vector<int> &out);

 private:
  std::vector<size_t> perm_, touched_;
};
// One draw with a fresh sampler (the ABI helper).
std::vector<size_t> sample_minibatch(size_t N, size_t b, std::mt19937 &rng);

// Rank rk's share of a batch of `total` positions split over nr ranks: [a0, a1) = [total rk / nr, total (rk + 1) / nr).
// The one definition of the sliced split (S-LBFGS LBF_SLBFGS_DP_SLICED, Adam); a share may be empty.
inline void rank_slice(long long total, int rk, int nr, long long *a0, long long *a1) {
  *a0 = total * rk / nr;
  *a1 = total * (rk + 1) / nr;
}

// An epoch's order of the Adam solver: out[0 .. N) = the identity, then Fisher-Yates downward, for i = N - 1 .. 1:
// j = (uint64(rng()) * (i + 1)) >> 32, swap out[i], out[j]. Raw 32-bit draws and no uniform_int_distribution, so the
// order is a function of the mt19937 stream alone, whatever the standard library; j is uniform up to a bias of at
// most N / 2^32. One draw per position: successive epochs continue one stream.
void epoch_order(std::mt19937 &rng, long long N, int *out);

} // namespace lbf
