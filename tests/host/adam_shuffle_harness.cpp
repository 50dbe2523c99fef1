// Stand-alone CPU program over the Adam solver's host-side sampling (lbfgs-ffnn_amd/csrc/sampler.{hpp,cpp}): the epoch
// shuffle and the rank split of a batch. Built by tests/test_adam_host.py with g++ under AddressSanitizer +
// UndefinedBehaviorSanitizer and run as a process of its own; no GPU, nothing loaded into Python.
//   usage: adam_shuffle_harness [N seed epochs]   (with arguments: also prints the orders, one epoch per line)
#include "sampler.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

int g_fail = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "FAILED %s (line %d)\n", #cond, __LINE__);        \
      ++g_fail;                                                              \
    }                                                                        \
  } while (0)

bool is_permutation(const std::vector<int> &o) {
  std::vector<char> seen(o.size(), 0);
  for (int v : o) {
    if (v < 0 || size_t(v) >= o.size() || seen[size_t(v)]) return false;
    seen[size_t(v)] = 1;
  }
  return true;
}

} // namespace

int main(int argc, char **argv) {
  // every size from the smallest on: the buffer is exactly N ints, so a write past it is an ASan report
  for (long long N : {1LL, 2LL, 3LL, 16LL, 37LL, 257LL, 4099LL}) {
    std::mt19937 rng(123u), twin(123u);
    std::vector<int> a(size_t(N), -1), b(size_t(N), -1), c(size_t(N), -1);
    lbf::epoch_order(rng, N, a.data());
    lbf::epoch_order(rng, N, b.data());
    CHECK(is_permutation(a) && is_permutation(b));
    if (N >= 16) CHECK(a != b); // the second epoch continues the stream
    // one draw per position below the top: after two epochs the stream is 2 (N - 1) draws on
    twin.discard(static_cast<unsigned long long>(2 * (N - 1)));
    CHECK(rng() == twin());
    std::mt19937 again(123u);
    lbf::epoch_order(again, N, c.data());
    CHECK(a == c);
  }
  {
    std::mt19937 rng(5u);
    lbf::epoch_order(rng, 0, nullptr); // an empty order touches nothing
    int one = -1;
    lbf::epoch_order(rng, 1, &one);
    CHECK(one == 0);
  }
  // the rank split: consecutive, covering, sizes within one of each other; a one-row batch leaves one rank all of it
  for (long long total : {0LL, 1LL, 5LL, 16LL, 257LL, 2147483647LL})
    for (int nr : {1, 2, 3, 8, 16}) {
      long long prev = 0, lo = total, hi = 0;
      for (int rk = 0; rk < nr; ++rk) {
        long long a0 = -1, a1 = -1;
        lbf::rank_slice(total, rk, nr, &a0, &a1);
        CHECK(a0 == prev && a1 >= a0);
        prev = a1;
        lo = a1 - a0 < lo ? a1 - a0 : lo;
        hi = a1 - a0 > hi ? a1 - a0 : hi;
      }
      CHECK(prev == total && hi - lo <= 1);
    }
  if (argc == 4) {
    const long long N = std::atoll(argv[1]);
    const int epochs = std::atoi(argv[3]);
    std::mt19937 rng(static_cast<unsigned>(std::strtoul(argv[2], nullptr, 10)));
    std::vector<int> o(static_cast<size_t>(N), 0);
    for (int e = 0; e < epochs; ++e) {
      lbf::epoch_order(rng, N, o.data());
      std::printf("order");
      for (int v : o) std::printf(" %d", v);
      std::printf("\n");
    }
  }
  if (g_fail) return 1;
  std::printf("adam shuffle harness ok\n");
  return 0;
}
