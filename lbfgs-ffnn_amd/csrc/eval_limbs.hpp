// Integer counts through a float sum all-reduce (Mlp::evaluate, metrics.hip). The communicators here carry
// fp32 sums only (comm.hpp), so a count travels as three 16-bit limbs, each stored as a float: a limb is below
// 2^16, the sum of one limb over at most 256 ranks is below 2^24 and therefore exact in fp32 in any order of
// addition, and the merged sum is exact for any total below 2^48 + carries (the merge is done in 64-bit integers,
// so a limb sum above 2^16 simply carries). Plain C++ (no HIP needed on the host side): tests/test_eval_api.py
// compiles it into a stand-alone program.
#pragma once

#if defined(__HIPCC__)
#define LBF_LIMB_HD __host__ __device__
#else
#define LBF_LIMB_HD
#endif

namespace lbf {

constexpr int kEvalLimbs = 3;        // 16-bit limbs per count
constexpr int kEvalMaxRanks = 256;   // 256 * (2^16 - 1) < 2^24
constexpr long long kEvalMaxCount = (1LL << 48) - 1; // per rank

// v < 2^48 -> out[0] (low) .. out[2] (high), each an integer in [0, 65535] held as a float
LBF_LIMB_HD inline void eval_limbs_split(unsigned long long v, float *out) {
  out[0] = float(unsigned(v & 0xFFFFull));
  out[1] = float(unsigned((v >> 16) & 0xFFFFull));
  out[2] = float(unsigned((v >> 32) & 0xFFFFull));
}

// the (summed) limbs back into the integer; every limb an exact integer below 2^24
LBF_LIMB_HD inline long long eval_limbs_merge(const float *in) {
  return (long long)in[0] + ((long long)in[1] << 16) + ((long long)in[2] << 32);
}

} // namespace lbf
