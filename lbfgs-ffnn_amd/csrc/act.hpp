// Activation functions (src/layer.hpp:16-47 forward; derivatives through the post-activation value y,
// src/cuda/kernels.cuh:109-133, equal to the CPU path's act'(Z) in exact arithmetic).
//
// act_c / dact_c take the activation as a template constant; with_act() switches ONCE on the
// (wave-uniform) runtime code and runs a body instantiated per activation, so element loops carry no
// per-element branch tree (a scalar branch per element costs an instruction-fetch redirect each,
// which dominated the GEMM epilogues when the switch sat inside them).
#pragma once

#include "kernels.hpp"

#include <hip/hip_runtime.h>

#include <type_traits>

namespace lbf {

// The rectifiers with curvature. All three are strictly increasing, so y determines x and act'
// through y is exact: leaky ReLU (slope 0.01) [y > 0] + 0.01 [y <= 0]; ELU (alpha 1) y + 1 for y <= 0; softplus
// 1 - e^-y. The forms below are the cancellation-safe ones: expm1f keeps ELU's small negative outputs and
// softplus' small derivatives (1 - expf(-y) is 0 or off by its whole value once y < 6e-8), and
// max(x, 0) + log1pf(expf(-|x|)) neither overflows at x > 88 nor returns 0 below x = -17.
constexpr float LEAKY_SLOPE = 0.01f;

template <int A> __device__ __forceinline__ float act_c(float x) {
  if constexpr (A == ACT_TANH) return tanhf(x);
  else if constexpr (A == ACT_RELU) return x > 0.0f ? x : 0.0f;
  else if constexpr (A == ACT_SIGMOID) return 1.0f / (1.0f + expf(-x));
  else if constexpr (A == ACT_LEAKY_RELU) return x > 0.0f ? x : LEAKY_SLOPE * x;
  else if constexpr (A == ACT_ELU) return x > 0.0f ? x : expm1f(x);
  else if constexpr (A == ACT_SOFTPLUS) return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x)));
  else return x;
}
template <int A> __device__ __forceinline__ float dact_c(float y) {
  if constexpr (A == ACT_TANH) return 1.0f - y * y;
  else if constexpr (A == ACT_RELU) return y > 0.0f ? 1.0f : 0.0f;
  else if constexpr (A == ACT_SIGMOID) return y * (1.0f - y);
  else if constexpr (A == ACT_LEAKY_RELU) return y > 0.0f ? 1.0f : LEAKY_SLOPE;
  else if constexpr (A == ACT_ELU) return y > 0.0f ? 1.0f : y + 1.0f;
  else if constexpr (A == ACT_SOFTPLUS) return -expm1f(-y);
  else return 1.0f;
}

template <class F> __device__ __forceinline__ void with_act(int a, F &&f) {
  switch (a) {
  case ACT_TANH: f(std::integral_constant<int, ACT_TANH>{}); break;
  case ACT_RELU: f(std::integral_constant<int, ACT_RELU>{}); break;
  case ACT_SIGMOID: f(std::integral_constant<int, ACT_SIGMOID>{}); break;
  case ACT_LEAKY_RELU: f(std::integral_constant<int, ACT_LEAKY_RELU>{}); break;
  case ACT_ELU: f(std::integral_constant<int, ACT_ELU>{}); break;
  case ACT_SOFTPLUS: f(std::integral_constant<int, ACT_SOFTPLUS>{}); break;
  default: f(std::integral_constant<int, ACT_LINEAR>{}); break;
  }
}

// The four bodies of the reference's activations. Register allocation is per kernel, so the transcendental bodies
// of ELU and softplus cost a kernel registers, scratch or occupancy on every activation's path. Each
// kernel that applies an activation therefore exists twice: an instance with these four bodies, the code it was
// before the rectifiers, and one with all seven (with_act) that the launcher picks when a rectifier is involved.
// The fused output-layer kernels (EPI_HEAD / EPI_HEAD_XENT, headc::tile, head.hip) have the four-body instance
// only: a network with a rectifier on its last or last hidden layer takes the unfused output route
// (Mlp::head_route).
template <class F> __device__ __forceinline__ void with_act4(int a, F &&f) {
  switch (a) {
  case ACT_TANH: f(std::integral_constant<int, ACT_TANH>{}); break;
  case ACT_RELU: f(std::integral_constant<int, ACT_RELU>{}); break;
  case ACT_SIGMOID: f(std::integral_constant<int, ACT_SIGMOID>{}); break;
  default: f(std::integral_constant<int, ACT_LINEAR>{}); break;
  }
}

// Runtime-coded forms for scalar (non-loop) uses. The *4 forms are the four-body ones of kernels instantiated
// without the rectifiers (with_act4's rule).
__device__ __forceinline__ float act_rt(int a, float x) {
  switch (a) {
  case ACT_TANH: return act_c<ACT_TANH>(x);
  case ACT_RELU: return act_c<ACT_RELU>(x);
  case ACT_SIGMOID: return act_c<ACT_SIGMOID>(x);
  case ACT_LEAKY_RELU: return act_c<ACT_LEAKY_RELU>(x);
  case ACT_ELU: return act_c<ACT_ELU>(x);
  case ACT_SOFTPLUS: return act_c<ACT_SOFTPLUS>(x);
  default: return x;
  }
}
__device__ __forceinline__ float dact_rt(int a, float y) {
  switch (a) {
  case ACT_TANH: return dact_c<ACT_TANH>(y);
  case ACT_RELU: return dact_c<ACT_RELU>(y);
  case ACT_SIGMOID: return dact_c<ACT_SIGMOID>(y);
  case ACT_LEAKY_RELU: return dact_c<ACT_LEAKY_RELU>(y);
  case ACT_ELU: return dact_c<ACT_ELU>(y);
  case ACT_SOFTPLUS: return dact_c<ACT_SOFTPLUS>(y);
  default: return 1.0f;
  }
}

__device__ __forceinline__ float act_rt4(int a, float x) {
  switch (a) {
  case ACT_TANH: return act_c<ACT_TANH>(x);
  case ACT_RELU: return act_c<ACT_RELU>(x);
  case ACT_SIGMOID: return act_c<ACT_SIGMOID>(x);
  default: return x;
  }
}
__device__ __forceinline__ float dact_rt4(int a, float y) {
  switch (a) {
  case ACT_TANH: return dact_c<ACT_TANH>(y);
  case ACT_RELU: return dact_c<ACT_RELU>(y);
  case ACT_SIGMOID: return dact_c<ACT_SIGMOID>(y);
  default: return 1.0f;
  }
}

} // namespace lbf
