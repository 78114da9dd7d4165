// nm_act.h - the hidden-layer activations of rsl_rl v1.0.2's ActorCritic (`get_activation`: elu, selu, relu, lrelu, tanh, sigmoid; crelu
// is a plain ReLU there; the user's choice is the reference config's `activation = 'elu' # can be elu, relu, selu, crelu, lrelu, tanh,
// sigmoid`, envs/nightmare_v3_config.py:109), written ONCE for every kernel that evaluates the networks: k_mlp_fused / k_linear_mfma
// (nm_policy.hip), k_ppo_fwdbwd / k_ppo_fwdbwd_split / k_ppo_act_fast (nm_ppo.hip) and the wave policy of nm_rollout.h.
//
// Codes: the NM_ACT_* enum of include/nightmare_hip.h (ELU = 0: every call that passes no code means ELU).
// For each code:
//   f<ACT>(z)   the forward value;
//   dfy<ACT>(y) the derivative written FROM THE OUTPUT y = f(z) - the backward kernels keep post-activation values only. Each is torch's
//               own backward formula on the result (threshold_backward, tanh_backward, sigmoid_backward, elu_backward with is_result).
// Both as compile-time templates (register-resident kernels: one instantiation per code, no branch) and as a runtime switch on a
// wave-uniform code (the generic kernels: one scalar branch per epilogue).
//
// Arithmetic: the hardware exponential (__expf = v_exp_f32 of z * log2 e, 1 ulp) and reciprocal (v_rcp_f32, 1 ulp); no libm call in an
// epilogue. Absolute error of each sequence against the exact function, |z| in the range a network produces (the exponent argument's own
// rounding grows with |z|, but the functions saturate there):
//   ELU      z > 0 ? z : e^z - 1                     < 1.2e-7 (e^z in (0, 1]: 1 ulp of 1, then one exact subtraction)
//   SELU     z > 0 ? l z : la (e^z - 1)              < 2.5e-7 (la = 1.758 times the ELU error, one rounding of the product)
//   ReLU     z > 0 ? z : 0                           exact
//   LReLU    z > 0 ? z : 0.01 z                      one rounding (relative 6e-8)
//   tanh     1 - 2 / (e^{2z} + 1)                    < 3e-7; saturates to exactly +-1 at +-inf (rcp(inf) = 0, rcp(1) = 1), no NaN for
//                                                    any finite z. Near 0 the result is a difference of two numbers near 1: absolute,
//                                                    not relative accuracy (|z| < 6e-8 gives 0 or +-1.2e-7).
//   sigmoid  1 / (1 + e^{-z})                        < 1.5e-7; 0 at -inf (rcp(inf)), 1 at +inf
// The derivatives from the output are exact functions of y up to one or two roundings (< 1.2e-7 absolute for y in the ranges above).
//
// Padding: f(0) = 0 for every code except sigmoid (f(0) = 0.5). A padded neuron (bias 0, weights 0) therefore never relies on f(0) = 0
// in these kernels: it is either written as an explicit 0 / bias-carrier 1 after the activation, or read only through packed weights that
// are zero by construction (nm_rollout.h: k_roll_pack), where a finite f(0) contributes exactly 0.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "../../include/nightmare_hip.h"

namespace nmact {

constexpr int kLinear = -1;                                        // no activation (a network's last layer)
constexpr float kSeluScale = 1.0507009873554804934193349852946f;  // torch.nn.SELU
constexpr float kSeluAlpha = 1.6732632423543772848170429916717f;
constexpr float kSeluScaleAlpha = 1.7580993408473766f;                 // scale * alpha, rounded once
constexpr float kLreluSlope = 0.01f;                               // torch.nn.LeakyReLU default negative_slope

__host__ __device__ constexpr bool valid(int act) { return act >= NM_ACT_ELU && act < NM_NUM_ACTIVATIONS; }

template <int ACT> __device__ __forceinline__ float f(float z) {
  static_assert(valid(ACT), "activation code");
  if constexpr (ACT == NM_ACT_ELU) return z > 0.0f ? z : __expf(z) - 1.0f;
  else if constexpr (ACT == NM_ACT_SELU) return z > 0.0f ? kSeluScale * z : kSeluScaleAlpha * (__expf(z) - 1.0f);
  else if constexpr (ACT == NM_ACT_RELU) return z > 0.0f ? z : 0.0f;
  else if constexpr (ACT == NM_ACT_LRELU) return z > 0.0f ? z : kLreluSlope * z;
  else if constexpr (ACT == NM_ACT_TANH) return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * z) + 1.0f);
  else return __builtin_amdgcn_rcpf(1.0f + __expf(-z));
}

template <int ACT> __device__ __forceinline__ float dfy(float y) {
  static_assert(valid(ACT), "activation code");
  if constexpr (ACT == NM_ACT_ELU) return fminf(y + 1.0f, 1.0f);                   // 1 if ELU > 0, else ELU + 1 = e^z (<= 1)
  else if constexpr (ACT == NM_ACT_SELU) return y > 0.0f ? kSeluScale : y + kSeluScaleAlpha;   // y <= 0: la e^z = y + la
  else if constexpr (ACT == NM_ACT_RELU) return y > 0.0f ? 1.0f : 0.0f;
  else if constexpr (ACT == NM_ACT_LRELU) return y > 0.0f ? 1.0f : kLreluSlope;
  else if constexpr (ACT == NM_ACT_TANH) return 1.0f - y * y;
  else return y * (1.0f - y);
}

// runtime forms: `act` is uniform over the wave (a kernel argument), so the switch is a scalar branch
__device__ __forceinline__ float f_rt(int act, float z) {
  switch (act) {
    case NM_ACT_SELU: return f<NM_ACT_SELU>(z);
    case NM_ACT_RELU: return f<NM_ACT_RELU>(z);
    case NM_ACT_LRELU: return f<NM_ACT_LRELU>(z);
    case NM_ACT_TANH: return f<NM_ACT_TANH>(z);
    case NM_ACT_SIGMOID: return f<NM_ACT_SIGMOID>(z);
    default: return f<NM_ACT_ELU>(z);
  }
}
__device__ __forceinline__ float dfy_rt(int act, float y) {
  switch (act) {
    case NM_ACT_SELU: return dfy<NM_ACT_SELU>(y);
    case NM_ACT_RELU: return dfy<NM_ACT_RELU>(y);
    case NM_ACT_LRELU: return dfy<NM_ACT_LRELU>(y);
    case NM_ACT_TANH: return dfy<NM_ACT_TANH>(y);
    case NM_ACT_SIGMOID: return dfy<NM_ACT_SIGMOID>(y);
    default: return dfy<NM_ACT_ELU>(y);
  }
}

// host: call fn(std::integral_constant<int, ACT>{}) for a runtime code (one kernel instantiation per code); the caller validated `act`
template <class F> inline auto dispatch(int act, F&& fn) {
  switch (act) {
    case NM_ACT_SELU: return fn(std::integral_constant<int, NM_ACT_SELU>{});
    case NM_ACT_RELU: return fn(std::integral_constant<int, NM_ACT_RELU>{});
    case NM_ACT_LRELU: return fn(std::integral_constant<int, NM_ACT_LRELU>{});
    case NM_ACT_TANH: return fn(std::integral_constant<int, NM_ACT_TANH>{});
    case NM_ACT_SIGMOID: return fn(std::integral_constant<int, NM_ACT_SIGMOID>{});
    default: return fn(std::integral_constant<int, NM_ACT_ELU>{});
  }
}

}  // namespace nmact
