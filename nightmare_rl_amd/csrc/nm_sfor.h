// nm_sfor.h - sfor<N>(f): f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), the compile-time loop the register-resident
// networks are written in (nm_ppo.hip, nm_rollout.h): the index is a constant inside the body, so register arrays stay registers.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

template <int N, class F, int... Is> __device__ __forceinline__ void sfor_impl(F&& f, std::integer_sequence<int, Is...>) { (f(std::integral_constant<int, Is>{}), ...); }
template <int N, class F> __device__ __forceinline__ void sfor(F&& f) { sfor_impl<N>(f, std::make_integer_sequence<int, N>{}); }
