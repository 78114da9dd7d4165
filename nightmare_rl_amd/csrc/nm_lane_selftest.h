// nm_lane_selftest.h - the cross-lane helpers that the lean step kernel takes in another form than the generic kernels (simt.h), each
// next to the form it replaces, on one wave of caller-given values. Written against simt.h like the stages, so the device kernel behind
// nm_lane_selftest() (nm_step_lean.hip) and the host emulation (tests) run the same lines. Not on any path of the product.
//
// Per wave and slot s, out0[s] holds the generic form's lane values and out1[s] the lean form's:
//   s = I, 0 <= I < 32                g + a * (x of lane I of this lane's half-wave): fma_half_lane<I> | fma_half_lane_dpp<I>
//   s = 32 + k, 0 <= k < kLaneMasks   a in the lanes of mask m[k], g elsewhere:       sel_mask         | sel_mask_open
#pragma once
#include <utility>

#include "simt.h"

namespace nm {
using namespace simt;
constexpr int kLaneMasks = 4;
constexpr int kLaneSlots = 32 + kLaneMasks;
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): the lane index of a helper is a template argument
template <class F, int... Is> NM_FN void lane_sfor_impl(F&& f, std::integer_sequence<int, Is...>) { (f(std::integral_constant<int, Is>{}), ...); }
template <int N, class F> NM_FN void lane_sfor(F&& f) { lane_sfor_impl(f, std::make_integer_sequence<int, N>{}); }

template <class real> NM_FN void lane_selftest_wave(const V<real>& x, const V<real>& a, const V<real>& g, const uint64_t* m, V<real>* out0, V<real>* out1) {
  const V<int> lane = lane_id();
  const VB h1 = (lane & 32) != 0;
  lane_sfor<32>([&](auto iT) {
    constexpr int I = decltype(iT)::value;
    out0[I] = fma_half_lane<I>(a, x, g, h1);
    out1[I] = fma_half_lane_dpp<I>(a, x, g, h1);
  });
#pragma unroll
  for (int k = 0; k < kLaneMasks; k++) {
    const uint64_t mk = mask_shl(m[k], 0);
    out0[32 + k] = sel_mask(mk, a, g);
    out1[32 + k] = sel_mask_open(mk, a, g);
  }
}
}  // namespace nm
