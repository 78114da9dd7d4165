// nm_wrench.h - the schedule of the external wrench on the base (nm_set_wrench_schedule; the rows and what the physics does with them:
// nm_core.h kWrenchP, level 7 of the step). Legged_gym-shaped trainers know it as "external force / torque on the base"; MuJoCo as
// xfrc_applied. The reference has no such line. Unlike a push (nm_push.h), which edits the state for one instant, a wrench acts through
// the physics for as long as its row holds it.
//
// The env object counts its full env steps on the host (wrench step index s: nm_hip.hip, next to push_step; K per K-step launch,
// physics-only launches and nm_reset leave it alone). With interval >= 1 and 1 <= duration <= interval, at the start of step s the
// env's row is
//     a fresh draw   if s >= interval && s % interval == 0         (window q = s / interval opens)
//     set to zero    if s >= interval && s % interval == duration  (the window closes; only when duration < interval)
//     unchanged      otherwise
// a stateless function of s. The draw of window q, per axis (0..2 = F x y z, 3..5 = tau x y z; word axis + (axis >= 3) of the row):
//     u = rand_u24_bits(seed + kWrenchKey, global env id, 6 q + axis) * 2^-24,    v = (2 u - 1) * max[axis]
// in the env's precision: 2 u - 1 is exact (u has 24 bits), so v is rounded once. The key is the global env id: sharding changes nothing.
// The pads of a row stay zero. A reset of an env does not touch its row.
//   * per-step path: the host launches k_wrench on the step's stream before k_env_step, on due steps only
//   * K-step launches: nmr::step_wrench (nm_env_loop.h) inside the wave that owns the env, parameters in nmr::WrenchArgs (nm_rollout.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nm_core.h"

namespace nm {

// what step s does to the rows: 0 nothing, 1 a fresh draw of window s / interval, 2 zero
inline int wrench_due(int interval, int duration, uint64_t s) {
  if (interval <= 0 || s < (uint64_t)interval) return 0;
  const uint64_t r = s % (uint64_t)interval;
  return r == 0 ? 1 : (duration < interval && r == (uint64_t)duration ? 2 : 0);
}
// the rows that hold once step s has begun: 1 = the draw of window s / interval, 2 = zero (what nm_set_wrench_schedule installs)
inline int wrench_held(int interval, int duration, uint64_t s) {
  if (interval <= 0 || s < (uint64_t)interval) return 2;
  return s % (uint64_t)interval < (uint64_t)duration ? 1 : 2;
}
// the window number as the counter sees it (mod 2^32)
inline uint32_t wrench_window(int interval, uint64_t s) { return (uint32_t)(s / (uint64_t)interval); }

template <class real> NM_FN real wrench_value(uint64_t seed, uint64_t genv, uint32_t q, int axis, real maxv) {
  const real u = (real)rand_u24_bits(seed + kWrenchKey, genv, 6u * q + (uint32_t)axis) * real(1.0 / 16777216.0);
  return (real(2) * u - real(1)) * maxv;
}
NM_FN int wrench_word(int axis) { return axis + (axis >= 3 ? 1 : 0); }

template <class real> struct WrenchMax { real v[6]; };

// one thread per (env, axis): the draw of window q, or zero
template <class real>
__global__ void k_wrench(real* __restrict__ rows, int N, uint64_t seed, int64_t env_offset, uint32_t q, int draw, WrenchMax<real> maxv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 6 * N) return;
  const int env = i / 6, axis = i - env * 6;
  rows[(size_t)env * kWrenchP + wrench_word(axis)] = draw ? wrench_value<real>(seed, (uint64_t)(env_offset + env), q, axis, maxv.v[axis]) : real(0);
}

}  // namespace nm
