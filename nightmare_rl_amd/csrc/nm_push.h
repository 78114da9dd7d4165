// nm_push.h - push perturbations (the `domain_rand.push_robots` of legged_gym-shaped config trees; SURVEY 8(f) row 4, the reference has
// no such line): every `interval` env steps the base's world-frame linear velocity qvel[env, 0:2] is SET to (vx, vy), each uniform in
// [-max, +max), before the physics of that step. A push is an edit of the state between two steps and nothing else: qacc_warmstart, the
// stale dof_vel / cvel buffers and qvel[2:] stay what they were.
//
// The env object counts its full env steps on the host (push step index s: nm_hip.hip, next to noise_step). The step with index s is
// pushed iff interval > 0 && s > 0 && s % interval == 0, and draws
//     u = rand_u24_bits(seed + kPushKey, global env id, 2 * (s / interval) + axis) * 2^-24,    v = (2 u - 1) * max
// in the env's precision: 2 u - 1 is exact (u has 24 bits), so v is rounded once. The key is the global env id: sharding changes nothing.
//   * per-step path: the host launches k_push on the step's stream before k_env_step, on due steps only
//   * K-step launches: nmr::step_push (nm_env_loop.h) inside the wave that owns the env, parameters in nmr::PushArgs (nm_rollout.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nm_core.h"

namespace nm {

constexpr uint64_t kPushKey = 0x50555348ull;

inline bool push_due(int interval, uint64_t s) { return interval > 0 && s > 0 && s % (uint64_t)interval == 0; }
// the counter of axis 0 of the push at step s (s % interval == 0); axis 1 draws the next one
inline uint32_t push_counter(int interval, uint64_t s) { return (uint32_t)(2 * (s / (uint64_t)interval)); }

template <class real> NM_FN real push_value(uint64_t seed, uint64_t genv, uint32_t ctr, real maxv) {
  const real u = (real)rand_u24_bits(seed + kPushKey, genv, ctr) * real(1.0 / 16777216.0);
  return (real(2) * u - real(1)) * maxv;
}

// one thread per (env, axis)
template <class real>
__global__ void k_push(real* __restrict__ qvel, int N, uint64_t seed, int64_t env_offset, uint32_t ctr0, real maxv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * N) return;
  const int env = i >> 1, axis = i & 1;
  qvel[(size_t)env * kNV + axis] = push_value<real>(seed, (uint64_t)(env_offset + env), ctr0 + (uint32_t)axis, maxv);
}

}  // namespace nm
