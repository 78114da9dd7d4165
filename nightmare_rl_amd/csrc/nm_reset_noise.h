// nm_reset_noise.h - randomised reset states (the `_reset_dofs` / `_reset_root_states` of legged_gym-shaped stacks; the reference has no
// such line: its reset_idx writes qpos0 and zero velocity, env.py:335-371). While the feature is on, an env's reset - time-out, termination
// or a host reset_idx - writes qpos0 and zero velocity as before and then overwrites 43 words of the same env's rows:
//     column c    word           value
//     0           qpos[2]        qpos0[2] + d(0)              base_height range
//     1..18       qpos[7 + j]    qpos0[7 + j] + d(1 + j)      dof_pos range
//     19..21      qvel[0:3]      d(c)                         base_lin_vel range (world frame)
//     22..24      qvel[3:6]      d(c)                         base_ang_vel range
//     25..42      qvel[6 + j]    d(c)                         dof_vel range
// qpos[0:2] and the base quaternion keep their qpos0 values (yaw is a symmetry of the flat floor under body-frame commands, and nothing
// here divides or takes a root: the fp32 build's 2.5-ulp sequences could not be restated bit for bit). A reset draw is an edit of the
// state between two steps and nothing else: qacc_warmstart, the stale dof_pos / dof_vel / cvel buffers, the command resample, rngctr and
// the feet state stay what they were, the resetting step returns the terminal observation, and the bad-state reset inside the physics
// still goes to qpos0.
//
// The draw, in the env's precision `real`, with lo_r = real(lo), w_r = real(hi) - real(lo) of the column's range:
//     u = rand_u24_bits(seed + kResetKey, global env id, 64 k + c) * 2^-24,    d(c) = lo_r + u * w_r
// product and sum rounded separately (contraction off, the rules of nm_draw_env_params), the counter in 32 bits (it wraps at k = 2^26).
// k is the env's reset count, a device uint32 [N] buffer read by all 43 columns and then incremented by one - by the env's one owner:
//   * per-step path: k_reset_noise, launched on the step's stream right behind k_env_step while the feature is on; it reads done[env]
//     on the device, so there is no host decision and the pair of launches can be captured into a graph
//   * nm_reset: k_reset_noise behind k_reset, for the ids it reset (distinct ids: a repeated id would have two owners)
//   * K-step launches: nmr::step_reset_noise (nm_env_loop.h) inside the wave that owns the env, parameters in nmr::ResetNoiseArgs
// A range (0, 0) gives +0 offsets: on with ten zeros equals off, bit for bit. The key is the global env id: sharding changes nothing.
#pragma once
#include <stdint.h>

#include "nm_core.h"

namespace nm {

constexpr uint64_t kResetKey = 0x5245534554ull;
constexpr int kResetCols = 43, kResetRanges = 5;     // ranges in the order base_height, dof_pos, base_lin_vel, base_ang_vel, dof_vel

// the column table
NM_HDFN int reset_col_range(int c) { return c == 0 ? 0 : c < 19 ? 1 : c < 22 ? 2 : c < 25 ? 3 : 4; }
NM_HDFN bool reset_col_qpos(int c) { return c < 19; }                                   // else a word of qvel
NM_HDFN int reset_col_word(int c) { return c == 0 ? 2 : c < 19 ? 6 + c : c - 19; }      // index into the env's qpos / qvel row

// the converted ranges: lo_r and w_r per range
template <class real> struct ResetNoise { real lo[kResetRanges], w[kResetRanges]; };
template <class real> NM_HDFN ResetNoise<real> reset_noise_params(const double* ranges10) {
  ResetNoise<real> p;
  for (int r = 0; r < kResetRanges; r++) { p.lo[r] = (real)ranges10[2 * r]; p.w[r] = (real)ranges10[2 * r + 1] - (real)ranges10[2 * r]; }
  return p;
}

// d(c) of reset k of the env with global id genv
template <class real> NM_HDFN real reset_noise_draw(const ResetNoise<real>& p, uint64_t seed, uint64_t genv, uint32_t k, int c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int r = reset_col_range(c);
  const real lo = r == 0 ? p.lo[0] : r == 1 ? p.lo[1] : r == 2 ? p.lo[2] : r == 3 ? p.lo[3] : p.lo[4];
  const real w = r == 0 ? p.w[0] : r == 1 ? p.w[1] : r == 2 ? p.w[2] : r == 3 ? p.w[3] : p.w[4];
  const real u = (real)rand_u24_bits(seed + kResetKey, genv, 64u * k + (uint32_t)c) * real(1.0 / 16777216.0);
  const real prod = u * w;
  return lo + prod;
}

#ifndef NM_EMUL
// column c of reset k of env `env` (local index; genv = its global id): the draw into its word. qpos0: the model's [kNQ] row in device memory.
template <class real>
NM_FN void reset_noise_apply(real* qpos, real* qvel, const real* qpos0, const ResetNoise<real>& p, uint64_t seed, uint64_t genv, size_t env,
                             uint32_t k, int c) {
  const real d = reset_noise_draw<real>(p, seed, genv, k, c);
  const int w = reset_col_word(c);
  if (reset_col_qpos(c)) simt::gst1(qpos, env * kNQ + w, simt::gld1(qpos0, (size_t)w) + d);
  else simt::gst1(qvel, env * kNV + w, d);
}

// One wave per env to reset: lanes 0..42 own the columns, lane 0 the count (its store needs the value every lane of the wave has loaded
// by then: nobody reads the count after it is written). ids: the envs to look at, or null = envs 0..n-1; done: [N] reset flags of the
// step that just ran, or null = every listed env (nm_reset).
template <class real>
__global__ void __launch_bounds__(256) k_reset_noise(real* __restrict__ qpos, real* __restrict__ qvel, uint32_t* __restrict__ count,
                                                    const real* __restrict__ qpos0, ResetNoise<real> p, uint64_t seed, int64_t env_offset,
                                                    const int64_t* __restrict__ done, const int32_t* __restrict__ ids, int n) {
  const int j = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), c = (int)(threadIdx.x & 63);
  if (j >= n) return;
  const int env = ids ? ids[j] : j;
  if (done && done[env] <= 0) return;
  const uint32_t k = count[env];
  if (c < kResetCols) reset_noise_apply<real>(qpos, qvel, qpos0, p, seed, (uint64_t)(env_offset + env), (size_t)env, k, c);
  if (c == 0) count[env] = k + 1u;
}
#endif

}  // namespace nm
