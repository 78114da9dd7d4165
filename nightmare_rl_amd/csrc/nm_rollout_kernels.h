// nm_rollout_kernels.h - the kernels of the K-step rollout that carry the policy (k_env_rollout, k_roll_act), for ONE hidden activation:
// included by nm_rollout_<activation>.hip, each a translation unit of its own that defines NM_ROLLOUT_ACT (an NM_ACT_* code) first.
//
// One translation unit per activation, not six instantiations in one: with all six k_env_rollout kernels (each a copy of the physics
// around the wave policy) in one unit the register allocation of every one of them, the ELU one included, went from 2 VGPR spills
// (520 B of scratch per lane) to 4 (548 B); alone in its unit each gets the allocation the single ELU kernel had. It also keeps the
// measurement build (-DNM_MEASURE) at one instantiation. The common part of the rollout (k_rollout_tail, k_rollout_clear, k_roll_pack and
// the host launchers that pick the activation's instantiation) is nm_rollout.hip.
#include <hip/hip_runtime.h>

#include "nm_env_loop.h"

#ifndef NM_ROLLOUT_ACT
#error "define NM_ROLLOUT_ACT (an NM_ACT_* code) before including nm_rollout_kernels.h"
#endif
#ifndef NM_WAVES_PER_SIMD
#define NM_WAVES_PER_SIMD 2
#endif

namespace nmr {

// The record of step t - 1 (t > 0; the episode books of nm_env_loop.h) and PPO.act of step t for the wave's envs + the launch arguments
// of the env step that follows.
// Out of line: its registers (weight ring, accumulators) are not live across the physics, and the physics' are not live here.
// WX: the launch carries the wrench schedule (level 7 alone), so that the step functions of the lower levels keep their code.
template <class S, int ACT, bool WX>
__device__ __noinline__ void policy_step(float* xb, const RollArgs* Rs, nm::Args<float>* As, int t, int wave, uint64_t noise0) {
  const int N = As->N;
  const size_t so = (size_t)t * N;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // state rows, observation, reward / done / time-out of the previous step: stored
  BookRegs rec;
  if (t > 0) books_load(rec, Rs, As, wave);          // issued before the observation loads below: they return together
  ActOut o{Rs->s_actions + so * nm::kNU, Rs->s_logp + so, Rs->s_values + so, Rs->s_mu + so * nm::kNU, Rs->s_sigma + so * nm::kNU, t == 0 ? Rs->s_obs : nullptr};
  // the observation is the one this wave's previous step wrote into the storage row of step t
  policy_wave<S, ACT>(xb, Rs->wp, Rs->bp, Rs->stdv, t == 0 ? Rs->obs0 : Rs->s_obs + so * nm::kNOBS, N, wave, Rs->seed, (uint64_t)simt::gld1(Rs->iter_dev, 0) * 4096ull + (uint64_t)t, o);
  if (t > 0) { books_file(rec, Rs, As, t - 1, wave); step_reset_noise(Rs, As, rec.d, wave); step_reset_rows(Rs, As, rec.d, wave); }   // the reset draw of step t - 1, before the push of step t
  if (threadIdx.x == 0) {
    As->actions = o.actions;
    As->obs = t + 1 < Rs->K ? Rs->s_obs + (so + N) * nm::kNOBS : Rs->obs_final;     // the step files its observation where the next act reads it
    step_args(As, Rs, t, noise0);
  }
  step_push(Rs, As, t, wave);
  if constexpr (WX) step_wrench(As, t, wave);
  step_close();
}
// PPO.compute_returns' `last_values = actor_critic.evaluate(last_critic_obs)` for the wave's envs: the forward once more, on the observation the
// last step left in obs_final (this wave's own stores: waited for by books_last), value head only - instead of nine framework launches
template <class S, int ACT>
__device__ __noinline__ void value_last(float* xb, const RollArgs* Rs, const nm::Args<float>* As, int wave) {
  ActOut o{nullptr, nullptr, Rs->last_values, nullptr, nullptr, nullptr};
  nm::wave_sync();
  policy_wave<S, ACT, kPolicyValueOnly>(xb, Rs->wp, Rs->bp, Rs->stdv, Rs->obs_final, As->N, wave, 0, 0, o);
}

template <class S, int ACT, int EP>      // EP: level of per-env physics parameters, above 0 launched only while rows are set (nm_core.h env_mu)
__global__ void __launch_bounds__(64, NM_WAVES_PER_SIMD) k_env_rollout(const nm::Model<float>* __restrict__ Mp, nm::Args<float> A, RollArgs R) {
  __shared__ typename nm::ShWSel<float, 2, EP>::type shl;
  nm::ShW<float, 2>& sh = nm::ShWSel<float, 2, EP>::images(shl);
  __shared__ nm::Model<float> Ms;
  __shared__ nm::Args<float> As;
  __shared__ RollArgs Rs;
  static_assert(sizeof(sh) >= kXFloats * sizeof(float), "the policy's activation rows alias the env images");
  int wave;
  if (!loop_begin(Mp, A, R, Ms, As, Rs, wave)) return;
  float* xb = reinterpret_cast<float*>(&sh);          // between two steps the env images hold nothing that is needed (env_load2 rewrites them)
  const uint64_t noise0 = A.noise_step;
  const int K = R.K;
  if (R.wave_clock && threadIdx.x == 0) R.wave_clock[2 * wave] = __builtin_amdgcn_s_memtime();
  for (int t = 0; t < K; t++) {
    policy_step<S, ACT, (EP >= 7)>(xb, &Rs, &As, t, wave, noise0);    // (+ the record of step t - 1)
    nm::wave_step<float, 2, EP>(sh, Ms, As, wave);        // env.step: load, decimation x mj_step, epilogue - the code of k_env_step
  }
  books_last(&Rs, &As, K - 1, wave);
  if (Rs.last_values) value_last<S, ACT>(xb, &Rs, &As, wave);
  if (Rs.wave_clock && threadIdx.x == 0) Rs.wave_clock[2 * wave + 1] = __builtin_amdgcn_s_memtime();
}
// One env's policy step as a launch of its own: PPO.act on the same wave code (the step-by-step counterpart of k_env_rollout and its
// bit-exact reference in tests/test_gpu_rollout.py). One wave = two envs.
template <class S, int ACT>
__global__ void __launch_bounds__(64) k_roll_act(const f32x4* __restrict__ wp, const float* __restrict__ bp, const float* __restrict__ stdv, const float* __restrict__ obs,
                                                 int N, uint64_t seed, const int64_t* __restrict__ iter_dev, int step, ActOut o) {
  __shared__ float xb[kXFloats];
  policy_wave<S, ACT>(xb, wp, bp, stdv, obs, N, (int)blockIdx.x, seed, (uint64_t)iter_dev[0] * 4096ull + (uint64_t)step, o);
}

template <int ACT>
int RollKernels<ACT>::act(const float* wp, const float* bp, const float* stdv, const float* obs, int N, uint64_t seed, const int64_t* iter_dev, int step,
                          const ActOut& o, hipStream_t s) {
  hipLaunchKernelGGL((k_roll_act<RefShape, ACT>), dim3((N + 1) / 2), dim3(64), 0, s, (const f32x4*)wp, bp, stdv, obs, N, seed, iter_dev, step, o);
  return hipGetLastError() != hipSuccess;
}
template <int ACT>
int RollKernels<ACT>::rollout(const nm::Model<float>* M_dev, const nm::Args<float>& a, const RollArgs& R, int level, hipStream_t s) {
  nmrows::with_level(level, [&](auto L) { hipLaunchKernelGGL((k_env_rollout<RefShape, ACT, decltype(L)::value>), dim3((a.N + 1) / 2), dim3(64), 0, s, M_dev, a, R); });
  return hipGetLastError() != hipSuccess;
}
template struct RollKernels<NM_ROLLOUT_ACT>;

}  // namespace nmr
