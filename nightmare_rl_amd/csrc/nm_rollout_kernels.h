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
#ifdef NM_ROLLOUT_PRIV
#include "nm_priv_obs.h"
#endif

#ifndef NM_ROLLOUT_ACT
#error "define NM_ROLLOUT_ACT (an NM_ACT_* code) before including nm_rollout_kernels.h"
#endif
#ifndef NM_WAVES_PER_SIMD
#define NM_WAVES_PER_SIMD 2
#endif

namespace nmr {

#ifndef NM_ROLLOUT_PRIV
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
  if (t > 0) step_sensor(Rs, As, Rs->s_obs + so * nm::kNOBS, rec.d, wave);      // the sensor model of step t - 1: the sensed row into the storage row act t reads
  ActOut o{Rs->s_actions + so * nm::kNU, Rs->s_logp + so, Rs->s_values + so, Rs->s_mu + so * nm::kNU, Rs->s_sigma + so * nm::kNU, t == 0 ? Rs->s_obs : nullptr};
  // the observation is the one this wave's previous step wrote into the storage row of step t
  policy_wave<S, ACT>(xb, Rs->wp, Rs->bp, Rs->stdv, t == 0 ? Rs->obs0 : Rs->s_obs + so * nm::kNOBS, N, wave, Rs->seed, (uint64_t)simt::gld1(Rs->iter_dev, 0) * 4096ull + (uint64_t)t, o);
  if (t > 0) { books_file(rec, Rs, As, t - 1, wave); step_reset_noise(Rs, As, rec.d, wave); step_reset_rows(Rs, As, rec.d, wave); }   // the reset draw of step t - 1, before the push of step t
  if (threadIdx.x == 0) {
    As->actions = o.actions;
    // the step files its observation where the next act reads it - or, while the sensor model is on, where the launcher pointed it: the true-obs buffer
    if (Rs->sensor.on == 0) As->obs = t + 1 < Rs->K ? Rs->s_obs + (so + N) * nm::kNOBS : Rs->obs_final;
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
  step_sensor_last(&Rs, &As, Rs.obs_final, wave);     // the last step's sensed row, in front of the value of it
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
#else   // NM_ROLLOUT_PRIV: the same two kernels for the asymmetric actor-critic (PrivShape), compiled by nm_rollout_priv_<activation>.hip
// ---- The asymmetric rollout: the critic reads the privileged row (nm_priv_obs.h: the step's observation + kPrivN columns of what the env's
// physics was drawn with), the actor its first kNOBS columns. The wave that owns the env gathers the columns itself, with the function
// k_priv_obs uses (nm::priv_value<float>: the same bits), at the place in the step where the per-step path launches k_priv_obs: behind the
// reset draws of the step that ended, in front of the push and the wrench of the step that begins.
typedef const __attribute__((address_space(1))) float* gfp_t;
typedef __attribute__((address_space(1))) float* gwp_t;

// The rows of the wave's two envs -> row 0 of xb (what policy_wave<.., LOAD = false> reads) and -> row_out [N,kPrivRow]: columns 0..65 from
// `obs` [N,kNOBS] (this wave's own stores, waited for by the caller), columns 66..88 from lanes 0..45 = (env lane / 23, column lane % 23).
// An env past N (odd N, last wave) gets the values of env N - 1 in LDS and files nothing. Out of line: its double arithmetic and the
// descriptor's words are nobody else's registers.
static __device__ __noinline__ void priv_gather(float* xb, const nm::PrivObsArgs<float>* desc, const float* obs, float* row_out, int N, int wave) {
  const int lane = threadIdx.x;
  const gfp_t og = (gfp_t)obs;
  const gwp_t rg = (gwp_t)row_out;
#pragma unroll
  for (int i = 0; i < (2 * nm::kNOBS + 63) / 64; i++) {
    const int idx = lane + 64 * i;
    if (idx < 2 * nm::kNOBS) {
      const int e = idx >= nm::kNOBS, k = idx - e * nm::kNOBS, env = wave * 2 + e;
      const float v = og[(size_t)min(env, N - 1) * nm::kNOBS + k];
      xb[e * kXW + k] = v;
      if (env < N) rg[(size_t)env * nm::kPrivRow + k] = v;
    }
  }
  if (lane < 2 * nm::kPrivN) {
    const int e = lane >= nm::kPrivN, c = lane - e * nm::kPrivN, env = wave * 2 + e;
    const float v = nm::priv_value<float>(*desc, (size_t)min(env, N - 1), c);
    xb[e * kXW + nm::kNOBS + c] = v;
    if (env < N) rg[(size_t)env * nm::kPrivRow + nm::kNOBS + c] = v;
  }
  if (lane < 2 * (PrivShape::up4(nm::kPrivRow) - nm::kPrivRow)) xb[(lane & 1) * kXW + nm::kPrivRow + (lane >> 1)] = 0.0f;
}
// t = 0: nothing is gathered - the env's current row (what step() or the launch before handed out) -> row 0 of xb, the storage's row 0
// and, its prefix, the observation storage's row 0
static __device__ __noinline__ void priv_first(float* xb, const float* rows, float* s_priv, float* s_obs, int N, int wave) {
  const int lane = threadIdx.x;
  const gfp_t rg = (gfp_t)rows;
#pragma unroll
  for (int i = 0; i < (2 * nm::kPrivRow + 63) / 64; i++) {
    const int idx = lane + 64 * i;
    if (idx < 2 * nm::kPrivRow) {
      const int e = idx >= nm::kPrivRow, k = idx - e * nm::kPrivRow, env = wave * 2 + e;
      const float v = rg[(size_t)min(env, N - 1) * nm::kPrivRow + k];
      xb[e * kXW + k] = v;
      if (env < N) {
        ((gwp_t)s_priv)[(size_t)env * nm::kPrivRow + k] = v;
        if (k < nm::kNOBS) ((gwp_t)s_obs)[(size_t)env * nm::kNOBS + k] = v;
      }
    }
  }
  if (lane < 2 * (PrivShape::up4(nm::kPrivRow) - nm::kPrivRow)) xb[(lane & 1) * kXW + nm::kPrivRow + (lane >> 1)] = 0.0f;
}

// The step function of the asymmetric launch. The row act t sees is the row the per-step path hands out after step t - 1: so the books of
// step t - 1 are filed and its reset draws made FIRST (their bodies end with a wait for their stores), then the wave gathers, then the
// policy runs; the push and the wrench of step t come last, as k_wrench of step t runs behind k_priv_obs of step t - 1.
template <class S, int ACT, bool WX>
__device__ __noinline__ void policy_step(float* xb, const RollPrivArgs* Rs, nm::Args<float>* As, int t, int wave, uint64_t noise0) {
  const int N = As->N;
  const size_t so = (size_t)t * N;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // state rows, observation, reward / done / time-out of the previous step: stored
  if (t > 0) {
    BookRegs rec;
    books_load(rec, Rs, As, wave);
    books_file(rec, Rs, As, t - 1, wave); step_reset_noise(Rs, As, rec.d, wave); step_reset_rows(Rs, As, rec.d, wave);
    step_sensor(Rs, As, Rs->s_obs + so * nm::kNOBS, rec.d, wave);      // the sensor model of step t - 1: the gather below reads the sensed row
    priv_gather(xb, Rs->desc, Rs->s_obs + so * nm::kNOBS, Rs->s_priv + so * nm::kPrivRow, N, wave);
  } else {
    priv_first(xb, Rs->priv0, Rs->s_priv, Rs->s_obs, N, wave);
  }
  ActOut o{Rs->s_actions + so * nm::kNU, Rs->s_logp + so, Rs->s_values + so, Rs->s_mu + so * nm::kNU, Rs->s_sigma + so * nm::kNU, nullptr};
  policy_wave<S, ACT, kPolicyFull, false>(xb, Rs->wp, Rs->bp, Rs->stdv, nullptr, N, wave, Rs->seed, (uint64_t)simt::gld1(Rs->iter_dev, 0) * 4096ull + (uint64_t)t, o);
  if (threadIdx.x == 0) {
    As->actions = o.actions;
    if (Rs->sensor.on == 0) As->obs = t + 1 < Rs->K ? Rs->s_obs + (so + N) * nm::kNOBS : Rs->obs_final;      // (on: the true-obs buffer, set by the launcher)
    step_args(As, Rs, t, noise0);
  }
  step_push(Rs, As, t, wave);
  if constexpr (WX) step_wrench(As, t, wave);
  step_close();
}
// the end of the launch, behind books_last (which has waited for the last step's stores and made its reset draws): the row once more,
// into the env's buffer, and PPO.compute_returns' last value on it
template <class S, int ACT>
__device__ __noinline__ void value_last(float* xb, const RollPrivArgs* Rs, const nm::Args<float>* As, int wave) {
  priv_gather(xb, Rs->desc, Rs->obs_final, Rs->priv_final, As->N, wave);
  if (!Rs->last_values) return;
  ActOut o{nullptr, nullptr, Rs->last_values, nullptr, nullptr, nullptr};
  policy_wave<S, ACT, kPolicyValueOnly, false>(xb, Rs->wp, Rs->bp, Rs->stdv, nullptr, As->N, wave, 0, 0, o);
}

template <class S, int ACT, int EP>
__global__ void __launch_bounds__(64, NM_WAVES_PER_SIMD) k_env_rollout(const nm::Model<float>* __restrict__ Mp, nm::Args<float> A, RollPrivArgs R) {
  __shared__ typename nm::ShWSel<float, 2, EP>::type shl;
  nm::ShW<float, 2>& sh = nm::ShWSel<float, 2, EP>::images(shl);
  __shared__ nm::Model<float> Ms;
  __shared__ nm::Args<float> As;
  __shared__ RollPrivArgs Rs;
  static_assert(sizeof(sh) >= kXFloats * sizeof(float), "the policy's activation rows alias the env images");
  int wave;
  if (!loop_begin(Mp, A, R, Ms, As, Rs, wave)) return;
  float* xb = reinterpret_cast<float*>(&sh);
  const uint64_t noise0 = A.noise_step;
  const int K = R.K;
  if (R.wave_clock && threadIdx.x == 0) R.wave_clock[2 * wave] = __builtin_amdgcn_s_memtime();
  for (int t = 0; t < K; t++) {
    policy_step<S, ACT, (EP >= 7)>(xb, &Rs, &As, t, wave, noise0);
    nm::wave_step<float, 2, EP>(sh, Ms, As, wave);
  }
  books_last(&Rs, &As, K - 1, wave);
  step_sensor_last(&Rs, &As, Rs.obs_final, wave);     // the last step's sensed row, in front of the final gather
  value_last<S, ACT>(xb, &Rs, &As, wave);
  if (Rs.wave_clock && threadIdx.x == 0) Rs.wave_clock[2 * wave + 1] = __builtin_amdgcn_s_memtime();
}
// PPO.act on a [N,89] row as a launch of its own: the step-by-step reference of the launch above. The loader of policy_wave takes the
// whole row (and files it in o.obs_store); the prefix, if wanted, is copied beside it.
template <class S, int ACT>
__global__ void __launch_bounds__(64) k_roll_act(const f32x4* __restrict__ wp, const float* __restrict__ bp, const float* __restrict__ stdv, const float* __restrict__ rows,
                                                 int N, uint64_t seed, const int64_t* __restrict__ iter_dev, int step, ActOut o, float* __restrict__ prefix_store) {
  __shared__ float xb[kXFloats];
  const int wave = (int)blockIdx.x, lane = threadIdx.x;
  if (prefix_store) {
    for (int idx = lane; idx < 2 * nm::kNOBS; idx += 64) {
      const int e = idx >= nm::kNOBS, k = idx - e * nm::kNOBS, env = wave * 2 + e;
      if (env < N) prefix_store[(size_t)env * nm::kNOBS + k] = rows[(size_t)env * nm::kPrivRow + k];
    }
  }
  policy_wave<S, ACT>(xb, wp, bp, stdv, rows, N, wave, seed, (uint64_t)iter_dev[0] * 4096ull + (uint64_t)step, o);
}

template <int ACT>
int RollPrivKernels<ACT>::act(const float* wp, const float* bp, const float* stdv, const float* rows, int N, uint64_t seed, const int64_t* iter_dev, int step,
                              const ActOut& o, float* prefix_store, hipStream_t s) {
  hipLaunchKernelGGL((k_roll_act<PrivShape, ACT>), dim3((N + 1) / 2), dim3(64), 0, s, (const f32x4*)wp, bp, stdv, rows, N, seed, iter_dev, step, o, prefix_store);
  return hipGetLastError() != hipSuccess;
}
template <int ACT>
int RollPrivKernels<ACT>::rollout(const nm::Model<float>* M_dev, const nm::Args<float>& a, const RollPrivArgs& R, int level, hipStream_t s) {
  nmrows::with_level(level, [&](auto L) { hipLaunchKernelGGL((k_env_rollout<PrivShape, ACT, decltype(L)::value>), dim3((a.N + 1) / 2), dim3(64), 0, s, M_dev, a, R); });
  return hipGetLastError() != hipSuccess;
}
template struct RollPrivKernels<NM_ROLLOUT_ACT>;
#endif

}  // namespace nmr
