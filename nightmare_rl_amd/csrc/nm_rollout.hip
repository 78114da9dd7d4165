// nm_rollout.hip - K env steps per launch with the policy inside the env's wavefront (C ABI: nm_rollout / nm_rollout_act in nm_hip.hip).
//
// The on-policy rollout of rsl_rl v1.0.2 (OnPolicyRunner.learn: `for i in range(num_steps_per_env): actions = alg.act(obs, critic_obs);
// obs, _, rewards, dones, infos = env.step(actions); alg.process_env_step(rewards, dones, infos)`, the loop reference train.py:54 drives,
// horizon envs/nightmare_v3_config.py:135) as ONE launch: every wave keeps its two envs for all K steps - policy forward + sampling
// (nm_rollout.h), the physics step and epilogue of k_env_step (nm::wave_step, the same code), the transition record - and goes straight
// from step t into step t + 1: no launch boundary, no wait for the slowest wave of the step. What crosses waves is collected per step
// (episode-sum atomics, reset counts) and closed by k_rollout_tail afterwards.
//
// A translation unit of its own: a second kernel around nm::wave_step in nm_hip.hip changed the register allocation of k_env_step
// (250 VGPRs / no spill -> 256 / 1 spill); here the two kernels cannot see each other.
//
// The kernels that carry the policy (k_env_rollout, k_roll_act) are in nm_rollout_kernels.h, compiled once per hidden activation in
// nm_rollout_<activation>.hip; this unit holds what does not depend on the activation and the launchers that choose the instantiation.
#include <hip/hip_runtime.h>

#include "nm_core.h"
#include "nm_rollout.h"

namespace nmr {

// Closes a rollout of K steps: what the closing wave of every k_env_step launch does per step (step_tail in nm_hip.hip), for all K steps in
// order, plus the two things of PPO.process_env_step / the runner that need them.
//   * extras['episode'] (ep_stats) is refreshed by every step in which >= 1 env reset (env.py:344-371), and the runner adds the CURRENT
//     extras to its running sum after every step (ep_acc[i] += ep_stats[ep_idx[i]]) - also the stale one of a step without resets;
//   * extras['time_outs'] likewise keeps the flags of the last step that had a reset, and PPO.process_env_step adds gamma * value *
//     time_outs at EVERY step - so an env's bootstrap term is applied from its time-out step until the next step with a reset.
//     `time_outs` on entry = the flags left by the steps before this rollout; on exit = those of the last refreshing step.
constexpr int kTailSteps = 4096;     // nm_rollout's limit on K
__global__ void __launch_bounds__(256) k_rollout_tail(TailArgs a) {
  __shared__ int cnts[kTailSteps];      // resets of step t (> 0: the step refreshed the extras) - read K times by every thread below
  const int tid = threadIdx.x, N = a.N, K = a.K;
  for (int t = tid; t < K; t += 256) cnts[t] = a.st_cnt[t * 4];
  __syncthreads();
  if (blockIdx.x == 0) {
    // extras['episode'][k] after every step, and the runner's running sum of it: thread k < 16 follows reward k, thread 16 + i the i-th
    // summed key - each walks the K steps on its own (no exchange: a summed key recomputes its reward's value), additions in step order
    if (tid < nm::kNREW + a.n_ep) {
      const bool sums = tid >= nm::kNREW;
      const int k = sums ? a.ep_idx[tid - nm::kNREW] : tid;
      float e = a.ep_stats ? a.ep_stats[k] : 0.f, acc = sums ? a.ep_acc[tid - nm::kNREW] : 0.f;
      for (int t = 0; t < K; t++) {
        const int cnt = cnts[t];
        if (cnt > 0) e = (float)(a.st_sum[(size_t)t * nm::kNREW + k] / (float)cnt / a.ep_len_s);
        acc += e;
      }
      if (sums) a.ep_acc[tid - nm::kNREW] = acc;
      else if (a.ep_stats) a.ep_stats[k] = e;
    }
    if (tid == 255) {
      long long c1 = 0, c2 = 0;
      for (int t = 0; t < K; t++) { c1 += a.st_cnt[t * 4 + 1]; c2 += a.st_cnt[t * 4 + 2]; }
      a.counters[0] += c1; a.counters[1] += c2;
      *a.to_owner = 0ull;          // the next nm_step rewrites extras['time_outs'] in full
    }
  }
  // time-out bootstrap and the final extras['time_outs'], one thread per env
  int tl = -1;
  for (int t = 0; t < K; t++) if (cnts[t] > 0) tl = t;
  for (int e = blockIdx.x * blockDim.x + tid; e < N; e += gridDim.x * blockDim.x) {
    const int ts = a.to_step[e];
    // k_ppo_record's `rew + gamma * value * time_out` with time_out = 1: the product rounded, then the sum rounded (bit for bit)
    auto boot = [&](int t) {
#pragma clang fp contract(off)      // HIP's __fmul_rn / __fadd_rn are plain operators: without this the pair becomes one fma (one rounding)
      const size_t i = (size_t)t * N + e;
      const float gv = a.gamma * a.s_values[i];
      a.s_rewards[i] = a.s_rewards[i] + gv;
    };
    const bool boots = a.gamma >= 0.f;
    if (boots && a.time_outs && a.time_outs[e] != 0.f)         // flags from before the rollout hold until the first refresh
      for (int t = 0; t < K && cnts[t] == 0; t++) boot(t);
    if (boots && ts >= 0 && a.time_outs)
      for (int t = ts; t < K && (t == ts || cnts[t] == 0); t++) boot(t);
    if (a.time_outs && tl >= 0) a.time_outs[e] = ts == tl ? 1.f : 0.f;
  }
}
// the per-step accumulators of a rollout back to zero (a launch of its own: after EVERY block of k_rollout_tail has read them)
__global__ void k_rollout_clear(int K, float* st_sum, int* st_cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < K * nm::kNREW) st_sum[i] = 0.f;
  if (i < K * 4) st_cnt[i] = 0;
}

int launch_pack(const float* flat, float* wp, float* bp, hipStream_t s) {
  const int n = RefShape::nfrag() * 256;
  hipLaunchKernelGGL(k_roll_pack<RefShape>, dim3((n + 255) / 256), dim3(256), 0, s, flat, wp, bp);
  return hipGetLastError() != hipSuccess;
}

int launch_pack_priv(const float* flat, float* wp, float* bp, hipStream_t s) {
  const int n = PrivShape::nfrag() * 256;
  hipLaunchKernelGGL(k_roll_pack<PrivShape>, dim3((n + 255) / 256), dim3(256), 0, s, flat, wp, bp);
  return hipGetLastError() != hipSuccess;
}

// The per-activation instantiations (nm_rollout_<activation>.hip; each k_env_rollout carries its own copy of the physics: ~19 s of device
// compile apiece). The measurement build (-DNM_MEASURE: stage-skipping switches, used with the ELU networks of scripts/) links ELU only.
template <class F> static int with_act(int act, F&& fn) {
#ifdef NM_MEASURE
  if (act != NM_ACT_ELU) return 1;
  return fn(std::integral_constant<int, NM_ACT_ELU>{});
#else
  return nmact::dispatch(act, fn);
#endif
}
int launch_act(const float* wp, const float* bp, const float* stdv, const float* obs, int N, uint64_t seed, const int64_t* iter_dev, int step, const ActOut& o,
               int act, hipStream_t s) {
  return with_act(act, [&](auto ACT) { return RollKernels<decltype(ACT)::value>::act(wp, bp, stdv, obs, N, seed, iter_dev, step, o, s); });
}
// the closing launches of a K-step launch: k_rollout_tail, then k_rollout_clear
static int launch_tail(const TailArgs& t, hipStream_t s) {
  hipLaunchKernelGGL(k_rollout_tail, dim3(min((t.N + 255) / 256, 64)), dim3(256), 0, s, t);
  if (hipGetLastError() != hipSuccess) return 1;
  hipLaunchKernelGGL(k_rollout_clear, dim3((t.K * nm::kNREW + 255) / 256), dim3(256), 0, s, t.K, t.st_sum, t.st_cnt);
  return hipGetLastError() != hipSuccess;
}
int launch_rollout(const nm::Model<float>* M_dev, const nm::Args<float>& a, const RollArgs& R, const TailArgs& t, int act, int level, hipStream_t s) {
  if (with_act(act, [&](auto ACT) { return RollKernels<decltype(ACT)::value>::rollout(M_dev, a, R, level, s); })) return 1;
  return launch_tail(t, s);
}
int launch_act_priv(const float* wp, const float* bp, const float* stdv, const float* rows, int N, uint64_t seed, const int64_t* iter_dev, int step, const ActOut& o,
                    float* prefix_store, int act, hipStream_t s) {
  return with_act(act, [&](auto ACT) { return RollPrivKernels<decltype(ACT)::value>::act(wp, bp, stdv, rows, N, seed, iter_dev, step, o, prefix_store, s); });
}
int launch_rollout_priv(const nm::Model<float>* M_dev, const nm::Args<float>& a, const RollPrivArgs& R, const TailArgs& t, int act, int level, hipStream_t s) {
  if (with_act(act, [&](auto ACT) { return RollPrivKernels<decltype(ACT)::value>::rollout(M_dev, a, R, level, s); })) return 1;
  return launch_tail(t, s);
}
// nm_play: the same closing launches. Without the bootstrap (t.gamma < 0) k_rollout_tail needs each env's LATEST time-out step only: the
// time-out buffer is refreshed by the last step in which some env reset, and an env's flag there is "it timed out in that very step".
int launch_play(const nm::Model<float>* M_dev, const nm::Args<float>& a, const PlayArgs& P, const TailArgs& t, int act, int level, hipStream_t s) {
  if (with_act(act, [&](auto ACT) { return PlayKernels<decltype(ACT)::value>::play(M_dev, a, P, level, s); })) return 1;
  return launch_tail(t, s);
}
// nm_step_tape: k_env_tape (nm_tape.hip) and the closing launches of nm_play - the books are the same
int launch_tape(const nm::Model<float>* M_dev, const nm::Args<float>& a, const TapeArgs& T, const TailArgs& t, int level, hipStream_t s) {
  if (tape_kernel(M_dev, a, T, level, s)) return 1;
  return launch_tail(t, s);
}

}  // namespace nmr
