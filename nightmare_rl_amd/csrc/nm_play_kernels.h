// nm_play_kernels.h - k_env_play: K x [policy, env.step] per launch with NOTHING collected for PPO, for ONE hidden activation: included by
// nm_play_<activation>.hip, each a translation unit of its own that defines NM_PLAY_ACT (an NM_ACT_* code) first (one unit per kernel
// around nm::wave_step: nm_rollout_kernels.h says what sharing a unit does to the register allocation).
//
// The loop of the reference's play.py:118-132 (`actions = nn.act(obs)` -> scale / clip -> servo command -> mj_step x decimation, in a
// viewer loop) for every env at once, on the wave code of the rollout: the wave that owns two envs evaluates the policy on the
// observation its previous step left, files the actions - the mean (`deterministic`, rsl_rl's act_inference) or mean + std * z with the
// keys of nm_rollout_act - and goes straight into nm::wave_step. Against k_env_rollout there is no rollout storage (one [N,66]
// observation buffer that the wave's own next act reads back, one [N,18] action buffer), no log-probability, value, mu or sigma row, no
// time-out bootstrap, no value of the last observation; the critic half of the merged network is still multiplied (its blocks share the
// actor's MFMA instructions: nm_rollout.h) but nothing of it is stored. K is not limited by the episode length: an env may time out
// several times per launch, and only its latest time-out step is kept (launch_play in nm_rollout.hip says why that is enough).
#include <hip/hip_runtime.h>

#include "nm_env_loop.h"

#ifndef NM_PLAY_ACT
#error "define NM_PLAY_ACT (an NM_ACT_* code) before including nm_play_kernels.h"
#endif
#ifndef NM_WAVES_PER_SIMD
#define NM_WAVES_PER_SIMD 2
#endif

namespace nmr {

// The rollout's policy_step with three differences: the policy files the actions only (kPolicyPlay: the mean itself when deterministic),
// its noise key starts at step0, and the env step's action and observation buffers are the same for every step (set by the host), so
// the act of step t reads back what this wave's step t - 1 wrote into P.obs. The episode books (nm_env_loop.h) are play's: no storage rows.
// Out of line, like policy_step: its registers are not live across the physics. WX: the launch carries the wrench schedule (level 7 alone).
template <class S, int ACT, bool WX>
__device__ __noinline__ void play_step(float* xb, const PlayArgs* Ps, nm::Args<float>* As, int t, int wave, uint64_t noise0) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // state rows, observation, reward / done / time-out of the previous step: stored
  BookRegs rec;
  if (t > 0) books_load(rec, Ps, As, wave);
  if (t > 0) step_sensor(Ps, As, Ps->obs, rec.d, wave);      // the sensor model of step t - 1 (the step filed the true row where the launcher pointed it): the sensed row act t reads
  ActOut o{Ps->actions, nullptr, nullptr, nullptr, nullptr, nullptr};
  policy_wave<S, ACT, kPolicyPlay>(xb, Ps->wp, Ps->bp, Ps->stdv, t == 0 ? Ps->obs0 : (const float*)Ps->obs, As->N, wave, Ps->seed,
                                   (uint64_t)simt::gld1(Ps->iter_dev, 0) * 4096ull + Ps->step0 + (uint64_t)t, o, Ps->deterministic != 0);
  if (t > 0) { books_file(rec, Ps, As, t - 1, wave); step_reset_noise(Ps, As, rec.d, wave); step_reset_rows(Ps, As, rec.d, wave); }   // the reset draw of step t - 1, before the push of step t
  if (threadIdx.x == 0) step_args(As, Ps, t, noise0);
  step_push(Ps, As, t, wave);
  if constexpr (WX) step_wrench(As, t, wave);
  step_close();
}

template <class S, int ACT, int EP>      // EP: level of per-env physics parameters, above 0 launched only while rows are set (nm_core.h env_mu)
__global__ void __launch_bounds__(64, NM_WAVES_PER_SIMD) k_env_play(const nm::Model<float>* __restrict__ Mp, nm::Args<float> A, PlayArgs P) {
  __shared__ typename nm::ShWSel<float, 2, EP>::type shl;
  nm::ShW<float, 2>& sh = nm::ShWSel<float, 2, EP>::images(shl);
  __shared__ nm::Model<float> Ms;
  __shared__ nm::Args<float> As;
  __shared__ PlayArgs Ps;
  static_assert(sizeof(sh) >= kXFloats * sizeof(float), "the policy's activation rows alias the env images");
  int wave;
  if (!loop_begin(Mp, A, P, Ms, As, Ps, wave)) return;     // (A.actions = P.actions, A.obs = P.obs for every step: set by the host)
  float* xb = reinterpret_cast<float*>(&sh);          // between two steps the env images hold nothing that is needed (env_load2 rewrites them)
  const uint64_t noise0 = A.noise_step;
  const int K = P.K;
  for (int t = 0; t < K; t++) {
    play_step<S, ACT, (EP >= 7)>(xb, &Ps, &As, t, wave, noise0);     // (+ the bookkeeping of step t - 1)
    nm::wave_step<float, 2, EP>(sh, Ms, As, wave);        // env.step: load, decimation x mj_step, epilogue - the code of k_env_step
  }
  books_last(&Ps, &As, K - 1, wave);
  step_sensor_last(&Ps, &As, Ps.obs, wave);     // the last step's sensed row
}

template <int ACT>
int PlayKernels<ACT>::play(const nm::Model<float>* M_dev, const nm::Args<float>& a, const PlayArgs& P, int level, hipStream_t s) {
  nmrows::with_level(level, [&](auto L) { hipLaunchKernelGGL((k_env_play<RefShape, ACT, decltype(L)::value>), dim3((a.N + 1) / 2), dim3(64), 0, s, M_dev, a, P); });
  return hipGetLastError() != hipSuccess;
}
template struct PlayKernels<NM_PLAY_ACT>;

}  // namespace nmr
