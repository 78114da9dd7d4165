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

#include "nm_core.h"
#include "nm_rollout.h"

#ifndef NM_PLAY_ACT
#error "define NM_PLAY_ACT (an NM_ACT_* code) before including nm_play_kernels.h"
#endif
#ifndef NM_WAVES_PER_SIMD
#define NM_WAVES_PER_SIMD 2
#endif

namespace nmr {

// The bookkeeping a viewer-less play.py wants for this wave's envs, in two halves like the rollout's record: cur_ret / cur_len / fin3 exactly
// as nm_ppo_record keeps them, and per env the sum and the number of the returns of the episodes it finished (the wave owns the env: plain
// load / add / store in step order, no atomics).
struct PlayRegs { float rw, to, cr, cl, rs, rc; long long d; };
__device__ __forceinline__ void play_record_load(PlayRegs& r, const PlayArgs* Ps, const nm::Args<float>* As, int wave) {
  const int lane = threadIdx.x, e = min(wave * 2 + (lane & 1), As->N - 1);
  r.rw = simt::gld1(As->rew, e); r.d = simt::gld1(As->done, e); r.to = simt::gld1(As->timeout_now, e);
  r.cr = simt::gld1((const float*)Ps->cur_ret, e); r.cl = simt::gld1((const float*)Ps->cur_len, e);
  r.rs = simt::gld1((const float*)Ps->ret_sum, e); r.rc = simt::gld1((const float*)Ps->ret_cnt, e);
}
__device__ __forceinline__ void play_record_file(const PlayRegs& r, const PlayArgs* Ps, const nm::Args<float>* As, int t, int wave) {
  const int lane = threadIdx.x, N = As->N, e = wave * 2 + lane;
  if (lane < 2 && e < N) {
    float cr = r.cr + r.rw, cl = r.cl + 1.0f;
    if (r.d > 0) {
      atomicAdd(Ps->fin3, cr); atomicAdd(Ps->fin3 + 1, cl); atomicAdd(Ps->fin3 + 2, 1.0f);
      simt::gst1(Ps->ret_sum, (size_t)e, r.rs + cr); simt::gst1(Ps->ret_cnt, (size_t)e, r.rc + 1.0f);
      cr = 0.f; cl = 0.f;
    }
    simt::gst1(Ps->cur_ret, (size_t)e, cr); simt::gst1(Ps->cur_len, (size_t)e, cl);
    if (r.to != 0.f) simt::gst1(Ps->to_step, (size_t)e, t);       // a later time-out of the same env overwrites: the latest one counts
    if (Ps->rec_done && e == Ps->rec_env) simt::gst1(Ps->rec_done, (size_t)t, (unsigned char)(r.d > 0 ? 1 : 0));
  }
}
// The bookkeeping of step t - 1 (t > 0) and the policy of step t for the wave's envs + the launch arguments of the env step that follows.
// Out of line, like the rollout's policy_step: its registers are not live across the physics.
template <class S, int ACT>
__device__ __noinline__ void play_step(float* xb, const PlayArgs* Ps, nm::Args<float>* As, int t, int wave, uint64_t noise0) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // state rows, observation, reward / done / time-out of the previous step: stored
  PlayRegs rec;
  if (t > 0) play_record_load(rec, Ps, As, wave);
  ActOut o{Ps->actions, nullptr, nullptr, nullptr, nullptr, nullptr};
  policy_wave<S, ACT, kPolicyPlay>(xb, Ps->wp, Ps->bp, Ps->stdv, t == 0 ? Ps->obs0 : (const float*)Ps->obs, As->N, wave, Ps->seed,
                                   (uint64_t)simt::gld1(Ps->iter_dev, 0) * 4096ull + Ps->step0 + (uint64_t)t, o, Ps->deterministic != 0);
  if (t > 0) play_record_file(rec, Ps, As, t - 1, wave);
  if (threadIdx.x == 0) {
    As->stat_sum = Ps->st_sum + (size_t)t * nm::kNREW;
    As->stat_cnt = Ps->st_cnt + (size_t)t * 4;
    As->noise_step = noise0 + (uint64_t)t;
    As->rec = Ps->rec_log ? Ps->rec_log + (size_t)t * kRecRow : nullptr;           // the state log's row of this step (env.py:261-272)
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the actions are in L2 before the load stage asks for them (other lanes of this wave)
  nm::wave_sync();
}
__device__ __noinline__ void play_record_last(const PlayArgs* Ps, const nm::Args<float>* As, int t, int wave) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  PlayRegs rec;
  play_record_load(rec, Ps, As, wave);
  play_record_file(rec, Ps, As, t, wave);
}

template <class S, int ACT>
__global__ void __launch_bounds__(64, NM_WAVES_PER_SIMD) k_env_play(const nm::Model<float>* __restrict__ Mp, nm::Args<float> A, PlayArgs P) {
  __shared__ nm::ShW<float, 2> sh;
  __shared__ nm::Model<float> Ms;
  __shared__ nm::Args<float> As;
  __shared__ PlayArgs Ps;
  static_assert(sizeof(sh) >= kXFloats * sizeof(float), "the policy's activation rows alias the env images");
  int wave = blockIdx.x;
#ifndef NM_NO_XCD_MAP
  {
    const int nwx = (int)gridDim.x >> 3;
    if (A.nxcd == 8 && wave < (nwx << 3)) wave = (wave & 7) * nwx + (wave >> 3);
  }
#endif
  if (wave * 2 >= A.N) return;
  As = A;                                             // (A.actions = P.actions, A.obs = P.obs for every step: set by the host)
  Ps = P;
  __syncthreads();
  {  // the model constants: L2 -> LDS, once for the whole launch
    const uint32_t* src = reinterpret_cast<const uint32_t*>(Mp);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&Ms);
    constexpr int kWords = (int)(sizeof(nm::Model<float>) / 4);
    for (int i = threadIdx.x; i < kWords; i += 64) dst[i] = src[i];
    __syncthreads();
  }
  float* xb = reinterpret_cast<float*>(&sh);          // between two steps the env images hold nothing that is needed (env_load2 rewrites them)
  if ((int)threadIdx.x < 2 && wave * 2 + (int)threadIdx.x < A.N) P.to_step[wave * 2 + threadIdx.x] = -1;
  const uint64_t noise0 = A.noise_step;
  const int K = P.K;
  for (int t = 0; t < K; t++) {
    play_step<S, ACT>(xb, &Ps, &As, t, wave, noise0);     // (+ the bookkeeping of step t - 1)
    nm::wave_step<float, 2>(sh, Ms, As, wave);        // env.step: load, decimation x mj_step, epilogue - the code of k_env_step
  }
  play_record_last(&Ps, &As, K - 1, wave);
}

template <int ACT>
int PlayKernels<ACT>::play(const nm::Model<float>* M_dev, const nm::Args<float>& a, const PlayArgs& P, hipStream_t s) {
  hipLaunchKernelGGL((k_env_play<RefShape, ACT>), dim3((a.N + 1) / 2), dim3(64), 0, s, M_dev, a, P);
  return hipGetLastError() != hipSuccess;
}
template struct PlayKernels<NM_PLAY_ACT>;

}  // namespace nmr
