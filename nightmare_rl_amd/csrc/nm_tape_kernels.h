// nm_tape_kernels.h - k_env_tape: K x env.step per launch with the actions of step t read from row t of a [K,N,18] device tape. The third
// kernel around nm::wave_step, compiled in a translation unit of its own (nm_tape.hip; nm_rollout_kernels.h says what sharing a unit
// does to the register allocation).
//
// The loop of the reference's custom_play.py:66-76 - and of every caller that already has its actions (a recorded action log, a fixed
// action stream, joint targets commanded on the real robot) - `for a in actions: env.step(a)` (envs/nightmare_v3_env.py:145-311) for every
// env at once, on the wave code of the rollout: the wave that owns two envs re-points the env step's action pointer to the next tape row
// and goes straight into nm::wave_step. Against k_env_play there is no policy and no sampling; the tape is written by an earlier launch on
// the same stream, so nothing inside the kernel orders it. Optionally every step files what it returned: the observation in row t of a
// [K,N,66] record (the step's observation pointer is re-pointed there), reward and reset flag in [K,N] rows (filed by the episode books).
// K is not limited by the episode length; the books (nm_env_loop.h) are play's.
#include <hip/hip_runtime.h>

#include "nm_env_loop.h"

#ifndef NM_WAVES_PER_SIMD
#define NM_WAVES_PER_SIMD 2
#endif

namespace nmr {

// The bookkeeping of step t - 1 (t > 0) and the launch arguments of env step t. Out of line, like play_step: nothing of it is live across
// the physics. WX: the launch carries the wrench schedule (level 7 alone).
template <bool WX>
__device__ __noinline__ void tape_step(const TapeArgs* Ts, nm::Args<float>* As, int t, int wave, uint64_t noise0) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // state rows, observation, reward / done / time-out of the previous step: stored
  if (t > 0) {
    BookRegs rec;
    books_load(rec, Ts, As, wave);
    books_file(rec, Ts, As, t - 1, wave);
    step_reset_noise(Ts, As, rec.d, wave);           // the reset draw of step t - 1, before the push of step t
    step_reset_rows(Ts, As, rec.d, wave);            // and the re-draw of its per-env rows
    // the sensor model of step t - 1: the sensed row into its record row, or (null) into the env's own buffer
    step_sensor(Ts, As, Ts->rec_obs ? Ts->rec_obs + (size_t)(t - 1) * As->N * nm::kNOBS : nullptr, rec.d, wave);
  }
  if (threadIdx.x == 0) {
    const size_t so = (size_t)t * As->N;
    As->actions = Ts->tape + so * nm::kNU;
    if (Ts->rec_obs && Ts->sensor.on == 0) As->obs = Ts->rec_obs + so * nm::kNOBS;      // (sensor model on: the true-obs buffer, set by the launcher)
    step_args(As, Ts, t, noise0);
  }
  step_push(Ts, As, t, wave);
  if constexpr (WX) step_wrench(As, t, wave);
  step_close();
}

template <int EP>      // EP: level of per-env physics parameters, above 0 launched only while rows are set (nm_core.h env_mu)
__global__ void __launch_bounds__(64, NM_WAVES_PER_SIMD) k_env_tape(const nm::Model<float>* __restrict__ Mp, nm::Args<float> A, TapeArgs T) {
  __shared__ typename nm::ShWSel<float, 2, EP>::type shl;
  nm::ShW<float, 2>& sh = nm::ShWSel<float, 2, EP>::images(shl);
  __shared__ nm::Model<float> Ms;
  __shared__ nm::Args<float> As;
  __shared__ TapeArgs Ts;
  int wave;
  if (!loop_begin(Mp, A, T, Ms, As, Ts, wave)) return;
  const uint64_t noise0 = A.noise_step;
  const int K = T.K;
  for (int t = 0; t < K; t++) {
    tape_step<(EP >= 7)>(&Ts, &As, t, wave, noise0);             // (+ the bookkeeping of step t - 1)
    nm::wave_step<float, 2, EP>(sh, Ms, As, wave);        // env.step: load, decimation x mj_step, epilogue - the code of k_env_step
  }
  books_last(&Ts, &As, K - 1, wave);
  step_sensor_last(&Ts, &As, Ts.rec_obs ? Ts.rec_obs + (size_t)(K - 1) * As.N * nm::kNOBS : nullptr, wave);     // the last step's sensed row
}

int tape_kernel(const nm::Model<float>* M_dev, const nm::Args<float>& a, const TapeArgs& T, int level, hipStream_t s) {
  nmrows::with_level(level, [&](auto L) { hipLaunchKernelGGL(k_env_tape<decltype(L)::value>, dim3((a.N + 1) / 2), dim3(64), 0, s, M_dev, a, T); });
  return hipGetLastError() != hipSuccess;
}

}  // namespace nmr
