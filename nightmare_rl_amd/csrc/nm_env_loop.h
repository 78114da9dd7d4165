// nm_env_loop.h - what the K-step launches k_env_rollout (nm_rollout_kernels.h), k_env_play (nm_play_kernels.h) and k_env_tape
// (nm_tape_kernels.h) share: the wave index, the launch prologue, the episode books of the wave's two envs, the per-step update of the
// env step's launch arguments, the push perturbation of a step (nm_push.h), the wrench schedule of a step (nm_wrench.h), the reset draw of a step (nm_reset_noise.h), the re-draw of its per-env rows (nm_reset_rows.h) and the sensor model of a step (nm_sensor.h). X below is the launch's own argument struct, RollArgs, PlayArgs or TapeArgs (nm_rollout.h): the helpers read
// the fields all carry (cur_ret, cur_len, fin3, to_step, st_sum, st_cnt, rec_log) and `if constexpr` on the struct's traits (kPlayBooks,
// kStepRecord) decides what only some of them file.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "nm_core.h"
#include "nm_env_rows.h"     // with_level: the launchers of the three K-step kernels pick the step's level through it
#include "nm_push.h"
#include "nm_reset_noise.h"
#include "nm_reset_rows.h"
#include "nm_rollout.h"
#include "nm_sensor.h"
#include "nm_wrench.h"

namespace nmr {

// XCD-aware block -> wave mapping: the dispatcher deals workgroups round-robin over the 8 XCDs (block b runs on XCD b % 8), each with
// its own L2. Consecutive envs share cache lines (rows of 100 / 96 / 72 bytes), so each XCD takes a CONTIGUOUS eighth of the waves:
// a line's bytes are then written through one L2 instead of being merged in memory from two.
__device__ __forceinline__ int wave_index(int nxcd) {
  int wave = blockIdx.x;
#ifndef NM_NO_XCD_MAP
  {
    const int nwx = (int)gridDim.x >> 3;          // workgroups per XCD (the remainder, if any, keeps the identity mapping)
    if (nxcd == 8 && wave < (nwx << 3)) wave = (wave & 7) * nwx + (wave >> 3);   // other partition modes (CPX, DPX): identity
  }
#endif
  return wave;
}

// The first lines of a K-step launch: the wave's index, the launch arguments and the model constants into the workgroup's LDS (once for
// all K steps), "no time-out yet" for the wave's envs. false: the wave has no env and leaves.
template <class X>
__device__ __forceinline__ bool loop_begin(const nm::Model<float>* __restrict__ Mp, const nm::Args<float>& A, const X& R, nm::Model<float>& Ms,
                                           nm::Args<float>& As, X& Rs, int& wave) {
  wave = wave_index(A.nxcd);
  if (wave * 2 >= A.N) return false;
  As = A;
  Rs = R;
  __syncthreads();
  {  // the model constants: L2 -> LDS
    const uint32_t* src = reinterpret_cast<const uint32_t*>(Mp);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&Ms);
    constexpr int kWords = (int)(sizeof(nm::Model<float>) / 4);
    for (int i = threadIdx.x; i < kWords; i += 64) dst[i] = src[i];
    __syncthreads();
  }
  if ((int)threadIdx.x < 2 && wave * 2 + (int)threadIdx.x < A.N) R.to_step[wave * 2 + threadIdx.x] = -1;
  return true;
}

// PPO.process_env_step + the runner's bookkeeping for this wave's envs (k_ppo_record's arithmetic), in two halves so that its loads travel
// with the next policy step's observation loads (one L2 round trip instead of two): `load` right after the step's stores have landed,
// `file` whenever the values are needed.
//   rollout: the transition's reward and done go into the storage rows of step t. The time-out bootstrap needs the step's
//            extras['time_outs'], a cross-wave quantity: k_rollout_tail adds it. An env times out at most once per launch.
//   play, tape: nothing is stored; per env the sum and the number of the returns of the episodes it finished (the wave owns the env:
//            plain load / add / store in step order, no atomics), the logged env's reset flag, and a later time-out of the same env
//            overwrites the earlier one's step. tape: the step's reward and reset flag also go into the caller's [K,N] record rows, if any.
struct BookRegs { float rw, to, cr, cl, rs, rc; long long d; };
template <class X>
__device__ __forceinline__ void books_load(BookRegs& r, const X* Xs, const nm::Args<float>* As, int wave) {
  const int lane = threadIdx.x, e = min(wave * 2 + (lane & 1), As->N - 1);
  // (global-memory accessors of simt.h: the pointers come out of LDS copies of the arguments - plain dereferences would be flat_load)
  r.rw = simt::gld1(As->rew, e); r.d = simt::gld1(As->done, e); r.to = simt::gld1(As->timeout_now, e);
  r.cr = simt::gld1((const float*)Xs->cur_ret, e); r.cl = simt::gld1((const float*)Xs->cur_len, e);
  if constexpr (X::kPlayBooks) { r.rs = simt::gld1((const float*)Xs->ret_sum, e); r.rc = simt::gld1((const float*)Xs->ret_cnt, e); }
}
template <class X>
__device__ __forceinline__ void books_file(const BookRegs& r, const X* Xs, const nm::Args<float>* As, int t, int wave) {
  constexpr bool PLAY = X::kPlayBooks;
  const int lane = threadIdx.x, N = As->N, e = wave * 2 + lane;
  if (lane < 2 && e < N) {
    // (with the compiler this was written for, the place of this compare decides the order the scheduler gives the books' loads: each
    // launch keeps the place it had when the two were written apart, and with it its instruction stream. C++ promises nothing of the
    // kind: after a compiler upgrade the two places may mean nothing - then write the compare once, first)
    bool d;
    if constexpr (!PLAY) d = r.d > 0;
    float cr = r.cr + r.rw, cl = r.cl + 1.0f;
    if constexpr (PLAY) d = r.d > 0;
    if constexpr (!PLAY) {
      const size_t so = (size_t)t * N;
      simt::gst1(Xs->s_rewards, so + e, r.rw);
      simt::gst1(Xs->s_dones, so + e, (unsigned char)(d ? 1 : 0));
    }
    if constexpr (X::kStepRecord) {
      const size_t so = (size_t)t * N;
      if (Xs->rec_rew) simt::gst1(Xs->rec_rew, so + e, r.rw);
      if (Xs->rec_dones) simt::gst1(Xs->rec_dones, so + e, (unsigned char)(d ? 1 : 0));
    }
    if (d) {
      atomicAdd(Xs->fin3, cr); atomicAdd(Xs->fin3 + 1, cl); atomicAdd(Xs->fin3 + 2, 1.0f);
      if constexpr (PLAY) { simt::gst1(Xs->ret_sum, (size_t)e, r.rs + cr); simt::gst1(Xs->ret_cnt, (size_t)e, r.rc + 1.0f); }
      cr = 0.f; cl = 0.f;
    }
    simt::gst1(Xs->cur_ret, (size_t)e, cr); simt::gst1(Xs->cur_len, (size_t)e, cl);
    if (r.to != 0.f) simt::gst1(Xs->to_step, (size_t)e, t);
    if constexpr (PLAY)
      if (Xs->rec_done && e == Xs->rec_env) simt::gst1(Xs->rec_done, (size_t)t, (unsigned char)(d ? 1 : 0));
  }
}
// The reset draw of the step whose books were just filed (nm_reset_noise.h; X::rnoise), for the envs of this wave that the step reset:
// `d` is the done word books_load left in lanes 0 / 1 (env 2 wave + lane). Lanes 0..42 own the 43 columns of one env at a time, lane 0 its
// reset count. Called behind the wait at the head of the step function (or of books_last): that wait is what orders the draw behind the
// in-kernel qpos0 store of the same words, which other lanes of this wave issued in the epilogue of the step before. The body ends with
// a wait of its own, so that a push of the next step (other lanes again, qvel[0:2]) lands behind the draw, as it does in the per-step
// path; step_close's wait then puts everything in L2 before the load stage asks for the state. The test is wave-uniform; the body is
// out of line, like push_store: taken once per episode, and its registers are nobody else's.
template <class X>
__device__ __noinline__ void reset_noise_store(const X* Xs, const nm::Args<float>* As, int mask, int wave) {
  const int lane = threadIdx.x;
  mask = __builtin_amdgcn_readfirstlane(mask);
#pragma unroll 1
  for (int hh = 0; hh < 2; hh++) {
    const int env = wave * 2 + hh;
    if (!((mask >> hh) & 1) || env >= As->N) continue;
    const uint32_t k = simt::gld1((const uint32_t*)Xs->rnoise.count, (size_t)env);
    if (lane < nm::kResetCols)
      nm::reset_noise_apply<float>(As->qpos, As->qvel, Xs->rnoise.qpos0, Xs->rnoise.p, As->seed, (uint64_t)(As->env_offset + env), (size_t)env, k, lane);
    if (lane == 0) simt::gst1(Xs->rnoise.count, (size_t)env, k + 1u);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
template <class X>
__device__ __forceinline__ void step_reset_noise(const X* Xs, const nm::Args<float>* As, long long d, int wave) {
  if (__builtin_amdgcn_readfirstlane(Xs->rnoise.on) == 0) return;
  const int mask = (int)(__builtin_amdgcn_ballot_w64(d > 0) & 3ull);
  if (mask) reset_noise_store(Xs, As, mask, wave);
}
// The re-draw of the per-env rows of the step whose books were just filed (nm_reset_rows.h; X::rrows), for the envs of this wave that the
// step reset, called right behind step_reset_noise with the same done word and the same wave-uniform test. Lanes 0..40 own the 41 words
// of one env at a time, lane 0 its reset-row count; the pools and their sizes are read from the env object's descriptor in device memory.
// The load stage of wave_step reads every row with vector loads (gldv / gldx), once per step, through the same L1 these vector stores
// write through: the wait at the head of the step function (or of books_last) is behind the previous step's loads of the same rows, the
// body ends with a wait of its own, and step_close's wait puts the stores in L2 before the load stage asks for the rows. The resetting
// step itself ran on the old rows. Out of line, like reset_noise_store: taken once per episode, and its registers are nobody else's.
template <class X>
__device__ __noinline__ void reset_rows_store(const X* Xs, const nm::Args<float>* As, int mask, int wave) {
  const int lane = threadIdx.x;
  mask = __builtin_amdgcn_readfirstlane(mask);
#pragma unroll 1
  for (int hh = 0; hh < 2; hh++) {
    const int env = wave * 2 + hh;
    if (!((mask >> hh) & 1) || env >= As->N) continue;
    const uint32_t k = simt::gld1((const uint32_t*)Xs->rrows.count, (size_t)env);
    if (lane < nm::kResetRowWords)
      nm::reset_rows_apply<float>(*As, Xs->rrows.desc, As->seed, (uint64_t)(As->env_offset + env), (size_t)env, k, lane);
    if (lane == 0) simt::gst1(Xs->rrows.count, (size_t)env, k + 1u);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
template <class X>
__device__ __forceinline__ void step_reset_rows(const X* Xs, const nm::Args<float>* As, long long d, int wave) {
  if (__builtin_amdgcn_readfirstlane(Xs->rrows.on) == 0) return;
  const int mask = (int)(__builtin_amdgcn_ballot_w64(d > 0) & 3ull);
  if (mask) reset_rows_store(Xs, As, mask, wave);
}
// The sensor model of the step that just ended (nm_sensor.h; X::sensor), for the wave's two envs: the true row the step filed in the env's
// true-obs buffer (where Args::obs points for the whole launch while the model is on) -> ring, count and the sensed row in `dst` [N,66]
// (null: the descriptor's `out`, the env's own buffer). `d` is the done word of that step in lanes 0 / 1 (env 2 wave + lane), as
// books_load leaves it. The 2 x 66 columns are split over the lanes in three rounds; an env past N on an odd last wave files nothing.
// Called behind the wait at the head of the step function (or behind books_last, which waits): the step's observation and done stores,
// issued by other lanes of this wave, have landed. Both counts are loaded before any round runs, and the store of a new count needs the
// loaded value, so every lane has read the count by then; a delayed read takes another ring slot than the one the round pushes into.
// The body ends with a wait of its own: the policy's (or priv_gather's) loads of the sensed row, by other lanes of this wave through
// the same L1, come behind the stores, and so does the next step's push into the ring. Within a launch only the wave that owns the env
// touches its ring and count; across launches, and against k_sensor, stream order covers it. The test is wave-uniform; the body is out
// of line, like reset_noise_store: while the model is off the step pays one scalar compare, and the body's registers are nobody else's.
template <class X>
__device__ __noinline__ void sensor_store(const X* Xs, const nm::Args<float>* As, float* dst, int mask, int wave) {
  const int lane = threadIdx.x, N = As->N;
  mask = __builtin_amdgcn_readfirstlane(mask);
  const nm::SensorDesc* dp = Xs->sensor.desc;
  nm::SensorDesc D;
  D.delay = simt::gld1(&dp->delay, 0); D.bias = simt::gld1(&dp->bias, 0); D.ring = simt::gld1(&dp->ring, 0); D.count = simt::gld1(&dp->count, 0);
  D.true_obs = simt::gld1(&dp->true_obs, 0); D.out = simt::gld1(&dp->out, 0); D.clip_obs = simt::gld1(&dp->clip_obs, 0); D.pad = 0;
  if (!dst) dst = D.out;
  // (lanes 0 / 1 load the two counts, as books_load loads the done words: a per-lane address is a vector load, whose L1 sees this wave's stores)
  const int nl = (int)simt::gld1((const uint32_t*)D.count, (size_t)min(wave * 2 + (lane & 1), N - 1));
  const uint32_t n0 = (uint32_t)__builtin_amdgcn_readlane(nl, 0), n1 = (uint32_t)__builtin_amdgcn_readlane(nl, 1);
#pragma unroll 1
  for (int i = 0; i < (2 * nm::kNOBS + 63) / 64; i++) {
    const int idx = lane + 64 * i, e = idx >= nm::kNOBS ? 1 : 0, c = idx - e * nm::kNOBS, env = wave * 2 + e;
    if (idx < 2 * nm::kNOBS && env < N) nm::sensor_apply(D, (size_t)env, c, e ? n1 : n0, ((mask >> e) & 1) != 0, dst);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
template <class X>
__device__ __forceinline__ void step_sensor(const X* Xs, const nm::Args<float>* As, float* dst, long long d, int wave) {
  if (__builtin_amdgcn_readfirstlane(Xs->sensor.on) == 0) return;
  sensor_store(Xs, As, dst, (int)(__builtin_amdgcn_ballot_w64(d > 0) & 3ull), wave);
}
// the same behind books_last, which keeps the done word to itself: lanes 0 / 1 load it again
template <class X>
__device__ __forceinline__ void step_sensor_last(const X* Xs, const nm::Args<float>* As, float* dst, int wave) {
  if (__builtin_amdgcn_readfirstlane(Xs->sensor.on) == 0) return;
  const long long d = simt::gld1(As->done, (size_t)min(wave * 2 + ((int)threadIdx.x & 1), As->N - 1));
  sensor_store(Xs, As, dst, (int)(__builtin_amdgcn_ballot_w64(d > 0) & 3ull), wave);
}
// the books of the launch's last step (no policy step follows it)
template <class X>
__device__ __noinline__ void books_last(const X* Xs, const nm::Args<float>* As, int t, int wave) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  BookRegs rec;
  books_load(rec, Xs, As, wave);
  books_file(rec, Xs, As, t, wave);
  step_reset_noise(Xs, As, rec.d, wave);             // a reset at the launch's last step
  step_reset_rows(Xs, As, rec.d, wave);
}

// The launch arguments of env step t that every K-step launch sets (lane 0, after the policy of step t), and what closes the policy step.
template <class X>
__device__ __forceinline__ void step_args(nm::Args<float>* As, const X* Xs, int t, uint64_t noise0) {
  As->stat_sum = Xs->st_sum + (size_t)t * nm::kNREW;
  As->stat_cnt = Xs->st_cnt + (size_t)t * 4;
  As->noise_step = noise0 + (uint64_t)t;
  As->rec = Xs->rec_log ? Xs->rec_log + (size_t)t * kRecRow : nullptr;           // the state log's row of this step (env.py:261-272)
}
// The push of env step t, if one is due (nm_push.h; X::push says when): lanes 0..3 of the wave own (env 2 wave + (lane >> 1), axis lane & 1)
// and store their draw into qvel. Called after the wait at the head of the policy step (the previous step's state rows of this wave
// are stored - and a store of the same lane to the same word stays behind them anyway) and before step_close, whose wait puts the push
// in L2 before the load stage of wave_step asks for qvel; at t = 0 stream order covers the previous launch. The branch is wave-uniform.
// Out of line, like books_last: taken once per `interval` steps, and its registers are nobody else's.
template <class X>
__device__ __noinline__ void push_store(const X* Xs, const nm::Args<float>* As, uint32_t q, int wave) {
  const int lane = threadIdx.x, env = wave * 2 + (lane >> 1);
  if (lane < 4 && env < As->N)
    simt::gst1(As->qvel, (size_t)env * nm::kNV + (lane & 1),
               nm::push_value<float>(As->seed, (uint64_t)(As->env_offset + env), Xs->push.ctr0 + 2u * q + (uint32_t)(lane & 1), Xs->push.maxv));
}
template <class X>
__device__ __forceinline__ void step_push(const X* Xs, const nm::Args<float>* As, int t, int wave) {
  const uint32_t iv = (uint32_t)__builtin_amdgcn_readfirstlane(Xs->push.interval);
  if (iv == 0) return;
  const uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)Xs->push.phase) + (uint32_t)t, q = p / iv;
  if (q * iv == p && (t > 0 || __builtin_amdgcn_readfirstlane(Xs->push.past0) != 0)) push_store(Xs, As, q, wave);
}
// The wrench schedule of env step t, if the step opens or closes a window (nm_wrench.h; the WrenchArgs behind the env's wrench rows say
// when - written by the launcher in front of this launch, read here through the scalar-uniform gld1): lanes 0..11 of the wave own
// (env 2 wave + lane / 6, axis lane % 6) and store their draw, or zero, into the env's wrench row. Called next to step_push, after the
// wait at the head of the policy step: the load stage of the step before read the row with vector loads (gldx) whose values it has long
// consumed, through the same L1 these vector stores write through, and step_close's wait puts the stores in L2 before the load stage of
// this step asks for the row; at t = 0 stream order covers the previous launch. Only the level-7 kernels call it, and the host writes
// interval = 0 unless the schedule is on. The branch is wave-uniform. Out of line, like push_store: taken twice per `interval`
// steps at most, and its registers are nobody else's.
static __device__ __noinline__ void wrench_store(const WrenchArgs* W, const nm::Args<float>* As, uint32_t q, int draw, int wave) {
  const int lane = threadIdx.x, half = lane >= 6 ? 1 : 0, axis = lane - 6 * half, env = wave * 2 + half;
  if (lane < 12 && env < As->N) {
    float v = 0.0f;
    if (draw) v = nm::wrench_value<float>(As->seed, (uint64_t)(As->env_offset + env), simt::gld1(&W->q0, 0) + q, axis, simt::gld1(W->maxv, (size_t)axis));
    simt::gst1(const_cast<float*>(nm::wrench_rows_of(*As)), (size_t)env * nm::kWrenchP + nm::wrench_word(axis), v);
  }
}
__device__ __forceinline__ void step_wrench(const nm::Args<float>* As, int t, int wave) {
  const WrenchArgs* W = static_cast<const WrenchArgs*>(nm::wrench_args_of(*As));
  const uint32_t iv = (uint32_t)__builtin_amdgcn_readfirstlane(simt::gld1(&W->interval, 0));
  if (iv == 0) return;
  const uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)simt::gld1(&W->phase, 0)) + (uint32_t)t, dq = p / iv, r = p - dq * iv;
  const uint32_t du = (uint32_t)__builtin_amdgcn_readfirstlane(simt::gld1(&W->duration, 0));
  if ((r == 0 || (du < iv && r == du)) && (dq > 0 || __builtin_amdgcn_readfirstlane(simt::gld1(&W->past0, 0)) != 0)) wrench_store(W, As, dq, r == 0, wave);
}
__device__ __forceinline__ void step_close() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the actions are in L2 before the load stage asks for them (other lanes of this wave)
  nm::wave_sync();
}

}  // namespace nmr
