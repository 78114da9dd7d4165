// nm_reset_rows.h - per-env randomisation rows re-drawn at every reset, from pools (Isaac Lab's `mode="reset"` events, legged_gym's
// per-reset payload; it replaces nothing upstream: the reference has one robot, one floor and ideal servos). Each of the six kinds of
// nmrows::Kind (nm_env_rows.h) may own a POOL of P rows in the env's dtype, 1 <= P <= 65536, a pool row holding exactly the words of that
// kind's per-env row:
//     kind      words   lanes    the env's row
//     kFric     4       0..3     envp + env kEnvP                  (mu, p_gain, kv, pad)
//     kBody     20      4..23    envp + N kEnvP + env kBodyP
//     kLat      1       24       lat_delay[env]                    (a 4-byte int in either dtype)
//     kGrav     8       25..32   grav_rows_of + env kGravP
//     kServo    4       33..36   servo_rows_of + env kServoP
//     kTorque   4       37..40   torque_rows_of + env kTorqueP
// 41 words, one lane each. While a kind has a pool, an env's reset - time-out, termination or a host reset_idx; not the bad-state reset
// inside the physics, and nm_step_physics never resets - overwrites that kind's row of that env with pool row
//     i = (rand_u24_bits(seed + kResetRowsKey, global env id, 8 k + kind) * P) >> 24          (64-bit integers: k_latency_draw's rule)
// the counter in 32 bits (it wraps at k = 2^29). A pool has no arithmetic: fp32 and fp64, host and device agree bit for bit by
// construction, the kinds whose rows the host derives (payload, gravity) work like the others, and correlated parameters - measured
// servo units - are expressible. k is the env's reset-row count, a device uint32 [N] buffer of its own (not the reset-noise count: the
// two features are switched on at different times), read by every lane of the env and then incremented by one - by the env's one owner:
//   * per-step path: k_reset_rows, launched on the step's stream right behind k_env_step while any pool is installed; it reads done[env]
//     on the device, so there is no host decision and the launches can be captured into a graph
//   * nm_reset: k_reset_rows behind k_reset, for the ids it reset (distinct ids: a repeated id would have two owners)
//   * K-step launches: nmr::step_reset_rows (nm_env_loop.h) inside the wave that owns the env, parameters in nmr::ResetRowsArgs
// The new rows hold from the first step of the new episode: the resetting step ran on the old rows and returns the terminal observation.
// The action history and the servo's limited targets are state and keep what they hold. A pool of one row equal to the rows every env
// holds is the feature off, bit for bit. The key is the global env id: sharding changes nothing.
#pragma once
#include <stdint.h>

#include "nm_core.h"

namespace nm {

constexpr uint64_t kResetRowsKey = 0x524553414D50ull;     // "RESAMP"
constexpr int kResetRowKinds = 6, kResetRowWords = kEnvP + kBodyP + 1 + kGravP + kServoP + kTorqueP;
constexpr uint32_t kResetRowsMaxPool = 65536u;
static_assert(kResetRowWords == 41, "the lane map below");

// the lane map: lanes first(kind) .. first(kind + 1) - 1 own the words of `kind`; the prefix table {0, 4, 24, 25, 33, 37, 41}
NM_HDFN int reset_rows_first(int kind) { return kind <= 0 ? 0 : kind == 1 ? 4 : kind == 2 ? 24 : kind == 3 ? 25 : kind == 4 ? 33 : kind == 5 ? 37 : 41; }
NM_HDFN int reset_rows_kind(int lane) { return lane < 4 ? 0 : lane < 24 ? 1 : lane < 25 ? 2 : lane < 33 ? 3 : lane < 37 ? 4 : 5; }
NM_HDFN int reset_rows_width(int kind) { return reset_rows_first(kind + 1) - reset_rows_first(kind); }

// the pool row of `kind` that reset k of the env with global id genv takes, out of P rows (P >= 1)
NM_HDFN uint32_t reset_rows_index(uint64_t seed, uint64_t genv, uint32_t k, int kind, uint32_t P) {
  const uint64_t bits = rand_u24_bits(seed + kResetRowsKey, genv, 8u * k + (uint32_t)kind);
  return (uint32_t)((bits * (uint64_t)P) >> 24);
}
// all six kinds at once; a size of 0 (no pool) gives 0. What nm_reset_rows_pick exports: the host evaluates the function the kernels call
NM_HDFN void nm_reset_rows_pick(uint64_t seed, uint64_t genv, uint32_t k, const uint32_t sizes[kResetRowKinds], uint32_t out[kResetRowKinds]) {
  for (int kind = 0; kind < kResetRowKinds; kind++) out[kind] = sizes[kind] ? reset_rows_index(seed, genv, k, kind, sizes[kind]) : 0u;
}

// The pools of one env object, in DEVICE memory of that object: the kernels read it there (the K-step launches have no LDS left for six
// pointers per argument struct). pool[kind]: P rows of the kind's width in the env's dtype (kLat: P ints); size[kind]: P, 0 = no pool.
struct ResetRowsDesc {
  uint64_t pool[kResetRowKinds];
  uint32_t size[kResetRowKinds];
};

#ifndef NM_EMUL
// word `lane` (0..40) of reset k of env `env` (local index; genv = its global id): pool[i][word] into the env's row, at the addresses
// nm_env_rows.h / nm_core.h define. A lane whose kind has no pool does nothing; the lanes of one kind compute the same i. A needs envp and
// N only. Vector loads and stores throughout.
template <class real>
NM_FN void reset_rows_apply(const Args<real>& A, const ResetRowsDesc* desc, uint64_t seed, uint64_t genv, size_t env, uint32_t k, int lane) {
  const int kind = reset_rows_kind(lane), w = lane - reset_rows_first(kind), W = reset_rows_width(kind);
  const uint32_t P = simt::gld1((const uint32_t*)desc->size, (size_t)kind);
  if (P == 0u) return;
  const uint64_t pool = simt::gld1((const uint64_t*)desc->pool, (size_t)kind);
  const size_t i = (size_t)reset_rows_index(seed, genv, k, kind, P);
  if (kind == 2) {       // the delay: a 4-byte word in either dtype
    simt::gst1(lat_delay(A), env, simt::gld1(reinterpret_cast<const int*>(pool), i));
    return;
  }
  const size_t N = (size_t)A.N;
  real* rows = kind == 0 ? const_cast<real*>(A.envp)
             : kind == 1 ? const_cast<real*>(A.envp) + N * kEnvP
             : kind == 3 ? const_cast<real*>(grav_rows_of(A))
             : kind == 4 ? const_cast<real*>(servo_rows_of(A))
                         : const_cast<real*>(torque_rows_of(A));
  simt::gst1(rows, env * (size_t)W + (size_t)w, simt::gld1(reinterpret_cast<const real*>(pool), i * (size_t)W + (size_t)w));
}

// One wave per env to look at: lanes 0..40 own the words, lane 0 the count (its store needs the value every lane of the wave has loaded
// by then: nobody reads the count after it is written). ids: the envs to look at, or null = envs 0..n-1; done: [N] reset flags of the
// step that just ran, or null = every listed env (nm_reset). The shape and launch geometry of k_reset_noise.
template <class real>
__global__ void __launch_bounds__(256) k_reset_rows(Args<real> A, const ResetRowsDesc* __restrict__ desc, uint32_t* __restrict__ count,
                                                   const int64_t* __restrict__ done, const int32_t* __restrict__ ids, int n) {
  const int j = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), c = (int)(threadIdx.x & 63);
  if (j >= n) return;
  const int env = ids ? ids[j] : j;
  if (done && done[env] <= 0) return;
  const uint32_t k = count[env];
  if (c < kResetRowWords) reset_rows_apply<real>(A, desc, A.seed, (uint64_t)(A.env_offset + env), (size_t)env, k, c);
  if (c == 0) count[env] = k + 1u;
}
#endif

}  // namespace nm
