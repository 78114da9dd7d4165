// nm_sample.h - the action noise of PPO.act (rsl_rl v1.0.2: Normal(mean, std).sample() and its log_prob), written ONCE for every kernel
// that draws an action: k_ppo_sample (nm_rl.hip), k_ppo_act_fast (nm_ppo.hip) and the wave policy of nm_rollout.h (k_roll_act,
// k_env_rollout, k_env_play). The one-launch rollout, the step-by-step path, nm_ppo_act and nm_play draw the same z for the same
// (seed, iteration, step, env, action pair) because they all feed box_muller the uniforms u24(seed, key, ctr) and u24(seed, key + 1, ctr),
//     key = env * 64 + f0  (f0 = the even action index of the pair),   ctr = iteration * 4096 + step
// - through normal_pair, except k_ppo_sample, which writes those two u24 calls out (nm_rl.hip says why).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nms {

// counter-based uniform in (0,1], 24 bits (the mixer of nm_core.h's rand_u24_bits)
__device__ __forceinline__ float u24(uint64_t seed, uint64_t a, uint64_t b) {
  uint64_t x = seed + 0x9E3779B97F4A7C15ull * (a + 1) + 0xD1B54A32D192ED03ull * b;
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return ((float)(uint32_t)(x >> 40) + 1.0f) * (1.0f / 16777216.0f);
}
// Box-Muller: two standard normals from two uniforms in (0,1]
__device__ __forceinline__ void box_muller(float u1, float u2, float z[2]) {
  const float rad = sqrtf(-2.0f * __logf(u1));
  float sn, cs;
  __sincosf(6.283185307179586f * u2, &sn, &cs);
  z[0] = rad * cs; z[1] = rad * sn;
}
// the two standard normals of the action pair `key`: from the uniforms of key and key + 1
__device__ __forceinline__ void normal_pair(uint64_t seed, uint64_t key, uint64_t ctr, float z[2]) {
  box_muller(u24(seed, key, ctr), u24(seed, key + 1, ctr), z);
}
// Normal.log_prob of the action mean + sd * z: -(a - m)^2 / (2 sd^2) - log sd - log sqrt(2 pi)
__device__ __forceinline__ float logp_term(float z, float sd) { return -0.5f * z * z - __logf(sd) - 0.9189385332046727f; }

}  // namespace nms
