// nm_priv_obs.h - the privileged critic row (asymmetric actor-critic; no upstream line: the reference has one robot and a critic that sees
// the actor's 66 floats). One float32 row of kNOBS + kPrivN words per env:
//     cols 0..65    the observation the same step returned, bit for bit (noise and clipping included)
//     cols 66..88   what the env's physics was drawn with, read from the per-env block behind nm::Args::envp (layout: nm_env_rows.h) and
//                   from the state, in this order (PC_* below):
//         friction 1        mu
//         gain ratios 2     p_gain / M.p_gain, kv / M.kv
//         payload mass 1    row[BP_MASS] - M.basec mass
//         payload com 3     row[BP_IPOS..+2] - M.basec ipos
//         latency steps 1   delay / nsub
//         gravity 3         row[GP_G..+2] / M.grav
//         servo 2           1 / rate (+inf -> 0), d_gain
//         torque limit 3    1 / fmax[k] (+inf -> 0)
//         wrench 6          F[3] / (M.total_mass M.grav), tau[3] / (M.total_mass M.grav x 1 m)     (the model's total mass, not the env's)
//         base height 1     qpos[2]
// While the block is not allocated every env gets the values the kinds' default rows (nm_env_rows.h) give: M.mu, 1, 1, 0, 0 0 0, 0,
// (0, 0, -1), 0, 0, 0 0 0, 0 x 6. The arithmetic is done in double whatever the env's dtype (a difference of two words of the env's dtype
// is exact there, a quotient rounds once) and the result is rounded to float once.
// k_priv_obs is launched behind the step's own launches (k_env_step, k_reset_noise, k_reset_rows, k_wrench), so the parameter columns
// show the block as those launches LEFT it - the rows the next step runs under - and base height is the state after an in-step reset.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nm_core.h"

namespace nm {

constexpr int kPrivN = 23, kPrivRow = kNOBS + kPrivN;
constexpr int PC_MU = 0, PC_PGAIN = 1, PC_KV = 2, PC_MASS = 3, PC_COM = 4, PC_LAT = 7, PC_GRAV = 8, PC_RATE = 11, PC_DGAIN = 12, PC_TORQUE = 13,
              PC_WRENCH = 16, PC_HEIGHT = 22;
constexpr int kPrivEnvs = 8;       // envs per 256-thread workgroup: 8 x 89 words, one contiguous run of the output

// The regions are the ones nmrows::layout names; the host fills them from the block's base (all null while there is no block).
template <class real> struct PrivObsArgs {
  const real *fric, *body, *grav, *servo, *torque, *wrench;
  const int* delay;
  const real* qpos;        // [N, kNQ]
  const float* obs;        // [N, kNOBS]: the observation the step wrote
  float* out;              // [N, kPrivRow]
  int N, nxcd, nsub;
  double mu, p_gain, kv, base_mass, base_ipos[3], grav0, weight;      // the model's own; weight = total_mass x grav
};

#ifndef NM_EMUL
// column c (0..kPrivN-1) of env e. The chain below only works out WHERE the column's word lies and what is done to it; the word is then
// loaded once, for all columns alike (the delay, a 4-byte int in either dtype, by a second load that does not depend on the first), and
// every column is (x - sub) / den or 1 / x: the lanes of a wave, which hold all 23 columns, wait for memory once and divide once instead
// of once per column kind. A copy is (x - 0) / 1 and a difference (x - sub) / 1: exact.
template <class real> NM_FN float priv_value(const PrivObsArgs<real>& a, size_t e, int c) {
  const real* p = a.qpos;
  size_t idx = e * kNQ + 2;
  double sub = 0.0, den = 1.0;
  bool recip = false;
  if (!a.fric) {
    if (c != PC_HEIGHT) return c == PC_MU ? (float)a.mu : (c == PC_PGAIN || c == PC_KV) ? 1.0f : c == PC_GRAV + 2 ? -1.0f : 0.0f;
  } else if (c < PC_MASS) {
    p = a.fric; idx = e * kEnvP + c; den = c == PC_PGAIN ? a.p_gain : c == PC_KV ? a.kv : 1.0;
  } else if (c < PC_LAT) {
    const int j = c - PC_COM;      // -1: the mass
    p = a.body; idx = e * kBodyP + (j < 0 ? BP_MASS : BP_IPOS + j);
    sub = j < 0 ? a.base_mass : j == 0 ? a.base_ipos[0] : j == 1 ? a.base_ipos[1] : a.base_ipos[2];
  } else if (c == PC_LAT) {
    den = (double)a.nsub;
  } else if (c < PC_RATE) {
    p = a.grav; idx = e * kGravP + GP_G + (c - PC_GRAV); den = a.grav0;
  } else if (c < PC_TORQUE) {
    p = a.servo; idx = e * kServoP + (c == PC_RATE ? SV_RATE : SV_DGAIN); recip = c == PC_RATE;      // 1 / +inf = 0: no limit
  } else if (c < PC_WRENCH) {
    p = a.torque; idx = e * kTorqueP + (c - PC_TORQUE); recip = true;                                // likewise
  } else if (c < PC_HEIGHT) {
    const int j = c - PC_WRENCH;
    p = a.wrench; idx = e * kWrenchP + (j < 3 ? WP_F + j : WP_T + j - 3); den = a.weight;
  }
  const int delay = a.fric ? a.delay[e] : 0;
  double x = (double)p[idx];
  if (c == PC_LAT) x = (double)delay;
  return (float)((recip ? 1.0 : x - sub) / (recip ? x : den));
}

// A workgroup owns kPrivEnvs consecutive envs, i.e. one contiguous run of kPrivEnvs x kPrivRow output words: thread i writes word i, i + 256,
// ... of the run (whole rows, coalesced), a word being a copy of the observation or one gathered value. The block -> env-range map is the
// step kernel's (nm_env_loop.h wave_index): with 8 XCDs, consecutive ranges go to the same XCD, whose L2 then holds the obs rows and the
// block's rows of a contiguous env range.
template <class real>
__global__ void __launch_bounds__(256) k_priv_obs(PrivObsArgs<real> a) {
  int blk = blockIdx.x;
  {
    const int nwx = (int)gridDim.x >> 3;
    if (a.nxcd == 8 && blk < (nwx << 3)) blk = (blk & 7) * nwx + (blk >> 3);
  }
  const int e0 = blk * kPrivEnvs;
  if (e0 >= a.N) return;
  const int cnt = (a.N - e0 < kPrivEnvs ? a.N - e0 : kPrivEnvs) * kPrivRow;
  float* __restrict__ dst = a.out + (size_t)e0 * kPrivRow;
  for (int i = threadIdx.x; i < cnt; i += 256) {
    const int el = i / kPrivRow, c = i - el * kPrivRow;
    const size_t e = (size_t)(e0 + el);
    dst[i] = c < kNOBS ? a.obs[e * kNOBS + c] : priv_value<real>(a, e, c - kNOBS);
  }
}
#endif

}  // namespace nm

// the launch of k_priv_obs<real> on `s` (nm_priv_obs.hip: the kernel has a unit of its own, as the lean step kernel has)
hipError_t nm_launch_priv_obs(const nm::PrivObsArgs<float>& a, hipStream_t s);
hipError_t nm_launch_priv_obs(const nm::PrivObsArgs<double>& a, hipStream_t s);
