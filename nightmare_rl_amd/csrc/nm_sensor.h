// nm_sensor.h - the per-env sensor model: observation latency and bias (no upstream line: the reference's policy reads the exact state
// of the current step, envs/nightmare_v3_env.py:274-305; a real Nightmare's IMU / state estimator and servo feedback arrive one to three
// control periods late and carry offsets that stay constant over an episode). The model is a pure function of the observation rows the
// step already files, so it sits BETWEEN the step and whoever reads the observation; the step kernels do not know it exists.
//     columns    group     treatment
//     0..8       imu       base lin vel, base ang vel, projected gravity: delayed by d_imu env steps and biased
//     9..11      -         commands: passed through bit for bit
//     12..47     joint     dof_pos, dof_vel: delayed by d_joint env steps and biased
//     48..65     -         previous actions: passed through bit for bit
// Per env e: two delays d_imu[e], d_joint[e] in 0..kSensorMaxDelay whole env steps, a float32 bias row b[e][66] in observation units (zero
// in the pass-through columns), a ring of the last kSensorSlots true observations and a count n[e] of the observations pushed since the
// ring was last cleared. With y_s the observation the step kernel produced at step s (after its own noise and clip - the "true" row):
//     1. push y_s (slot n mod 4), n <- n + 1
//     2. column c of group g:   sensed[c] = clamp(y_{s - min(d_g, n - 1)}[c] + b[c], -clip_obs, +clip_obs)     one fp32 add; the step's clip_obs
//        pass-through column:   sensed[c] = y_s[c]
//     3. if the step's done flag is set, n <- 0 - AFTER the read: the done step's own reading is delayed like any other, and the next
//        step sees only itself
// nm_reset clears n for the ids it resets; construction, nm_set_sensor and nm_draw_sensor clear it for every env: a reading never reaches
// behind a clear. The model is float32 whatever the env's dtype (observations are float in both builds).
// Who runs it, always the env's one owner:
//   * per-step path: k_sensor (nm_sensor.hip), launched by nm_step behind k_env_step and the reset launches while the model is on; the step
//     then files its observation in the env's true-obs buffer and k_sensor writes the caller's. Physics-only steps do not touch the model
//   * K-step launches: nmr::step_sensor (nm_env_loop.h) inside the wave that owns the env, between two steps
// Delays 0 and bias 0 give the step's own row under == (y + 0 and a clamp the step has already applied; a -0 reads +0 in a delayed column).
#pragma once
#include <math.h>
#include <stdint.h>

#include "nm_core.h"

namespace nm {

constexpr uint64_t kSensorKey = 0x53454E534Full;      // nm_draw_sensor: rand_u24_bits(seed + kSensorKey, global env id, column) ("SENSO")
constexpr int kSensorMaxDelay = 3, kSensorSlots = 4;  // the ring holds y_s and the kSensorMaxDelay rows before it
constexpr int kSensorGroups = 2, kSensorImu = 0, kSensorJoint = 1;
constexpr int kSensorKinds = 5;                       // bias maxima in the order lin_vel, ang_vel, gravity, dof_pos, dof_vel
constexpr int kSensorDrawWords = kNOBS + kSensorGroups;      // what one env's draw holds: 66 bias words, then the two delays
static_assert(kSensorSlots == kSensorMaxDelay + 1 && (kSensorSlots & (kSensorSlots - 1)) == 0, "slot = count mod kSensorSlots, by a mask");

// the column tables: group (-1 = pass-through) and bias kind (-1 = none) of observation column c
NM_HDFN int sensor_col_group(int c) { return c < 9 ? kSensorImu : c < 12 ? -1 : c < 48 ? kSensorJoint : -1; }
NM_HDFN int sensor_col_kind(int c) { return c < 3 ? 0 : c < 6 ? 1 : c < 9 ? 2 : c < 12 ? -1 : c < 30 ? 3 : c < 48 ? 4 : -1; }

// The model's memory, all device memory of the env object. The K-step kernels read the struct itself from device memory (their argument
// structs sit in LDS, which has no room for it - as nm::ResetRowsDesc); k_sensor takes it by value.
struct SensorDesc {
  const int32_t* delay;     // [N,2]: d_imu, d_joint
  const float* bias;        // [N,66]
  float* ring;              // [N,4,66]: slot (n mod 4) takes the push of an env whose count is n
  uint32_t* count;          // [N]
  float* true_obs;          // [N,66]: where the step files its observation while the model is on
  float* out;               // [N,66]: where a K-step launch without a row of its own (nm_step_tape without an observation record) files the sensed row
  float clip_obs;           // the step kernel's float32 clip
  int pad;
};
static_assert(sizeof(SensorDesc) == 56, "six pointers and two words");

// Steps 1-3 for column c of env `env` (local index), whose count was n before this step (read by the caller BEFORE any lane calls this:
// column 0 stores the new count). y comes from D.true_obs, the sensed value goes to out [N,66]. The one definition of the model: k_sensor,
// nmr::step_sensor and the host emulation (tests/sensor_emul.cpp) call it.
NM_FN void sensor_apply(const SensorDesc& D, size_t env, int c, uint32_t n, bool done, float* out) {
  const size_t row = env * kNOBS + (size_t)c;
  const float y = simt::gld1((const float*)D.true_obs, row);
  simt::gst1(D.ring, (env * kSensorSlots + (size_t)(n & (kSensorSlots - 1))) * kNOBS + (size_t)c, y);
  float v = y;
  const int g = sensor_col_group(c);
  if (g >= 0) {
    const uint32_t d = (uint32_t)simt::gld1(D.delay, env * kSensorGroups + (size_t)g), k = d < n ? d : n;      // min(d_g, n' - 1), n' = n + 1
    float x = y;
    if (k) x = simt::gld1((const float*)D.ring, (env * kSensorSlots + (size_t)((n - k) & (kSensorSlots - 1))) * kNOBS + (size_t)c);   // another slot than the push's
    x = x + simt::gld1(D.bias, row);
    v = fminf(fmaxf(x, -D.clip_obs), D.clip_obs);
  }
  simt::gst1(out, row, v);
  if (c == 0) simt::gst1(D.count, env, done ? 0u : n + 1u);
}

// Word w of the draw of the env with global id genv: w < 66 the bias of column w -> *bias_out, (2 u - 1) * bmax[kind] with
// u = rand_u24_bits(seed + kSensorKey, genv, w) * 2^-24 (2 u - 1 is exact in float32, the product rounds once; +0 in a pass-through
// column); w = 66 + g the delay of group g -> *delay_out, lo[g] + ((bits * (hi[g] - lo[g] + 1)) >> 24) in 64-bit integers
// (nm_draw_action_latency's rule). The host calls the same function (nm_sensor_draw_values).
NM_HDFN void sensor_draw(uint64_t seed, uint64_t genv, const int32_t* lo, const int32_t* hi, const float* bmax, int w, int32_t* delay_out, float* bias_out) {
  const uint64_t bits = rand_u24_bits(seed + kSensorKey, genv, (uint32_t)w);
  if (w < kNOBS) {
    const int kind = sensor_col_kind(w);
    const float u = (float)bits * (1.0f / 16777216.0f), s = 2.0f * u - 1.0f;
    *bias_out = kind < 0 ? 0.0f : s * (kind == 0 ? bmax[0] : kind == 1 ? bmax[1] : kind == 2 ? bmax[2] : kind == 3 ? bmax[3] : bmax[4]);
  } else {
    const int g = w - kNOBS;
    *delay_out = lo[g] + (int32_t)((bits * (uint64_t)(hi[g] - lo[g] + 1)) >> 24);
  }
}

}  // namespace nm

#ifndef NM_EMUL
#include <hip/hip_runtime.h>
// the launches of nm_sensor.hip (the kernels have a unit of their own, as k_priv_obs has), all on `s`:
// k_sensor - the model for every env behind a step: done [N] = the step's reset flags, out [N,66] = the caller's observation buffer
hipError_t nm_launch_sensor(const nm::SensorDesc& d, const int64_t* done, float* out, int N, hipStream_t s);
// n <- 0 for the n listed envs (ids null: envs 0..n-1)
hipError_t nm_launch_sensor_clear(uint32_t* count, const int32_t* ids, int n, hipStream_t s);
// the draw of every env's delays [N,2] and bias [N,66]
struct nm_sensor_draw_args { int32_t lo[2], hi[2]; float bmax[nm::kSensorKinds]; };
hipError_t nm_launch_sensor_draw(int32_t* delay, float* bias, int N, uint64_t seed, int64_t env_offset, const nm_sensor_draw_args& a, hipStream_t s);
// *dst = d (the descriptor the K-step kernels read), behind what `s` carries
hipError_t nm_launch_sensor_desc(nm::SensorDesc* dst, const nm::SensorDesc& d, hipStream_t s);
#endif
