// nm_sensor.hip - the kernels of the per-env sensor model (nm_sensor.h) outside the K-step launches: k_sensor, the model behind one
// nm_step; k_sensor_clear, k_sensor_draw and k_sensor_desc, the small launches of nm_reset, nm_draw_sensor and the K-step launchers.
#include "nm_sensor.h"

namespace nm {

// One wave per env: lane l owns column l, lanes 0 / 1 also columns 64 / 65. Every lane loads the env's count before lane 0 stores the
// new one (the store's value depends on the load, and the wave's loads return in order), and no other wave touches the env.
__global__ void __launch_bounds__(256) k_sensor(SensorDesc D, const int64_t* __restrict__ done, float* __restrict__ out, int N) {
  const int env = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = (int)(threadIdx.x & 63);
  if (env >= N) return;
  const uint32_t n = D.count[env];
  const bool dn = done[env] > 0;
  sensor_apply(D, (size_t)env, lane, n, dn, out);
  if (lane < kNOBS - 64) sensor_apply(D, (size_t)env, lane + 64, n, dn, out);
}

__global__ void k_sensor_clear(uint32_t* __restrict__ count, const int32_t* __restrict__ ids, int n) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) count[ids ? ids[j] : j] = 0u;
}

// one thread per (env, word of the env's draw)
__global__ void k_sensor_draw(int32_t* __restrict__ delay, float* __restrict__ bias, int N, uint64_t seed, int64_t env_offset, nm_sensor_draw_args a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kSensorDrawWords * N) return;
  const int env = i / kSensorDrawWords, w = i - env * kSensorDrawWords;
  sensor_draw(seed, (uint64_t)(env_offset + env), a.lo, a.hi, a.bmax, w, delay + (size_t)env * kSensorGroups + (w < kNOBS ? 0 : w - kNOBS),
              bias + (size_t)env * kNOBS + (w < kNOBS ? w : 0));
}

__global__ void k_sensor_desc(SensorDesc* dst, SensorDesc d) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *dst = d;
}

}  // namespace nm

hipError_t nm_launch_sensor(const nm::SensorDesc& d, const int64_t* done, float* out, int N, hipStream_t s) {
  hipLaunchKernelGGL(nm::k_sensor, dim3((unsigned)(((size_t)N * 64 + 255) / 256)), dim3(256), 0, s, d, done, out, N);
  return hipGetLastError();
}
hipError_t nm_launch_sensor_clear(uint32_t* count, const int32_t* ids, int n, hipStream_t s) {
  hipLaunchKernelGGL(nm::k_sensor_clear, dim3((n + 255) / 256), dim3(256), 0, s, count, ids, n);
  return hipGetLastError();
}
hipError_t nm_launch_sensor_draw(int32_t* delay, float* bias, int N, uint64_t seed, int64_t env_offset, const nm_sensor_draw_args& a, hipStream_t s) {
  hipLaunchKernelGGL(nm::k_sensor_draw, dim3((nm::kSensorDrawWords * N + 255) / 256), dim3(256), 0, s, delay, bias, N, seed, env_offset, a);
  return hipGetLastError();
}
hipError_t nm_launch_sensor_desc(nm::SensorDesc* dst, const nm::SensorDesc& d, hipStream_t s) {
  hipLaunchKernelGGL(nm::k_sensor_desc, dim3(1), dim3(64), 0, s, dst, d);
  return hipGetLastError();
}
