// nm_step_lean.hip - k_env_step for the shipped default configuration: every question the stages put to the configuration is answered at
// compile time (nm::CfgLean, nm_core.h), so the wave carries no test of a model flag or of an optional launch argument and none of the
// code behind them. A translation unit of its own (nm_step_kernel.h says why). nm_hip.hip decides per launch whether this kernel or
// the generic one runs.
#include "nm_step_kernel.h"
#include "nm_lane_selftest.h"
#include "../../include/nightmare_hip.h"

hipError_t nm_launch_step_lean(int N, hipStream_t s, const nm::Model<float>* M_dev, const nm::Args<float>& a) {
  constexpr int G = NM_ENVS_PER_WAVE, W = kWG;
  hipLaunchKernelGGL((k_env_step<float, G, 0, nm::CfgLean>), dim3((N + G * W - 1) / (G * W)), dim3(64 * W), 0, s, M_dev, a);
  return hipGetLastError();
}

// The lean kernel's cross-lane helper forms against the forms they replace (nm_lane_selftest.h), one wave per 64 values. Every lane of
// every wave runs (the DPP forms read their neighbours): lanes behind n take zeros and store nothing.
struct LaneMasks { uint64_t m[nm::kLaneMasks]; };
__global__ void __launch_bounds__(64) k_lane_selftest(const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ g, LaneMasks lm, int n,
                                                      float* __restrict__ out) {
  const int i = (int)(blockIdx.x * 64 + threadIdx.x);
  const bool in = i < n;
  const int j = in ? i : 0;
  const float xv = in ? x[j] : 0.f, av = in ? a[j] : 0.f, gv = in ? g[j] : 0.f;
  float o0[nm::kLaneSlots], o1[nm::kLaneSlots];
  nm::lane_selftest_wave<float>(xv, av, gv, lm.m, o0, o1);
  if (in) {
#pragma unroll
    for (int s = 0; s < nm::kLaneSlots; s++) {
      out[(size_t)s * n + i] = o0[s];
      out[(size_t)(nm::kLaneSlots + s) * n + i] = o1[s];
    }
  }
}
extern "C" int nm_lane_selftest(const float* x_dev, const float* a_dev, const float* g_dev, const uint64_t* masks_host, int32_t n, float* out_dev, void* stream) {
  if (!x_dev || !a_dev || !g_dev || !masks_host || !out_dev || n <= 0) return 1;
  LaneMasks lm;
  for (int k = 0; k < nm::kLaneMasks; k++) lm.m[k] = masks_host[k];
  hipLaunchKernelGGL(k_lane_selftest, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, x_dev, a_dev, g_dev, lm, (int)n, out_dev);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
