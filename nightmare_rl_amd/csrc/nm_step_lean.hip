// nm_step_lean.hip - k_env_step for the shipped default configuration: every question the stages put to the configuration is answered at
// compile time (nm::CfgLean, nm_core.h), so the wave carries no test of a model flag or of an optional launch argument and none of the
// code behind them. A translation unit of its own (nm_step_kernel.h says why). nm_hip.hip decides per launch whether this kernel or
// the generic one runs.
#include "nm_step_kernel.h"

hipError_t nm_launch_step_lean(int N, hipStream_t s, const nm::Model<float>* M_dev, const nm::Args<float>& a) {
  constexpr int G = NM_ENVS_PER_WAVE, W = kWG;
  hipLaunchKernelGGL((k_env_step<float, G, 0, nm::CfgLean>), dim3((N + G * W - 1) / (G * W)), dim3(64 * W), 0, s, M_dev, a);
  return hipGetLastError();
}
