// nm_priv_obs.hip - k_priv_obs (nm_priv_obs.h) for both env dtypes, behind nm_launch_priv_obs(): the gather of the privileged critic row.
#include "nm_priv_obs.h"

template <class real> static hipError_t launch(const nm::PrivObsArgs<real>& a, hipStream_t s) {
  hipLaunchKernelGGL(nm::k_priv_obs<real>, dim3((unsigned)((a.N + nm::kPrivEnvs - 1) / nm::kPrivEnvs)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t nm_launch_priv_obs(const nm::PrivObsArgs<float>& a, hipStream_t s) { return launch(a, s); }
hipError_t nm_launch_priv_obs(const nm::PrivObsArgs<double>& a, hipStream_t s) { return launch(a, s); }
