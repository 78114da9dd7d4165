// nm_rollout_tanh.hip - the rollout kernels (k_env_rollout, k_roll_act) for hidden activation NM_ACT_TANH, a translation unit of
// their own (why: nm_rollout_kernels.h).
#define NM_ROLLOUT_ACT NM_ACT_TANH
#include "nm_rollout_kernels.h"
