// nm_rollout_priv_selu.hip - the rollout kernels of the asymmetric actor-critic (k_env_rollout, k_roll_act over PrivShape: the critic reads
// the privileged row) for hidden activation NM_ACT_SELU, a translation unit of their own (why: nm_rollout_kernels.h).
#define NM_ROLLOUT_ACT NM_ACT_SELU
#define NM_ROLLOUT_PRIV
#include "nm_rollout_kernels.h"
