// nm_play_elu.hip - the play kernel (k_env_play) for hidden activation NM_ACT_ELU, a translation unit of its own (why:
// nm_play_kernels.h).
#define NM_PLAY_ACT NM_ACT_ELU
#include "nm_play_kernels.h"
