// nm_play_selu.hip - the play kernel (k_env_play) for hidden activation NM_ACT_SELU, a translation unit of its own (why:
// nm_play_kernels.h).
#define NM_PLAY_ACT NM_ACT_SELU
#include "nm_play_kernels.h"
