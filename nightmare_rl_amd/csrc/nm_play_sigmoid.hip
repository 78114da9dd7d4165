// nm_play_sigmoid.hip - the play kernel (k_env_play) for hidden activation NM_ACT_SIGMOID, a translation unit of its own (why:
// nm_play_kernels.h).
#define NM_PLAY_ACT NM_ACT_SIGMOID
#include "nm_play_kernels.h"
