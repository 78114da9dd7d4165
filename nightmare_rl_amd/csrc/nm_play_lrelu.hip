// nm_play_lrelu.hip - the play kernel (k_env_play) for hidden activation NM_ACT_LRELU, a translation unit of its own (why:
// nm_play_kernels.h).
#define NM_PLAY_ACT NM_ACT_LRELU
#include "nm_play_kernels.h"
