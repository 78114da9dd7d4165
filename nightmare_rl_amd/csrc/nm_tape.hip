// nm_tape.hip - the tape kernel (k_env_tape: K env steps per launch from a [K,N,18] action tape; C ABI nm_step_tape in nm_hip.hip), a
// translation unit of its own (why: nm_tape_kernels.h).
#include "nm_tape_kernels.h"
