// interp_c0.hip -- class 0's k_interpret kernels for counter streams
// (interp_launch.h lists every unit's share).
#include "interp_launch.h"

INTERP_CLASS0(INTERP_DEFINE, false)
