// interp_c0_rec.hip -- class 0's k_interpret kernels for recorded streams (DevWorld::rec)
// (interp_launch.h lists every unit's share).
#include "interp_launch.h"

INTERP_CLASS0(INTERP_DEFINE, true)
