// interp_lists_rec.hip -- the list classes' k_interpret kernels for recorded streams (DevWorld::rec)
// (interp_launch.h lists every unit's share).
#include "interp_launch.h"

INTERP_LISTS(INTERP_DEFINE, true)
