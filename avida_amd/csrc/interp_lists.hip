// interp_lists.hip -- the list classes' k_interpret kernels for counter streams
// (interp_launch.h lists every unit's share).
#include "interp_launch.h"

INTERP_LISTS(INTERP_DEFINE, false)
