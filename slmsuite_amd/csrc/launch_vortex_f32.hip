#define VX_REAL float
#define VX_WITH_SCAN 1
#include "launch_vortex_impl.hpp"
