#define VX_REAL double
#include "launch_vortex_impl.hpp"
