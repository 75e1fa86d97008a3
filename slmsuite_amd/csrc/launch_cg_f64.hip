#define CG_REAL double
#include "launch_cg_impl.hpp"
