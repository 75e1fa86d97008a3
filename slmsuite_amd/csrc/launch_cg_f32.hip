#define CG_REAL float
#include "launch_cg_impl.hpp"
