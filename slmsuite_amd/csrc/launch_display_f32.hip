#define DISP_REAL float
#include "launch_display_impl.hpp"
