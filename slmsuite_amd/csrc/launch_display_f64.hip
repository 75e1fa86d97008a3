#define DISP_REAL double
#include "launch_display_impl.hpp"
