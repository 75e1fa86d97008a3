#define PATTERN_REAL float
#include "launch_pattern_impl.hpp"
