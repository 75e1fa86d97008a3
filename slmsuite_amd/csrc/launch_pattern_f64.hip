#define PATTERN_REAL double
#include "launch_pattern_impl.hpp"
