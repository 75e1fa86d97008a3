#define POLY_REAL double
#include "launch_poly_impl.hpp"
