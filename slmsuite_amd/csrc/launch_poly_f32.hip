#define POLY_REAL float
#include "launch_poly_impl.hpp"
