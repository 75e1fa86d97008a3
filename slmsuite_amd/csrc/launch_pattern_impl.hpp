// Launcher of pattern_kernel for one grid type (launch_pattern_f32.hip / launch_pattern_f64.hip).
#pragma once
#include "pattern_kernels.hpp"
#include "dispatch.hpp"

namespace hgs {

template <typename O, bool PROD, int MODE> static int launch_pattern_one(hipStream_t s, const PatArgs<PATTERN_REAL, void>& v) {
    PatArgs<PATTERN_REAL, O> a;
    a.out = static_cast<O*>(v.out);
    a.x = v.x; a.y = v.y; a.S = v.S; a.W = v.W; a.H = v.H;
    a.quad = v.quad; a.round_g = v.round_g; a.dec_double = v.dec_double; a.pixel_mask = v.pixel_mask;
    a.l = v.l; a.p = v.p; a.n = v.n; a.m = v.m;
    a.shift = v.shift; a.off = v.off; a.half = v.half; a.base = v.base; a.kx = v.kx; a.ky = v.ky; a.s = v.s;
    for (int i = 0; i < 4; ++i) a.set[i] = v.set[i];
    // one lane per four values, plus the lane that takes the values outside the aligned quads
    const dim3 grid((unsigned)((poly_lanes(a.S) + POLY_WG - 1) / POLY_WG));
    dispatch_note(dispatch_site<KPattern, PATTERN_REAL, (int)sizeof(O), PROD, MODE>(), a.quad ? DF_QUAD : 0u);
    hipLaunchKernelGGL((pattern_kernel<PATTERN_REAL, O, PROD, MODE>), grid, dim3(POLY_WG), 0, s, a);
    return (int)hipGetLastError();
}

template <typename O, bool PROD> static int launch_pattern_as(int mode, hipStream_t s, const PatArgs<PATTERN_REAL, void>& a) {
    switch (mode) {
        case PAT_BLAZE: return launch_pattern_one<O, PROD, PAT_BLAZE>(s, a);
        case PAT_SINUSOID: return launch_pattern_one<O, PROD, PAT_SINUSOID>(s, a);
        case PAT_BINARY: return launch_pattern_one<O, PROD, PAT_BINARY>(s, a);
        case PAT_AXICON: return launch_pattern_one<O, PROD, PAT_AXICON>(s, a);
        case PAT_LG: return launch_pattern_one<O, PROD, PAT_LG>(s, a);
        default: return launch_pattern_one<O, PROD, PAT_HG>(s, a);
    }
}

template <> int launch_pattern<PATTERN_REAL>(int mode, bool product, int out_bytes, hipStream_t s, const PatArgs<PATTERN_REAL, void>& a) {
    if (out_bytes == 4)
        return product ? launch_pattern_as<float, true>(mode, s, a) : launch_pattern_as<float, false>(mode, s, a);
    return product ? launch_pattern_as<double, true>(mode, s, a) : launch_pattern_as<double, false>(mode, s, a);
}

}  // namespace hgs
