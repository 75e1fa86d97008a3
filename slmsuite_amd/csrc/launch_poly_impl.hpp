// Launcher of poly_kernel for one grid type (launch_poly_f32.hip / launch_poly_f64.hip).
#pragma once
#include "poly_kernels.hpp"
#include "dispatch.hpp"

namespace hgs {

template <typename O, bool PROD> static int launch_poly_as(int n_masks, hipStream_t s, const PolyArgs<POLY_REAL, void>& v) {
    PolyArgs<POLY_REAL, O> a;
    a.out = static_cast<O*>(v.out);
    a.x = v.x; a.y = v.y; a.table = v.table; a.vortex = v.vortex;
    a.S = v.S; a.W = v.W; a.deg = v.deg; a.mask_mode = v.mask_mode;
    a.x_scale = v.x_scale; a.y_scale = v.y_scale;
    // one lane per four values of a mask, plus the lane that takes the values outside its aligned quads
    const dim3 grid((unsigned)((poly_lanes(a.S) + POLY_WG - 1) / POLY_WG), n_masks);
    dispatch_note(dispatch_site<KPoly, POLY_REAL, (int)sizeof(O), PROD>(), n_masks > 1 ? DF_BATCH : 0u);
    hipLaunchKernelGGL((poly_kernel<POLY_REAL, O, PROD>), grid, dim3(POLY_WG), 0, s, a);
    return (int)hipGetLastError();
}

template <> int launch_poly<POLY_REAL>(int n_masks, bool product, int out_bytes, hipStream_t s, const PolyArgs<POLY_REAL, void>& a) {
    if (out_bytes == 4)
        return product ? launch_poly_as<float, true>(n_masks, s, a) : launch_poly_as<float, false>(n_masks, s, a);
    return product ? launch_poly_as<double, true>(n_masks, s, a) : launch_poly_as<double, false>(n_masks, s, a);
}

}  // namespace hgs
