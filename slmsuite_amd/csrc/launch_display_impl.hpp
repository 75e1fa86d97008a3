// Launchers of the hgs_get_display kernels for one element type (launch_display_f32.hip / launch_display_f64.hip).
#pragma once
#include "display_kernels.hpp"
#include "dispatch.hpp"

namespace hgs {

template <> int launch_display_range<DISP_REAL>(int batch, hipStream_t s, const DisplayArgs<DISP_REAL>& a) {
    hipLaunchKernelGGL(phase_range_kernel<DISP_REAL>, dim3(a.range_blocks, batch), dim3(DISP_WG), 0, s, a);
    return (int)hipGetLastError();
}

template <> int launch_display<DISP_REAL>(int batch, bool bits16, hipStream_t s, const DisplayArgs<DISP_REAL>& a) {
    // one lane per four pixels of a hologram, plus the lane that takes the pixels outside its aligned quads
    const dim3 grid((unsigned)((disp_lanes(a.S) + DISP_WG - 1) / DISP_WG), batch);
    const unsigned flags = batch > 1 ? DF_BATCH : 0u;
    if (bits16) {
        dispatch_note(dispatch_site<KDisplay, DISP_REAL, 16>(), flags);
        hipLaunchKernelGGL((phase_display_kernel<DISP_REAL, 16>), grid, dim3(DISP_WG), 0, s, a);
    } else {
        dispatch_note(dispatch_site<KDisplay, DISP_REAL, 8>(), flags);
        hipLaunchKernelGGL((phase_display_kernel<DISP_REAL, 8>), grid, dim3(DISP_WG), 0, s, a);
    }
    return (int)hipGetLastError();
}

}  // namespace hgs
