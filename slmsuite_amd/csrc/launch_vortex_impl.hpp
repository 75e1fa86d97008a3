// Launchers of the hgs_remove_vortices kernels for one element type (launch_vortex_f32.hip / launch_vortex_f64.hip).
#pragma once
#include "vortex_kernels.hpp"
#include "dispatch.hpp"

namespace hgs {

template <> int launch_vortex_find<VX_REAL>(hipStream_t s, const VortexFindArgs<VX_REAL>& a) {
    if (a.pass == 0) dispatch_note(dispatch_site<KVortexFind, VX_REAL>());      // (one record per search, not per pass)
    hipLaunchKernelGGL(vortex_find_kernel<VX_REAL>, dim3(vortex_find_blocks(a.P)), dim3(VX_WG), 0, s, a);
    return (int)hipGetLastError();
}

template <> int launch_vortex_remove<VX_REAL>(hipStream_t s, const VortexRemoveArgs<VX_REAL>& a) {
    const size_t lanes = (a.P + VX_PIX - 1) / VX_PIX;
    dispatch_note(dispatch_site<KVortexRemove, VX_REAL>());
    hipLaunchKernelGGL(vortex_remove_kernel<VX_REAL>, dim3((unsigned)((lanes + VX_WG - 1) / VX_WG)), dim3(VX_WG), 0, s, a);
    return (int)hipGetLastError();
}

#ifdef VX_WITH_SCAN
int launch_vortex_scan(hipStream_t s, unsigned* counts, unsigned n, int32_t* count) {
    hipLaunchKernelGGL(vortex_scan_kernel<VX_SCAN_WG>, dim3(1), dim3(VX_SCAN_WG), 0, s, counts, n, count);
    return (int)hipGetLastError();
}
#endif

}  // namespace hgs
