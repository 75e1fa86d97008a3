// Launchers of the optimize(method="CG") kernels for one element type (launch_cg_f32.hip / launch_cg_f64.hip).
#pragma once
#include "cg_kernels.hpp"
#include "dispatch.hpp"

namespace hgs {

template <> int launch_cg_seed<CG_REAL>(int blocks, hipStream_t s, const CgSeedArgs<CG_REAL>& a) {
    dispatch_note(dispatch_site<KCgSeed, CG_REAL>());
    hipLaunchKernelGGL(cg_seed_kernel<CG_REAL>, dim3(blocks), dim3(CG_WG), 0, s, a);
    return (int)hipGetLastError();
}

template <> int launch_cg_adam<CG_REAL>(hipStream_t s, const CgAdamArgs<CG_REAL>& a) {
    // one lane per four SLM pixels, plus the lane that takes what a count that is no multiple of four leaves over
    const size_t lanes = a.S / 4 + ((a.S & 3) ? 1 : 0);
    dispatch_note(dispatch_site<KCgAdam, CG_REAL>());
    hipLaunchKernelGGL(cg_adam_kernel<CG_REAL>, dim3((unsigned)((lanes + CG_WG - 1) / CG_WG)), dim3(CG_WG), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace hgs
