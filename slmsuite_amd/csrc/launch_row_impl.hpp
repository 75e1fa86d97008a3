// Included by launch_row_f32.hip / launch_row_f64.hip with HGS_REAL defined.
#include "launch.hpp"
#include <cstdlib>

namespace hgs {

// prefetching form (row_kernel PREF): transform image + the 32 KB image of the next row
template <typename R, int N, int NS>
static int launch_row_pref(dim3 grid, hipStream_t s, const RowArgs<R>& a) {
    constexpr size_t lds = (lds_elems<N>() + N) * sizeof(Cx<R>);
    static_assert(lds > 48 * 1024, "launch_row_pref: the two images need the raised LDS limit");
#ifdef HGS_REAL_IS_FLOAT
    if (a.zero_mask != nullptr) return launch_instance<KRowZ, R, N, 2, NS, true, false>(grid, dim3(RowCfg<N>::WG), lds, s, row_flags(grid, a), a);
#endif
    return launch_instance<KRow, R, N, 2, NS, true, false>(grid, dim3(RowCfg<N>::WG), lds, s, row_flags(grid, a), a);
}

template <typename R, int N, int MODE, int NS = 16>
static int launch_row_one(dim3 grid, hipStream_t s, const RowArgs<R>& a) {
    // The shifted 4096-point kernel needs 117 VGPRs, so four workgroups fit a CU.  Measured (cfg 2 / a batch of eight):
    // a masked launch (active columns only) gains from the fourth -- 20.5 -> 19.0 us, 103 -> 88 us -- a dense one does
    // not (28.2 us either way; batch 174 -> 195 us: the load bursts of 1,024 rows at once).  Asking for 48 KB of LDS
    // keeps a dense launch at three.
    constexpr size_t lds_need = (size_t)RowCfg<N>::FPW * lds_elems<N>() * sizeof(Cx<R>);
    const bool masked = a.load_mask != nullptr || a.store_mask != nullptr;
    const size_t lds = (NS < 16 && N == 4096 && !masked && lds_need < 48 * 1024) ? (size_t)48 * 1024 : lds_need;
#ifdef HGS_REAL_IS_FLOAT
    // (RowArgs::zero_mask: the instances that honour it, MODE 2 only; anywhere else the mask is an error, not ignored)
    if (a.zero_mask != nullptr) {
        if constexpr (MODE == 2) return launch_instance<KRowZ, R, N, MODE, NS, false, false>(grid, dim3(RowCfg<N>::WG), lds, s, row_flags(grid, a), a);
        else return (int)hipErrorInvalidValue;
    }
#else
    if (a.zero_mask != nullptr) return (int)hipErrorInvalidValue;
#endif
    return launch_instance<KRow, R, N, MODE, NS, false, false>(grid, dim3(RowCfg<N>::WG), lds, s, row_flags(grid, a), a);
}

// shifted form (row_kernel NS = 8): fp32, one-row workgroups, SLM within eight of the sixteen register slots (RowArgs::shifted, m0)
template <typename R, int N>
static int launch_row_n(int mode, dim3 grid, hipStream_t s, const RowArgs<R>& a) {
#ifdef HGS_REAL_IS_FLOAT
    if constexpr (N == 4096) {
        // (RowArgs::zero_mask is no load / store mask: every column is read and written, the prefetching form stays)
        if (a.prefetch && mode == 2 && a.load_mask == nullptr && a.store_mask == nullptr)
            return a.shifted ? launch_row_pref<R, N, 8>(grid, s, a) : launch_row_pref<R, N, 16>(grid, s, a);
    }
    if constexpr (N >= 4096) {
        if (a.shifted) {
            switch (mode) {
                case 0: return launch_row_one<R, N, 0, 8>(grid, s, a);
                case 1: return launch_row_one<R, N, 1, 8>(grid, s, a);
                case 2: return launch_row_one<R, N, 2, 8>(grid, s, a);
                case 3: return launch_row_one<R, N, 3, 8>(grid, s, a);      // (fp32 only: the engine keeps MODE 1 in float64)
            }
        }
    }
#else
    // float64 (round 5): the same shifted form at 4096 / 8192 columns (no MODE 3: the engine keeps MODE 1 in float64)
    if constexpr (N >= 4096) {
        if (a.shifted) {
            switch (mode) {
                case 0: return launch_row_one<R, N, 0, 8>(grid, s, a);
                case 1: return launch_row_one<R, N, 1, 8>(grid, s, a);
                case 2: return launch_row_one<R, N, 2, 8>(grid, s, a);
            }
        }
    }
#endif
    switch (mode) {
        case 0: return launch_row_one<R, N, 0>(grid, s, a);
        case 1: return launch_row_one<R, N, 1>(grid, s, a);
        case 2: return launch_row_one<R, N, 2>(grid, s, a);
#ifdef HGS_REAL_IS_FLOAT
        case 3: return launch_row_one<R, N, 3>(grid, s, a);      // MODE 2 that also writes the phase (last launch of a call)
#endif
    }
    return (int)hipErrorInvalidValue;
}

template <> int launch_row<HGS_REAL>(int N, int mode, dim3 grid, hipStream_t s, const RowArgs<HGS_REAL>& a) {
    switch (N) {
        case 64: return launch_row_n<HGS_REAL, 64>(mode, grid, s, a);
        case 128: return launch_row_n<HGS_REAL, 128>(mode, grid, s, a);
        case 256: return launch_row_n<HGS_REAL, 256>(mode, grid, s, a);
        case 512: return launch_row_n<HGS_REAL, 512>(mode, grid, s, a);
        case 1024: return launch_row_n<HGS_REAL, 1024>(mode, grid, s, a);
        case 2048: return launch_row_n<HGS_REAL, 2048>(mode, grid, s, a);
        case 4096: return launch_row_n<HGS_REAL, 4096>(mode, grid, s, a);
        case 8192: return launch_row_n<HGS_REAL, 8192>(mode, grid, s, a);
    }
    return (int)hipErrorInvalidValue;
}

#ifndef HGS_REAL_IS_FLOAT
// float64 single-pass MRAF (col_fused_kernel with CParams::split + col_kernel<LOAD | INV> into gh2): the row kernel that joins
// the two parts, H = gh * wscale + gh2 (a.gh2 and a.gh2_mask set); rows of 4096 / 8192 (the split form has one-row workgroups)
template <int N, int MODE, int NS = 16>
static int launch_row_split64_one(dim3 grid, hipStream_t s, const RowArgs<double>& a) {
    constexpr size_t lds = (size_t)RowCfg<N>::FPW * lds_elems<N>() * sizeof(Cx<double>);
    static_assert(lds > 48 * 1024, "launch_row_split64_one: a float64 image of 4096 points needs the raised LDS limit");
    return launch_instance<KRow, double, N, MODE, NS, false, true>(grid, dim3(RowCfg<N>::WG), lds, s, row_flags(grid, a), a);
}
template <int N>
static int launch_row_split64_n(int mode, dim3 grid, hipStream_t s, const RowArgs<double>& a) {
    if (a.shifted) return mode == 1 ? launch_row_split64_one<N, 1, 8>(grid, s, a) : launch_row_split64_one<N, 2, 8>(grid, s, a);
    return mode == 1 ? launch_row_split64_one<N, 1>(grid, s, a) : launch_row_split64_one<N, 2>(grid, s, a);
}
int launch_row_split(int N, int mode, dim3 grid, hipStream_t s, const RowArgs<double>& a) {
    if (mode != 1 && mode != 2) return (int)hipErrorInvalidValue;
    if (N == 4096) return launch_row_split64_n<4096>(mode, grid, s, a);
    if (N == 8192) return launch_row_split64_n<8192>(mode, grid, s, a);
    return (int)hipErrorInvalidValue;
}
#endif

template <> size_t row_lds_bytes<HGS_REAL>(int N) {
    const int T = N / 16, WG = T >= 256 ? T : 256;
    return (size_t)(WG / T) * (N + N / 16) * sizeof(Cx<HGS_REAL>);
}

}  // namespace hgs
