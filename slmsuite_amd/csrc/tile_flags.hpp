// The flag word of a four-column tile (col_tile2_kernel): the column scan writes one byte per column, bit 0 of which says that
// the column holds a non-zero (or NaN) weight or target; the kernel reads the four bytes of a tile as ONE aligned little-endian
// word -- byte k is column k of the tile, half tile h owns bytes 2 h and 2 h + 1.  A word of -1 stands for "no flags: every
// column counts as active".  Host code includes this header too (tests/tile_flags_host.cpp checks it exhaustively).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HGS_FLAGS_HD __host__ __device__
#else
#define HGS_FLAGS_HD
#endif

namespace hgs {

// column c (0 / 1) of half tile `half` (0 / 1) holds a weight or a target
HGS_FLAGS_HD constexpr bool tile2_col_active(int fw, int half, int c) {
    return (((unsigned)fw >> (16 * half + 8 * c)) & 1u) != 0u;
}
// neither column of the half tile does
HGS_FLAGS_HD constexpr bool tile2_half_empty(int fw, int half) {
    return (((unsigned)fw >> (16 * half)) & 0x0101u) == 0u;
}

// The walk of a workgroup over ITS half tiles (tiles ct, ct + ct_step, ... below ntiles, half `half` of each) that stops at the
// first one which is not empty: returns that tile's index and leaves its flag word in *fw, or returns a value >= ntiles (and
// *fw untouched) when none is left.  `load(i)` gives the flag word of tile i and is called for tiles below ntiles only, once per
// tile looked at.  The kernel passes uniform_load_i32 of the scan's bytes: tile index, word and loop are scalars, no vector
// register is touched (col_tile2_kernel with ColArgs::h_prezeroed; tests/tile_flags_next_host.cpp walks it on the host).
// (ct_step >= 1)
template <typename Load>
HGS_FLAGS_HD inline int tile2_next_nonempty(Load&& load, int ct, int ct_step, int ntiles, int half, int* fw) {
    while (ct < ntiles) {
        const int w = load(ct);
        if (!tile2_half_empty(w, half)) { *fw = w; return ct; }
        ct += ct_step;
    }
    return ct;
}

}  // namespace hgs
