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

}  // namespace hgs
