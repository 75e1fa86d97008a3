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

// The same walk over the POSITIONS of the ascending list of tiles that hold anything (any byte of the flag word with bit 0 set;
// `nlist` entries, `list(p)` gives entry p): the workgroup owns positions *pos, *pos + step, ... below nlist and half `half` of
// the tile each of them names.  Stops at the first position whose half is not empty: returns that TILE, leaves its flag word in
// *fw and the position in *pos; or returns ntiles (and *fw untouched, *pos >= nlist) when none is left.  A listed tile has at
// least one non-empty half, so of the two workgroups that share a position at least one stops there; with no more listed tiles
// than workgroup pairs nobody owns two.  Scalars throughout, like tile2_next_nonempty (tests/tile_list_host.cpp walks both).
// (step >= 1)
template <typename List, typename Load>
HGS_FLAGS_HD inline int tile2_next_listed(List&& list, Load&& load, int* pos, int step, int nlist, int ntiles, int half, int* fw) {
    int p = *pos;
    while (p < nlist) {
        const int t = list(p);
        const int w = load(t);
        if (!tile2_half_empty(w, half)) { *fw = w; *pos = p; return t; }
        p += step;
    }
    *pos = p;
    return ntiles;
}
// a tile belongs on that list
HGS_FLAGS_HD constexpr bool tile2_listed(int fw) { return ((unsigned)fw & 0x01010101u) != 0u; }

// Weight-norm slots of the half-width kernel's flag-reading instances: one double per hologram, tile, half and wave, indexed by
// WHAT was summed and never by who summed it, so that sum w'^2 does not depend on the schedule.
constexpr int TILE2_WSLOT_WAVES = 4;       // waves of a 4096-row workgroup (256 lanes)
HGS_FLAGS_HD constexpr int tile2_wslots(int Pw) { return Pw / 4 * 2 * TILE2_WSLOT_WAVES; }      // per hologram
HGS_FLAGS_HD constexpr int tile2_wslot(int tile, int half, int wave) { return (tile * 2 + half) * TILE2_WSLOT_WAVES + wave; }

}  // namespace hgs
