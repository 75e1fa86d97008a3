// Host check of tile2_next_nonempty() of slmsuite_amd/csrc/tile_flags.hpp (tests/test_tile_flags_next.py builds and runs it, with
// -fsanitize=address,undefined): the walk col_tile2_kernel makes over its workgroup's half tiles when H of the empty columns is
// in place already (ColArgs::h_prezeroed), against a brute-force walk over a 64-tile row of flag words.
//   * the row lives in a heap block of exactly 64 words and the loader refuses every other index: a look past the row is a
//     failure here and a report of the sanitizer;
//   * strides 1, 8 and 32, every start the stride allows (and starts at / past the end), both halves;
//   * strides 8 and 32 visit at most eight tiles: EVERY empty / non-empty pattern of the visited tiles, each non-empty one in each
//     of its three fillings (column 0, column 1, both), the other half and the bits above bit 0 filled four ways;
//   * stride 1 visits 64 tiles (2^64 patterns): every one of the 16 bit-0 patterns of a word at every position of an otherwise
//     empty row, every PAIR of non-empty positions, the all-empty and the all-full row, and 4,000 pseudo-random rows of every
//     density from 1/64 to 63/64;
//   * what comes back: the index of the first non-empty half tile at or after the start and ITS word, or an index >= 64 and the
//     word untouched when none is left; one load per tile looked at, none past the tile found.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "tile_flags.hpp"

static constexpr int NT = 64;
static long checked = 0, bad = 0;

static bool ref_half_empty(int fw, int half) {      // byte 2 h + c of the little-endian word is column c of half h; bit 0 counts
    std::uint32_t u;
    std::memcpy(&u, &fw, 4);
    return (((u >> (8 * (2 * half))) & 1u) == 0u) && (((u >> (8 * (2 * half + 1))) & 1u) == 0u);
}

struct Row {
    std::unique_ptr<int[]> w{new int[NT]};
    long loads = 0, oob = 0;
    int last = -1;
    int load(int i) {
        if (i < 0 || i >= NT) { ++oob; return -1; }
        ++loads;
        last = i;
        return w[i];
    }
};

static void check_walks(Row& row, const char* what) {
    for (int step : {1, 8, 32}) {
        for (int half = 0; half < 2; ++half) {
            for (int ct0 = 0; ct0 < NT + step + 1; ++ct0) {
                if (ct0 >= step && ct0 < NT - 1) continue;          // (starts a workgroup can have, then the end and past it)
                // a workgroup's walk: start, then from behind every tile found, as the kernel's loop does
                int ct = ct0;
                for (;;) {
                    int ref = ct;
                    long looked = 0;
                    while (ref < NT) { ++looked; if (!ref_half_empty(row.w[ref], half)) break; ref += step; }
                    const int sentinel = 0x5a5a5a5a;
                    int fw = sentinel;
                    row.loads = 0;
                    row.last = -1;
                    const int got = hgs::tile2_next_nonempty([&](int i) { return row.load(i); }, ct, step, NT, half, &fw);
                    ++checked;
                    bool ok = row.oob == 0 && row.loads == looked;
                    if (ref < NT) ok = ok && got == ref && fw == row.w[ref] && row.last == ref;
                    else ok = ok && got >= NT && fw == sentinel;
                    if (!ok) {
                        if (bad++ < 10) std::printf("%s: step %d half %d from %d: got %d (word %08x, %ld loads, %ld out of range), expected %d (%ld loads)\n",
                                                    what, step, half, ct, got, (unsigned)fw, row.loads, row.oob, ref, looked);
                        row.oob = 0;
                    }
                    if (got >= NT) break;
                    ct = got + step;
                }
            }
        }
    }
}

// word of a tile: bit 0 of the four column bytes from `act` (bit k = column k), everything else from `fill`
static int word(unsigned act, std::uint32_t fill) {
    std::uint32_t u = fill & 0xfefefefeu;
    for (int k = 0; k < 4; ++k) u |= ((act >> k) & 1u) << (8 * k);
    int w;
    std::memcpy(&w, &u, 4);
    return w;
}

int main() {
    Row row;
    const std::uint32_t fills[] = {0x00000000u, 0xfefefefeu, 0x06040200u, 0x80fe0002u};
    // stride 1: one word of every pattern in an empty row; pairs; empty; full
    for (std::uint32_t fill : fills) {
        for (int pos = 0; pos < NT; ++pos)
            for (unsigned act = 0; act < 16; ++act) {
                for (int i = 0; i < NT; ++i) row.w[i] = word(0, fill);
                row.w[pos] = word(act, fill);
                check_walks(row, "single");
            }
        for (int i = 0; i < NT; ++i) row.w[i] = word(0, fill);
        check_walks(row, "empty");
        for (int i = 0; i < NT; ++i) row.w[i] = word(15, fill);
        check_walks(row, "full");
    }
    for (int p = 0; p < NT; ++p)
        for (int q = p + 1; q < NT; ++q) {
            for (int i = 0; i < NT; ++i) row.w[i] = word(0, fills[(p + q) & 3]);
            row.w[p] = word(1u << (p & 3), fills[q & 3]);
            row.w[q] = word(1u << (q & 3), fills[p & 3]);
            check_walks(row, "pair");
        }
    // the last byte of the last word alone (column 1 of half 1 of tile 63)
    for (int i = 0; i < NT; ++i) row.w[i] = 0;
    row.w[NT - 1] = word(8, 0);
    check_walks(row, "last byte");
    // no flags: every word -1
    for (int i = 0; i < NT; ++i) row.w[i] = -1;
    check_walks(row, "no flags");
    // strides 8 and 32: every empty / non-empty pattern of the tiles a walk visits, each filling of a non-empty half
    for (int step : {8, 32}) {
        const int nv = NT / step;
        for (int start = 0; start < step; start += (step == 8 ? 1 : 5))
            for (unsigned pat = 0; pat < (1u << nv); ++pat)
                for (unsigned filling = 1; filling < 4; ++filling)
                    for (int f = 0; f < 4; ++f) {
                        // (the tiles the walk does not visit are full: stepping onto one would be seen)
                        for (int i = 0; i < NT; ++i) row.w[i] = word(15, fills[f]);
                        for (int k = 0; k < nv; ++k) {
                            const bool on = (pat >> k) & 1u;
                            // half 0 carries the pattern, half 1 its complement: both halves are walked
                            const unsigned a0 = on ? filling : 0u, a1 = on ? 0u : filling;
                            row.w[start + k * step] = word(a0 | (a1 << 2), fills[(f + k) & 3]);
                        }
                        // only the walks that start on this residue see the pattern; the others see full rows, which is checked too
                        check_walks(row, step == 8 ? "stride 8" : "stride 32");
                    }
    }
    // pseudo-random rows, every density
    std::uint64_t s = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (std::uint32_t)(s >> 33); };
    for (int n = 0; n < 4000; ++n) {
        const unsigned dens = 1 + n % 63;
        for (int i = 0; i < NT; ++i) {
            unsigned act = 0;
            for (int k = 0; k < 4; ++k) act |= (rnd() % 64 < dens ? 1u : 0u) << k;
            row.w[i] = word(act, rnd());
        }
        check_walks(row, "random");
    }
    std::printf("checked %ld bad %ld\n", checked, bad);
    return bad ? 1 : 0;
}
