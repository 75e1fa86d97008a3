// Host check of slmsuite_amd/csrc/tile_flags.hpp (tests/test_tile_flags.py builds and runs it, with -fsanitize=address,undefined):
// the two decoders of a tile's flag word against the obvious definition -- take the word apart into its four bytes, byte k is
// column k of the tile, half tile h owns bytes 2 h and 2 h + 1, a column is active when bit 0 of its byte is set -- over all
// 2^16 values of either half word, with several fillings of the other half, and for the word -1 ("no flags").
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "tile_flags.hpp"

static bool ref_active(int fw, int half, int c) {
    unsigned char bytes[4];
    std::uint32_t u;
    std::memcpy(&u, &fw, 4);
    for (int k = 0; k < 4; ++k) bytes[k] = (unsigned char)((u >> (8 * k)) & 0xffu);      // (little-endian word: byte k = column k)
    return (bytes[2 * half + c] & 1) != 0;
}
static bool ref_half_empty(int fw, int half) { return !ref_active(fw, half, 0) && !ref_active(fw, half, 1); }

// (constant expressions: the kernel's uses fold where the word is known)
static_assert(hgs::tile2_col_active(-1, 0, 0) && hgs::tile2_col_active(-1, 1, 1), "-1: every column active");
static_assert(!hgs::tile2_half_empty(-1, 0) && !hgs::tile2_half_empty(-1, 1), "-1: no half tile empty");
static_assert(hgs::tile2_half_empty(0x0001fefe, 0) && !hgs::tile2_half_empty(0x0001fefe, 1), "bit 0 of each byte only");

int main() {
    long checked = 0, bad = 0;
    const std::uint32_t other[] = {0x0000u, 0xffffu, 0x0101u, 0xfefeu, 0x0001u, 0x0100u, 0xa5a5u, 0x8080u};
    auto check = [&](int fw) {
        for (int half = 0; half < 2; ++half) {
            for (int c = 0; c < 2; ++c) {
                ++checked;
                if (hgs::tile2_col_active(fw, half, c) != ref_active(fw, half, c)) {
                    if (bad++ < 10) std::printf("col_active(%08x, %d, %d) = %d\n", (unsigned)fw, half, c, (int)hgs::tile2_col_active(fw, half, c));
                }
            }
            ++checked;
            if (hgs::tile2_half_empty(fw, half) != ref_half_empty(fw, half)) {
                if (bad++ < 10) std::printf("half_empty(%08x, %d) = %d\n", (unsigned)fw, half, (int)hgs::tile2_half_empty(fw, half));
            }
        }
    };
    for (std::uint32_t hw = 0; hw < 0x10000u; ++hw) {
        for (std::uint32_t o : other) {
            for (int where = 0; where < 2; ++where) {
                const std::uint32_t u = where ? (hw << 16) | o : (o << 16) | hw;
                int fw;
                std::memcpy(&fw, &u, 4);
                check(fw);
            }
        }
    }
    check(-1);
    // -1 by the definition itself: every column fetched, no half tile skipped
    for (int half = 0; half < 2; ++half) {
        if (hgs::tile2_half_empty(-1, half)) ++bad;
        for (int c = 0; c < 2; ++c)
            if (!hgs::tile2_col_active(-1, half, c)) ++bad;
    }
    std::printf("checked %ld bad %ld\n", checked, bad);
    return bad ? 1 : 0;
}
