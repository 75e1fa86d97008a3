// Host check of tile2_next_listed() of slmsuite_amd/csrc/tile_flags.hpp (tests/test_tile_list.py builds and runs it, with
// -fsanitize=address,undefined): the walk col_tile2_kernel makes over the POSITIONS of the scan's tile list (ColArgs::tile_list),
// played for every workgroup of a grid exactly as the kernel's loop plays it, against the flag words themselves and against the
// static walk over all tiles (tile2_next_nonempty).
//   * flag words and list live in heap blocks of exactly their size and the loaders refuse every other index;
//   * grids of 2, 4, ..., 16 workgroups with the kernel's plain pairing (workgroups 2 i and 2 i + 1 take the halves of one
//     position) and, at 16, its XCD pairing as well;
//   * every bit-0 pattern of the bytes of rows of 1 - 5 tiles (16^n rows), every empty / non-empty pattern of the halves of rows of
//     6 tiles (4^6, the filling of a non-empty half and the bits above bit 0 rotating), and 3,000 pseudo-random rows of 64 tiles of
//     every density;
//   * what must hold: every non-empty half tile is visited exactly once, hence by exactly one workgroup; a workgroup's visits
//     ascend; no empty half tile is visited; the visits are those of the static walk; the word handed back is the tile's; with
//     no more listed tiles than workgroup pairs no workgroup visits two; "none left" returns the tile count and leaves the word.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "tile_flags.hpp"

static long checked = 0, bad = 0;

static bool ref_half_empty(int fw, int half) {      // byte 2 h + c of the little-endian word is column c of half h; bit 0 counts
    std::uint32_t u;
    std::memcpy(&u, &fw, 4);
    return (((u >> (8 * (2 * half))) & 1u) == 0u) && (((u >> (8 * (2 * half + 1))) & 1u) == 0u);
}

struct Row {
    int nt;
    std::unique_ptr<int[]> w, list;
    int nlist = 0;
    long oob = 0;
    explicit Row(int n) : nt(n), w(new int[n]), list(new int[n]) {}
    int load(int i) {
        if (i < 0 || i >= nt) { ++oob; return 0; }
        return w[i];
    }
    int at(int p) {
        if (p < 0 || p >= nlist) { ++oob; return 0; }
        return list[p];
    }
    // what the device kernel writes with the scan: the ascending tiles with bit 0 set in any byte
    void build() {
        nlist = 0;
        for (int t = 0; t < nt; ++t)
            if (hgs::tile2_listed(w[t])) list[nlist++] = t;
    }
};

static void fail(const char* what, int G, int xmap, const char* why, int a, int b) {
    if (bad++ < 12) std::printf("%s: grid %d xmap %d: %s (%d, %d)\n", what, G, xmap, why, a, b);
}

static void check_grid(Row& row, int G, bool xmap, const char* what) {
    const int nt = row.nt, step = G / 2;
    std::vector<int> seen_list(2 * nt, 0), seen_walk(2 * nt, 0), owner(2 * nt, -1);
    for (int x = 0; x < G; ++x) {
        int half, ct0;
        if (xmap) { const int xcd = x & 7, idx = x >> 3; half = idx & 1; ct0 = (idx >> 1) * 8 + xcd; }
        else { half = x & 1; ct0 = x >> 1; }
        const int sentinel = 0x5a5a5a5a;
        // the list walk, as the kernel's loop: first position, then from behind every position found
        int pos = ct0, fw = sentinel, prev = -1, visits = 0;
        int ct = hgs::tile2_next_listed([&](int p) { return row.at(p); }, [&](int i) { return row.load(i); }, &pos, step, row.nlist, nt, half, &fw);
        while (ct < nt) {
            if (ct < 0) { fail(what, G, xmap, "negative tile", x, ct); break; }
            if (fw != row.w[ct]) fail(what, G, xmap, "word of another tile", x, ct);
            if (pos < 0 || pos >= row.nlist || row.list[pos] != ct || (pos - ct0) % step != 0) fail(what, G, xmap, "position does not name the tile", x, pos);
            if (ct <= prev) fail(what, G, xmap, "visits do not ascend", x, ct);
            prev = ct;
            ++visits;
            ++seen_list[2 * ct + half];
            owner[2 * ct + half] = x;
            int fwn = sentinel;
            pos += step;
            const int ctn = hgs::tile2_next_listed([&](int p) { return row.at(p); }, [&](int i) { return row.load(i); }, &pos, step, row.nlist, nt, half, &fwn);
            if (ctn >= nt && (ctn != nt || fwn != sentinel || pos < row.nlist)) fail(what, G, xmap, "none left: tile count, word untouched, position past the list", x, ctn);
            ct = ctn;
            fw = fwn;
        }
        if (visits == 0 && ct != nt) fail(what, G, xmap, "no visit must return the tile count", x, ct);
        if (row.nlist <= step && visits > 1) fail(what, G, xmap, "two visits with no more listed tiles than pairs", x, visits);
        // the static walk of the same workgroup
        int fs = sentinel;
        int cs = hgs::tile2_next_nonempty([&](int i) { return row.load(i); }, ct0, step, nt, half, &fs);
        while (cs < nt) {
            ++seen_walk[2 * cs + half];
            cs = hgs::tile2_next_nonempty([&](int i) { return row.load(i); }, cs + step, step, nt, half, &fs);
        }
    }
    ++checked;
    if (row.oob) { fail(what, G, xmap, "load outside the row or the list", (int)row.oob, 0); row.oob = 0; }
    for (int t = 0; t < nt; ++t)
        for (int h = 0; h < 2; ++h) {
            const int want = ref_half_empty(row.w[t], h) ? 0 : 1;
            if (seen_list[2 * t + h] != want) fail(what, G, xmap, want ? "non-empty half tile not visited exactly once" : "empty half tile visited", t, h);
            if (seen_walk[2 * t + h] != seen_list[2 * t + h]) fail(what, G, xmap, "not the visits of the static walk", t, h);
        }
}

static void check_row(Row& row, const char* what) {
    row.build();
    for (int G = 2; G <= 16; G += 2) check_grid(row, G, false, what);
    check_grid(row, 16, true, what);
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
    const std::uint32_t fills[] = {0x00000000u, 0xfefefefeu, 0x06040200u, 0x80fe0002u};
    // 1 - 5 tiles: every bit-0 pattern of every byte
    for (int n = 1; n <= 5; ++n) {
        Row row(n);
        const long total = 1l << (4 * n);
        for (long pat = 0; pat < total; ++pat) {
            for (int i = 0; i < n; ++i) row.w[i] = word((unsigned)(pat >> (4 * i)) & 15u, fills[(pat + i) & 3]);
            check_row(row, "exhaustive");
        }
    }
    {   // 6 tiles: every empty / non-empty pattern of the twelve halves
        Row row(6);
        for (unsigned pat = 0; pat < (1u << 12); ++pat) {
            for (int i = 0; i < 6; ++i) {
                const unsigned filling = 1 + (pat + i) % 3;          // column 0, column 1, both
                const unsigned a0 = ((pat >> (2 * i)) & 1u) ? filling : 0u, a1 = ((pat >> (2 * i + 1)) & 1u) ? filling : 0u;
                row.w[i] = word(a0 | (a1 << 2), fills[(pat + i) & 3]);
            }
            check_row(row, "six tiles");
        }
    }
    // 64 tiles, pseudo-random, every density; then empty, full, the first and the last byte alone
    Row row(64);
    std::uint64_t s = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (std::uint32_t)(s >> 33); };
    for (int n = 0; n < 3000; ++n) {
        const unsigned dens = 1 + n % 63;
        for (int i = 0; i < 64; ++i) {
            unsigned act = 0;
            for (int k = 0; k < 4; ++k) act |= (rnd() % 64 < dens ? 1u : 0u) << k;
            row.w[i] = word(act, rnd());
        }
        check_row(row, "random");
    }
    for (int i = 0; i < 64; ++i) row.w[i] = word(0, fills[i & 3]);
    check_row(row, "empty");
    for (int i = 0; i < 64; ++i) row.w[i] = word(15, fills[i & 3]);
    check_row(row, "full");
    for (int i = 0; i < 64; ++i) row.w[i] = 0;
    row.w[0] = word(1, 0);
    check_row(row, "first byte");
    row.w[0] = 0;
    row.w[63] = word(8, 0);
    check_row(row, "last byte");
    std::printf("checked %ld bad %ld\n", checked, bad);
    return bad ? 1 : 0;
}
