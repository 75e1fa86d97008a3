// Host replay of cgemm_streamk's control flow (slmsuite_amd/csrc/cgemm.hpp) against the tables of
// slmsuite_amd/csrc/streamk_schedule.hpp, for tests/test_streamk_schedule.py.  No HIP: the schedule header is plain C++.
//
//   streamk_schedule_host case TM TN KT G   -> one JSON line: what the schedule looks like and how many checks it violates
//   streamk_schedule_host sweep             -> every (tiles_m, tiles_n) in 1..6, KT in 1..40, G in 1..min(total, 64), then
//                                              "checked <cases> bad <violations>"
//
// The replay walks, per workgroup, exactly what the kernel walks: lo / hi, (tile, kt) from lo, per step `more`, the
// advance to (ntile, nkt), and the store when nkt == 0 || !more with seg = w - first_wg[tile].  Checked (the letters are
// those of the test's docstring):
//   a  every workgroup has lo < hi (G <= total)
//   b  every k-step of every tile is accumulated exactly once, into accumulators that hold nothing of another tile,
//      and nothing is left unstored when a workgroup ends
//   c  every (tile, seg) is stored exactly once, 0 <= seg < nseg[tile] <= planes
//   d  the segs of a tile are exactly 0 .. nseg - 1 (the consumers add that prefix) and between them hold KT steps
//   e  planes == max nseg
//   f  EPI 1: slot < tiles_n * 2 * planes; and the last element either epilogue writes, for the last of two holograms,
//      lies inside what sk_c_elems / sk_part_elems size the buffers to
//   g  first_wg[t] + nseg[t] - 1 == sk_owner(last step of t)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "streamk_schedule.hpp"

using namespace hgs;

struct Shape {
    int G = 0, planes = 0;
    long long whole = 0;      // workgroups whose range holds at least one whole tile
    long long cross = 0;      // workgroups whose range touches more than one tile
    long long aligned = 0;    // stores with nkt == 0 and !more at once: the range ends on a tile boundary
    long long mid = 0;        // stores with nkt == 0 and more: accumulators cleared inside a range
    long long prefetch = 0;   // steps that prefetch their successor (more)
    long long maxlen = 0;     // longest range
    long long bad = 0;
};

static int g_shown = 0;
static void violation(Shape& s, const char* what, int tm, int tn, int KT, int G, long long a = 0, long long b = 0) {
    ++s.bad;
    if (g_shown++ < 20) fprintf(stdout, "violation %s: tiles %d x %d KT %d G %d (%lld, %lld)\n", what, tm, tn, KT, G, a, b);
}

static Shape replay(int tm, int tn, int KT, int G) {
    Shape s;
    const int tiles = tm * tn;
    const long long total = (long long)tiles * KT;
    std::vector<int> first(tiles), nseg(tiles);
    const int planes = sk_fill(tiles, KT, G, first.data(), nseg.data());
    s.G = G;
    s.planes = planes;
    // a ragged problem of these tile counts, two holograms: what the engine would allocate for it
    const int CG = 128, B = 2;
    const long long M = (long long)tm * CG - 5, N = (long long)tn * CG - 7, ldP = (long long)tm * CG;
    const long long c_elems = (long long)sk_c_elems(B, planes, (size_t)M, (size_t)N);
    const long long part_elems = (long long)sk_part_elems(B, tn, planes, (size_t)ldP);

    std::vector<int> acc((size_t)total, 0);                    // accumulations per (tile, kt)
    std::vector<int> stored((size_t)tiles * (planes + 1), 0);  // stores per (tile, seg), seg clipped to `planes` for the count
    std::vector<long long> held((size_t)tiles, 0);             // steps that reached a store of the tile
    int max_nseg = 1;
    for (int t = 0; t < tiles; ++t) {
        if (nseg[t] > max_nseg) max_nseg = nseg[t];
        if (nseg[t] < 1 || nseg[t] > planes) violation(s, "c: nseg outside 1..planes", tm, tn, KT, G, t, nseg[t]);
        if (first[t] + nseg[t] - 1 != sk_owner((long long)(t + 1) * KT - 1, total, G))
            violation(s, "g: last owner", tm, tn, KT, G, t, first[t] + nseg[t] - 1);
    }
    if (planes != max_nseg) violation(s, "e: planes != max nseg", tm, tn, KT, G, planes, max_nseg);

    for (int w = 0; w < G; ++w) {
        const long long lo = sk_begin(total, G, w), hi = sk_begin(total, G, w + 1);
        if (lo >= hi) {
            if (G <= total) violation(s, "a: empty range", tm, tn, KT, G, w, lo);
            continue;
        }
        if (hi - lo > s.maxlen) s.maxlen = hi - lo;
        int tile = (int)(lo / KT), kt = (int)(lo - (long long)tile * KT);
        long long pending = 0;       // steps in the accumulators
        int pending_tile = -1, n_stores = 0;
        bool whole = false;
        for (long long it = lo; it < hi; ++it) {
            const bool more = it + 1 < hi;
            int ntile = tile, nkt = kt + 1;
            if (nkt == KT) { nkt = 0; ntile = tile + 1; }
            if (more) ++s.prefetch;
            if (tile < 0 || tile >= tiles) { violation(s, "b: tile outside the grid", tm, tn, KT, G, w, tile); break; }
            if (pending > 0 && pending_tile != tile) violation(s, "b: accumulators hold another tile", tm, tn, KT, G, w, tile);
            ++acc[(size_t)tile * KT + kt];
            ++pending;
            pending_tile = tile;
            if (nkt == 0 || !more) {
                const int seg = w - first[tile];
                ++n_stores;
                if (nkt == 0 && !more) ++s.aligned;
                if (nkt == 0 && more) ++s.mid;
                if (pending == KT) whole = true;
                if (seg < 0 || seg >= nseg[tile] || seg >= planes) {
                    violation(s, "c: seg outside 0..nseg-1", tm, tn, KT, G, tile, seg);
                } else {
                    ++stored[(size_t)tile * (planes + 1) + seg];
                    held[tile] += pending;
                }
                if (seg >= 0) {
                    const int m0 = (tile % tm) * CG, n0 = (tile / tm) * CG;
                    // EPI 0: C[(b * planes + seg) * M * N + m * N + n], the tile's last valid element of the last hologram
                    const long long mlast = (m0 + CG <= M ? m0 + CG : M) - 1, nlast = (n0 + CG <= N ? n0 + CG : N) - 1;
                    const long long c_at = ((long long)(B - 1) * planes + seg) * M * N + mlast * N + nlast;
                    if (c_at >= c_elems) violation(s, "f: C store past sk_c_elems", tm, tn, KT, G, c_at, c_elems);
                    // EPI 1: part[(b * tiles_n * 2 * planes + slot) * ldP + m], both wave columns
                    for (int wn = 0; wn < 2; ++wn) {
                        const long long slot = ((long long)(n0 / CG) * 2 + wn) * planes + seg;
                        if (slot >= (long long)tn * 2 * planes) violation(s, "f: slot", tm, tn, KT, G, slot, (long long)tn * 2 * planes);
                        const long long p_at = ((long long)(B - 1) * tn * 2 * planes + slot) * ldP + mlast;
                        if (p_at >= part_elems) violation(s, "f: part store past sk_part_elems", tm, tn, KT, G, p_at, part_elems);
                    }
                }
                pending = 0;         // clear()
            }
            tile = ntile; kt = nkt;
        }
        if (pending != 0) violation(s, "b: steps left unstored", tm, tn, KT, G, w, pending);
        if (n_stores > 1) ++s.cross;
        if (whole) ++s.whole;
    }
    for (long long i = 0; i < total; ++i)
        if (acc[(size_t)i] != 1) violation(s, "b: step not accumulated exactly once", tm, tn, KT, G, i, acc[(size_t)i]);
    for (int t = 0; t < tiles; ++t) {
        for (int sg = 0; sg < nseg[t] && sg < planes; ++sg)
            if (stored[(size_t)t * (planes + 1) + sg] != 1)
                violation(s, "d: seg of the prefix not stored exactly once", tm, tn, KT, G, t, sg);
        if (held[t] != KT) violation(s, "d: the planes of a tile do not hold KT steps", tm, tn, KT, G, t, held[t]);
    }
    return s;
}

int main(int argc, char** argv) {
    if (argc == 6 && !strcmp(argv[1], "case")) {
        const int tm = atoi(argv[2]), tn = atoi(argv[3]), KT = atoi(argv[4]);
        int G = atoi(argv[5]);
        const long long total = (long long)tm * tn * KT;
        if (tm < 1 || tn < 1 || KT < 1 || G < 1) return 2;
        if (G > total) G = (int)total;        // what the engine launches
        const Shape s = replay(tm, tn, KT, G);
        printf("{\"G\": %d, \"planes\": %d, \"whole\": %lld, \"cross\": %lld, \"aligned\": %lld, \"mid\": %lld, \"prefetch\": %lld, "
               "\"maxlen\": %lld, \"bad\": %lld}\n", s.G, s.planes, s.whole, s.cross, s.aligned, s.mid, s.prefetch, s.maxlen, s.bad);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "sweep")) {
        long long checked = 0, bad = 0;
        for (int tm = 1; tm <= 6; ++tm)
            for (int tn = 1; tn <= 6; ++tn)
                for (int KT = 1; KT <= 40; ++KT) {
                    const long long total = (long long)tm * tn * KT;
                    for (int G = 1; G <= 64 && G <= total; ++G) {
                        bad += replay(tm, tn, KT, G).bad;
                        ++checked;
                    }
                }
        printf("checked %lld bad %lld\n", checked, bad);
        return 0;
    }
    fprintf(stderr, "usage: %s case TM TN KT G | sweep\n", argv[0]);
    return 2;
}
