// The stream-K schedule of cgemm_streamk (cgemm.hpp), as plain functions: which steps a workgroup walks, which workgroup
// owns a step, and per output tile the first workgroup and the number of partial planes its k-steps are spread over.
// Plain C++ -- no HIP, no engine state, no device -- so that the kernel, the engine's tables (CompressedBackend::sk_retable) and
// the microbenchmark share one statement of it and the schedule can be swept without a GPU
// (tests/test_streamk_schedule.py replays the kernel's control flow against these tables).
//
// The (output tile, k tile) iteration space is one line of total = tiles * KT steps, tile-major.  Workgroup w of G takes
// [sk_begin(w), sk_begin(w + 1)).  With G <= total every workgroup owns at least one step and the owners of a tile are
// consecutive: w - first[tile] is the plane a workgroup stores its share of `tile` to, and the consumers
// (sep_n2f_sum, sep_f2n_finish) add planes 0 .. nseg[tile] - 1.
#pragma once
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HGS_SK_HD __host__ __device__
#else
#define HGS_SK_HD
#endif

namespace hgs {

HGS_SK_HD inline long long sk_begin(long long total, int G, int w) { return total * w / G; }
// workgroup whose range [sk_begin(w), sk_begin(w + 1)) holds step idx
HGS_SK_HD inline int sk_owner(long long idx, long long total, int G) {
    long long w = idx * G / total;
    while (sk_begin(total, G, (int)w + 1) <= idx) ++w;
    while (sk_begin(total, G, (int)w) > idx) --w;
    return (int)w;
}

// first[t] = owner of step 0 of tile t, nseg[t] = number of workgroups that hold steps of it; returns the largest nseg:
// the number of planes the partial results need (CgemmSkArgs::planes, the size of the consumers' input)
inline int sk_fill(int tiles, int KT, int G, int* first, int* nseg) {
    const long long total = (long long)tiles * KT;
    int planes = 1;
    for (int t = 0; t < tiles; ++t) {
        first[t] = sk_owner((long long)t * KT, total, G);
        nseg[t] = sk_owner((long long)(t + 1) * KT - 1, total, G) - first[t] + 1;
        if (nseg[t] > planes) planes = nseg[t];
    }
    return planes;
}

// What the partial results take, in float2 elements, for `batch` holograms:
//   EPI 0 (f2n) stores C[(b * planes + seg) * M * N + m * N + n];
//   EPI 1 (n2f) stores part[(b * tiles_n * 2 * planes + slot) * ldP + m], slot = (tile column * 2 + wave column) * planes + seg.
inline size_t sk_c_elems(int batch, int planes, size_t M, size_t N) { return (size_t)batch * planes * M * N; }
inline size_t sk_part_elems(int batch, int tiles_n, int planes, size_t ldP) { return (size_t)batch * tiles_n * 2 * planes * ldP; }

}  // namespace hgs
