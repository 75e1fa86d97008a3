// Kernels of hgs_remove_vortices: find the phase vortices of the stored farfield phase inside the eroded target mask and
// subtract them (analysis.image_vortices :1207-1237, image_vortices_coordinates :1240-1267, image_remove_vortices
// :1270-1309 of the reference; Hologram._remove_vortices, _hologram.py:961-998).
//
//   dd_a = mod(diff(phase, axis = a, prepend = nan) - pi, 2 pi),  a = 0 (rows), 1 (columns)
//   winding(y, x) = rint(-(dd0[y, x] - dd1[y, x] - dd0[y, x - 1] + dd1[y - 1, x]) / 2 pi),  NaN -> 0 (row 0 and column 0)
//   mask = binary_erosion(target > 0, ones((5, 5))): the whole 5 x 5 neighbourhood inside the grid with target > 0
//   phase -= sum over the vortices (xv, yv, w) inside the mask of  w * atan2(x - xv, y - yv)      (x first: the reference's
//   argument order; x, y the un-centred pixel indices of _generate_grid; the result is not wrapped)
//
// phase_ff and the target are P-sized arrays in the engine's layout: pixel (y, x) sits at x * Ph + col_pos(y, lane_T).  Every
// kernel here enumerates MEMORY positions, so that neighbouring lanes touch neighbouring addresses, and recovers (y, x) from
// the position.
//
// The vortex list comes out in memory order without an atomic append: vortex_find_kernel counts per block (pass 0), a
// single-block scan turns the counts into offsets and leaves the total on the device, and the same kernel scatters
// (pass 1).  The winding number is evaluated in double for either element type, in the reference's order of operations:
// on float64 input it is the reference's own arithmetic, on float32 input the exact differences of the stored values.
//
// vortex_remove_kernel is bound by the vector ALU (K atan2 per pixel): a lane owns VX_PIX pixels, the list is staged
// through LDS in chunks of VX_CHUNK (every lane reads the same entry: a broadcast), the sum is kept in double (one
// conversion and one add per term next to the ~25 operations of the atan2; it takes the summation order out of the
// float32 error) and phase_ff is read and written once per pixel.
#pragma once
#include "kernels.hpp"

namespace hgs {

constexpr int VX_WG = 256;        // lanes per block of every kernel here
constexpr int VX_PIX = 4;         // pixels per lane of the removal
constexpr int VX_CHUNK = 1024;    // list entries staged per LDS round: 12 KiB of float, 24 KiB of double
constexpr int VX_SCAN_WG = 1024;

struct VxGeo { int Ph, Pw, lane_T; };

// (y, x) of memory position i of a P-sized array (the inverse of x * Ph + col_pos(y, lane_T))
__device__ __forceinline__ void vx_pixel(const VxGeo& g, size_t i, int* y, int* x) {
    const int xx = (int)(i / (size_t)g.Ph), pos = (int)(i - (size_t)xx * g.Ph);
    *x = xx;
    *y = g.lane_T > 0 ? pos / 16 + (pos % 16) * g.lane_T : pos;
}
__device__ __forceinline__ size_t vx_at(const VxGeo& g, int y, int x) { return (size_t)x * g.Ph + col_pos(y, g.lane_T); }

// numpy's mod(v - pi, 2 pi) (npy_divmod: fmod, then the divisor's sign)
__device__ __forceinline__ double vx_wrap(double v) {
    double m = ::fmod(v - 3.141592653589793, 6.283185307179586);
    if (m != 0 && m < 0) m += 6.283185307179586;
    return m;
}

template <typename R> struct VortexFindArgs {
    const R* pff;          // [P] stored farfield phase
    const R* t;            // [P] target (NaN = MRAF noise region: outside the mask)
    unsigned* counts;      // [gridDim.x] pass 0: out, vortices of each block; pass 1: in, the exclusive offsets of the scan
    int32_t* list;         // [cap][3] (x, y, w), pass 1
    unsigned cap;
    int pass;
    size_t P;
    VxGeo g;
};

// winding number of the plaquette (y-1..y, x-1..x) if (y, x) lies inside the eroded mask, else 0
template <typename R> __device__ __forceinline__ int vx_winding(const VortexFindArgs<R>& a, int y, int x) {
    const VxGeo& g = a.g;
    if (y < 2 || x < 2 || y > g.Ph - 3 || x > g.Pw - 3) return 0;      // the 5 x 5 neighbourhood leaves the grid (and row / column 0)
    const double p11 = (double)a.pff[vx_at(g, y, x)], p01 = (double)a.pff[vx_at(g, y - 1, x)];
    const double p10 = (double)a.pff[vx_at(g, y, x - 1)], p00 = (double)a.pff[vx_at(g, y - 1, x - 1)];
    const double s = -(vx_wrap(p11 - p01) - vx_wrap(p11 - p10) - vx_wrap(p10 - p00) + vx_wrap(p01 - p00)) / 6.283185307179586;
    if (!(::fabs(s) < 1.0e9)) return 0;                               // NaN (or a non-finite phase): no vortex
    const int w = (int)::rint(s);
    if (w == 0) return 0;
    for (int dx = -2; dx <= 2; ++dx)
        for (int dy = -2; dy <= 2; ++dy)
            if (!(a.t[vx_at(g, y + dy, x + dx)] > (R)0)) return 0;
    return w;
}

template <typename R> __global__ __launch_bounds__(VX_WG) void vortex_find_kernel(VortexFindArgs<R> a) {
    __shared__ unsigned wave_n[VX_WG / 64];
    const size_t i = (size_t)blockIdx.x * VX_WG + threadIdx.x;
    int y = 0, x = 0, w = 0;
    if (i < a.P) {
        vx_pixel(a.g, i, &y, &x);
        w = vx_winding<R>(a, y, x);
    }
    const unsigned long long ballot = __ballot(w != 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_n[wave] = (unsigned)__popcll(ballot);
    __syncthreads();
    unsigned before = 0, total = 0;
    for (int k = 0; k < VX_WG / 64; ++k) {
        if (k < wave) before += wave_n[k];
        total += wave_n[k];
    }
    if (a.pass == 0) {
        if (threadIdx.x == 0) a.counts[blockIdx.x] = total;
        return;
    }
    if (w != 0) {
        const unsigned k = a.counts[blockIdx.x] + before + (unsigned)__popcll(ballot & ((1ull << lane) - 1ull));
        if (k < a.cap) {
            a.list[3 * (size_t)k + 0] = x;
            a.list[3 * (size_t)k + 1] = y;
            a.list[3 * (size_t)k + 2] = w;
        }
    }
}

// counts[n] -> exclusive offsets in place, the total to *count.  One block: a lane sums a contiguous run, the run sums are
// scanned in LDS, the lane writes its run back.
template <int WG> __global__ __launch_bounds__(WG) void vortex_scan_kernel(unsigned* counts, unsigned n, int32_t* count) {
    __shared__ unsigned run[WG];
    const unsigned per = (n + WG - 1) / WG;
    const unsigned lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
    unsigned s = 0;
    for (unsigned k = lo; k < hi; ++k) s += counts[k];
    run[threadIdx.x] = s;
    __syncthreads();
    for (unsigned d = 1; d < WG; d <<= 1) {           // inclusive scan
        const unsigned v = threadIdx.x >= d ? run[threadIdx.x - d] : 0u;
        __syncthreads();
        run[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned off = run[threadIdx.x] - s;
    for (unsigned k = lo; k < hi; ++k) {
        const unsigned c = counts[k];
        counts[k] = off;
        off += c;
    }
    if (threadIdx.x == WG - 1) *count = (int32_t)run[WG - 1];
}

// atan2(a, b) of the removal.  float: the arguments are differences of pixel indices -- finite, integer valued, |.| < 2^24 --
// so ocml's atan2f pays for what cannot happen here (frexp / ldexp scaling around the division, the infinity and NaN
// classes: 45 vector operations per call, measured in the ISA); this one is min / max, one v_rcp_f32, an odd polynomial
// on [0, 1] (atan v = v + v t p(t), t = v^2, p of degree 7 fitted for relative error: 7.7e-8 absolute, 1.0e-7 relative
// over 2e6 float32 arguments against float64 atan) and three selects.  atan2(0, 0) = 0 as in NumPy.  double: ocml's.
template <typename R> __device__ __forceinline__ R vx_atan2(R a, R b) { return Math<R>::atan2(a, b); }
template <> __device__ __forceinline__ float vx_atan2<float>(float a, float b) {
    const float aa = fabsf(a), ab = fabsf(b);
    const float mx = fmaxf(fmaxf(aa, ab), 1.0f), mn = fminf(aa, ab);       // (mx < 1 only at the vortex itself: 0 / 1)
    const float v = mn * __builtin_amdgcn_rcpf(mx), t = v * v;
    float p = fmaf(t, 0.0029206459876149893f, -0.01636774279177189f);
    p = fmaf(t, p, 0.04321156442165375f);
    p = fmaf(t, p, -0.07552189379930496f);
    p = fmaf(t, p, 0.10665993392467499f);
    p = fmaf(t, p, -0.14211052656173706f);
    p = fmaf(t, p, 0.19993773102760315f);
    p = fmaf(t, p, -0.33333152532577515f);
    float r = fmaf(v, t * p, v);
    r = aa > ab ? 1.5707963267948966f - r : r;
    r = b < 0.0f ? 3.14159265358979323846f - r : r;
    return copysignf(r, a);
}

template <typename R> struct VortexRemoveArgs {
    R* pff;                  // [P] in / out
    const int32_t* list;     // [*count][3] (x, y, w)
    const int32_t* count;    // device resident
    size_t P;
    VxGeo g;
};

template <typename R> __global__ __launch_bounds__(VX_WG) void vortex_remove_kernel(VortexRemoveArgs<R> a) {
    __shared__ R vx[VX_CHUNK], vy[VX_CHUNK], vw[VX_CHUNK];
    const int n = *a.count;
    const size_t first = ((size_t)blockIdx.x * VX_WG + threadIdx.x) * VX_PIX;
    R fx[VX_PIX], fy[VX_PIX];
    double acc[VX_PIX];
#pragma unroll
    for (int p = 0; p < VX_PIX; ++p) {
        int y = 0, x = 0;
        if (first + p < a.P) vx_pixel(a.g, first + p, &y, &x);
        fx[p] = (R)x;
        fy[p] = (R)y;
        acc[p] = 0;
    }
    for (int base = 0; base < n; base += VX_CHUNK) {
        const int m = min(VX_CHUNK, n - base);
        __syncthreads();                                        // the previous chunk has been consumed
        for (int k = threadIdx.x; k < m; k += VX_WG) {
            const int32_t* e = a.list + 3 * (size_t)(base + k);
            vx[k] = (R)e[0];
            vy[k] = (R)e[1];
            vw[k] = (R)e[2];
        }
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const R xv = vx[k], yv = vy[k], w = vw[k];
#pragma unroll
            for (int p = 0; p < VX_PIX; ++p) acc[p] += (double)(w * vx_atan2<R>(fx[p] - xv, fy[p] - yv));
        }
    }
#pragma unroll
    for (int p = 0; p < VX_PIX; ++p)
        if (first + p < a.P) a.pff[first + p] = (R)((double)a.pff[first + p] - acc[p]);
}

// launch front-ends (launch_vortex_f32.hip / launch_vortex_f64.hip); they note their instance in the dispatch record and
// return hipError_t as int
template <typename R> int launch_vortex_find(hipStream_t s, const VortexFindArgs<R>& a);
template <typename R> int launch_vortex_remove(hipStream_t s, const VortexRemoveArgs<R>& a);
int launch_vortex_scan(hipStream_t s, unsigned* counts, unsigned n, int32_t* count);     // (defined next to the float32 pair)

inline unsigned vortex_find_blocks(size_t P) { return (unsigned)((P + VX_WG - 1) / VX_WG); }

}  // namespace hgs
