// Kernels of hgs_get_display: the gray levels an SLM takes, straight from the device phase -- Hologram.get_phase
// (_hologram.py:786-811), the float branch of SLM.set_phase (hardware/slms/slm.py:664-681) and SLM._phase2gray (:695-783) of
// the reference, to the bit.  R = 2^bitdepth, s = phase_scaling; per pixel
//   p = phase + pi (rounded to the engine's precision; with a kernel requested: phase + kernel, no pi)     in the engine's type
//   x = (double)p (+ correction)                                                                           in double from here
//   y = x * f,   f = -(R * s / 2 / pi)
//   s == 1:  m = max y;  m >= 0: y -= R * 2 * ceil(m / R);   out = ((int64)rint(y) - 1) & (R - 1)
//   s != 1:  min y <= -R or max y > 0:  y -= 1;  y = mod(y, R s) (NumPy's: fmod, then the divisor's sign);  y += R (1 - s);
//                                       s > 1: y < 0 -> R - 1
//            otherwise:                 y += R - 1
//            out = y truncated toward zero
// Every product and every sum rounds on its own: the data-dependent shift of the s == 1 branch moves values onto rounding
// ties, so a contracted multiply-add gives other levels (the translation units are built without contraction, and the
// functions below say so themselves).  max and min of doubles do not depend on the order of the reduction.
//
// Two launches, nothing read by the host in between: phase_range_kernel leaves per-block (max, min) pairs of y -- at most
// DISP_RANGE_BLOCKS per hologram --, every block of phase_display_kernel folds them first (one pair per lane) and converts.
// Both are bandwidth bound.  A hologram's S pixels start at element b * S of the batch, which is a multiple of four only
// for some shapes, so the lanes work on quads aligned in the WHOLE array: a quad moves as one 16-byte load of float phase
// (2 x 16 of double) and one packed store (a dword of uint8, 8 bytes of uint16); the up to three pixels before the first
// aligned quad of a hologram and the up to three after its last one are taken one by one by a single lane.  The kernel and
// the correction are indexed per hologram: vector loads where the hologram starts on a quad, element by element otherwise.
#pragma once
#include <type_traits>
#include "kernels.hpp"

namespace hgs {

constexpr int DISP_WG = 256;
constexpr int DISP_PIX = 4;              // pixels per lane
constexpr int DISP_RANGE_BLOCKS = 256;   // most blocks of the range pass per hologram (= pairs a display block folds: one per lane)

template <typename R> struct DisplayArgs {
    const R* phase;        // [B][S]
    const R* kern;         // [S] propagation kernel, or nullptr: p = phase + pi
    const double* corr;    // [S] wavefront correction, or nullptr
    double* partial;       // [B][range_blocks][2] (max, min) of y
    void* out;             // [B][S] uint8 (bits <= 8) or uint16
    size_t S;
    int range_blocks;      // grid.x of the range pass
    int unit;              // s == 1
    int fill;              // s > 1
    double f;              // -(R * s / 2 / pi)
    double res;            // R
    double period;         // R * s
    double lift;           // R * (1 - s)
};

// where hologram b's aligned quads start and how many there are: elements [lo, lo + head) and [lo + head + 4 nq, lo + S)
// are the loose ones
struct DispSpan { size_t lo, head, nq; };
__device__ __forceinline__ DispSpan disp_span(size_t S, int b) {
    DispSpan d;
    d.lo = (size_t)b * S;
    d.head = (DISP_PIX - (d.lo & (DISP_PIX - 1))) & (DISP_PIX - 1);
    if (d.head > S) d.head = S;
    d.nq = (S - d.head) / DISP_PIX;
    return d;
}
inline size_t disp_lanes(size_t S) { return S / DISP_PIX + 1; }      // every quad a hologram can hold, and the loose-pixel lane

// y of a pixel: ph its phase value, kn its kernel value (unused without a kernel), cr its correction (unused without one)
template <typename R> __device__ __forceinline__ double disp_y(const DisplayArgs<R>& a, R ph, R kn, double cr) {
#pragma clang fp contract(off)
    const R p = a.kern ? ph + kn : ph + (R)3.14159265358979323846;
    double x = (double)p;
    if (a.corr) x = x + cr;
    return x * a.f;
}
template <typename R> __device__ __forceinline__ double disp_y_at(const DisplayArgs<R>& a, const R* ph, size_t k) {
    return disp_y<R>(a, ph[k], a.kern ? a.kern[k] : (R)0, a.corr ? a.corr[k] : 0.0);
}

// four consecutive elements; vec: p is aligned to the four of them (one 16-byte access of float, two of double)
template <typename T> __device__ __forceinline__ void disp_load4(const T* p, T (&v)[4], bool vec = true) {
    typedef T t4 __attribute__((ext_vector_type(4)));
    if (vec) {
        const t4 q = *reinterpret_cast<const t4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    }
}
// y of the aligned quad that starts at pixel k of the hologram
template <typename R> __device__ __forceinline__ void disp_y4(const DisplayArgs<R>& a, const R* ph, size_t k, bool head0, double (&y)[4]) {
    R v[4], kn[4] = {(R)0, (R)0, (R)0, (R)0};
    double cr[4] = {0.0, 0.0, 0.0, 0.0};
    disp_load4<R>(ph + k, v);
    if (a.kern) disp_load4<R>(a.kern + k, kn, head0);        // (k is a multiple of four only where the hologram starts on one)
    if (a.corr) disp_load4<double>(a.corr + k, cr, head0);
#pragma unroll
    for (int j = 0; j < DISP_PIX; ++j) y[j] = disp_y<R>(a, v[j], kn[j], cr[j]);
}

__device__ __forceinline__ void disp_wave_range(double& mx, double& mn) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ox = __shfl_xor(mx, d), on = __shfl_xor(mn, d);
        mx = ox > mx ? ox : mx;
        mn = on < mn ? on : mn;
    }
}
// (max, min) over the block, valid in every lane; scratch: 2 * DISP_WG / 64 doubles
__device__ __forceinline__ void disp_block_range(double& mx, double& mn, double* scratch) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    disp_wave_range(mx, mn);
    if (lane == 0) { scratch[2 * wid] = mx; scratch[2 * wid + 1] = mn; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < DISP_WG / 64; ++k) {
        const double ox = scratch[2 * k], on = scratch[2 * k + 1];
        mx = ox > mx ? ox : mx;
        mn = on < mn ? on : mn;
    }
}

// grid (range_blocks, B): the lanes stride over the quads of hologram blockIdx.y; lane 0 of block 0 also takes the loose pixels
template <typename R> __global__ __launch_bounds__(DISP_WG) void phase_range_kernel(DisplayArgs<R> a) {
    __shared__ double scratch[2 * DISP_WG / 64];
    const int b = blockIdx.y;
    const DispSpan sp = disp_span(a.S, b);
    const R* ph = a.phase + sp.lo;
    double mx = -INFINITY, mn = INFINITY;
    const size_t stride = (size_t)gridDim.x * DISP_WG;
    for (size_t q = (size_t)blockIdx.x * DISP_WG + threadIdx.x; q < sp.nq; q += stride) {
        const size_t k = sp.head + DISP_PIX * q;
        double y[4];
        disp_y4<R>(a, ph, k, sp.head == 0, y);
#pragma unroll
        for (int j = 0; j < DISP_PIX; ++j) {
            mx = y[j] > mx ? y[j] : mx;
            mn = y[j] < mn ? y[j] : mn;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (size_t k = 0; k < a.S; ++k) {
            if (k == sp.head) k += DISP_PIX * sp.nq;          // skip the quads
            if (k >= a.S) break;
            const double y = disp_y_at<R>(a, ph, k);
            mx = y > mx ? y : mx;
            mn = y < mn ? y : mn;
        }
    }
    disp_block_range(mx, mn, scratch);
    if (threadIdx.x == 0) {
        double* o = a.partial + 2 * ((size_t)b * a.range_blocks + blockIdx.x);
        o[0] = mx;
        o[1] = mn;
    }
}

// what the extremes select, the same for every pixel of a hologram
struct DispRule {
    double shift;     // s == 1: R * 2 * ceil(m / R) where m >= 0, else 0 (nothing is subtracted then)
    int shifted;      // s == 1: m >= 0
    int wrap;         // s != 1: the mod branch
};

template <typename R> __device__ __forceinline__ unsigned disp_level(const DisplayArgs<R>& a, const DispRule& r, double y) {
#pragma clang fp contract(off)
    const long long mask = (long long)a.res - 1;
    if (a.unit) {
        if (r.shifted) y = y - r.shift;
        return (unsigned)((((long long)::rint(y)) - 1) & mask);
    }
    if (r.wrap) {
        y = y - 1.0;
        double m = ::fmod(y, a.period);
        if (m != 0 && m < 0) m = m + a.period;
        y = m + a.lift;
        if (a.fill && y < 0) y = a.res - 1.0;
    } else {
        y = y + (a.res - 1.0);
    }
    return (unsigned)(long long)y;
}

// grid (ceil(disp_lanes(S) / DISP_WG), B): lane i < nq converts quad i of hologram blockIdx.y, lane nq the loose pixels
template <typename R, int BITS> __global__ __launch_bounds__(DISP_WG) void phase_display_kernel(DisplayArgs<R> a) {
    using O = typename std::conditional<BITS == 8, uint8_t, uint16_t>::type;
    typedef O o4 __attribute__((ext_vector_type(4)));
    __shared__ double scratch[2 * DISP_WG / 64];
    const int b = blockIdx.y;
    double mx = -INFINITY, mn = INFINITY;
    if ((int)threadIdx.x < a.range_blocks) {
        const double* pr = a.partial + 2 * ((size_t)b * a.range_blocks + threadIdx.x);
        mx = pr[0];
        mn = pr[1];
    }
    disp_block_range(mx, mn, scratch);
    DispRule r;
    r.shifted = mx >= 0;
    r.shift = a.res * 2.0 * ::ceil(mx / a.res);
    r.wrap = mn <= -a.res || mx > 0;

    const DispSpan sp = disp_span(a.S, b);
    const R* ph = a.phase + sp.lo;
    O* out = reinterpret_cast<O*>(a.out) + sp.lo;
    const size_t i = (size_t)blockIdx.x * DISP_WG + threadIdx.x;
    if (i < sp.nq) {
        const size_t k = sp.head + DISP_PIX * i;
        double y[4];
        disp_y4<R>(a, ph, k, sp.head == 0, y);
        o4 g;
        g.x = (O)disp_level<R>(a, r, y[0]);
        g.y = (O)disp_level<R>(a, r, y[1]);
        g.z = (O)disp_level<R>(a, r, y[2]);
        g.w = (O)disp_level<R>(a, r, y[3]);
        *reinterpret_cast<o4*>(out + k) = g;
    } else if (i == sp.nq) {
        for (size_t k = 0; k < a.S; ++k) {
            if (k == sp.head) k += DISP_PIX * sp.nq;          // skip the quads
            if (k >= a.S) break;
            out[k] = (O)disp_level<R>(a, r, disp_y_at<R>(a, ph, k));
        }
    }
}

// launch front-ends (launch_display_f32.hip / launch_display_f64.hip); launch_display notes its instance in the dispatch
// record; both return hipError_t as int.  bits16: uint16 output.
template <typename R> int launch_display_range(int batch, hipStream_t s, const DisplayArgs<R>& a);
template <typename R> int launch_display(int batch, bool bits16, hipStream_t s, const DisplayArgs<R>& a);

inline int display_range_blocks(size_t S) {
    const size_t need = (S / DISP_PIX + DISP_WG - 1) / DISP_WG;
    return (int)(need < 1 ? 1 : need > (size_t)DISP_RANGE_BLOCKS ? (size_t)DISP_RANGE_BLOCKS : need);
}

}  // namespace hgs
