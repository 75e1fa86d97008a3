// Kernel of hgs_pattern_eval / hgs_set_array_pattern: the analytic masks of the reference's toolbox.phase that are no
// polynomials -- sinusoid and binary gratings (phase.py:78-258), the quadrant masks built from gratings (:261-389), axicon
// (:455-498), Laguerre-Gauss and Hermite-Gauss mode masks (:1842-1935).  blaze and lens are polynomials and run through
// poly_kernel; only inside a quadrant mask is a blaze formed here.
//
//   MODE          value at (x, y)
//   PAT_BLAZE     kx x + ky y                                       (kx = 2 pi vx, ky = 2 pi vy; quadrant masks only)
//   PAT_SINUSOID  half (1 + sin(kx x + ky y + shift)) + base        (half = (a - b) / 2, base = b)
//   PAT_BINARY    a where the decision quantity d > 0 or |d| <= 1e-8, else b   (see pattern_binary_on)
//   PAT_AXICON    2 pi sqrt((x kx)^2 + (y ky)^2); 2 pi k |x| or 2 pi k |y| where the other component of k vanishes
//   PAT_LG        l atan2(x, y) + pi [L_p^|l|(s (x^2 + y^2)) < 0]   (s = 16 / w^2; each term only for l != 0, p != 0)
//   PAT_HG        pi where H_n(s x) H_m(s y) > 0, else 0            (s = 4 / w)
//
// Continuous values are formed in double whatever the grid's type G and rounded once (round_g: to G, then stored as O; masks
// whose type in the reference is float64 for either grid are stored unrounded).  L_p^alpha and H_n run their three-term
// recurrences in double.  The decision quantity of a binary grating selects a SET that has to be the reference's, so it is
// formed with NumPy's roundings in the type NumPy forms it in -- G, or double where the vector came as float64 scalars or
// counts pixels -- with every product and sum rounded on its own and no contraction.
//
// QUAD (grating modes): the lane picks one of four parameter sets by its row and column -- windows that start at row H/2 and
// column W/2, in the order top-right, bottom-right, top-left, bottom-left -- and writes 0 into the last row and the last
// column: the reference clips a window's end to H - 1 and W - 1, so an even side loses them as an odd one does.  The parameters are the same for every lane and travel by value: they arrive through the scalar path.
//
// Coordinates and stores are those of poly_kernels.hpp: axis vectors (PROD) or full arrays; quads aligned by address, the
// loose values before the first and after the last one by a single lane.
#pragma once
#include <cstdint>
#include "poly_kernels.hpp"

namespace hgs {

enum { PAT_BLAZE = 0, PAT_SINUSOID = 1, PAT_BINARY = 2, PAT_AXICON = 3, PAT_LG = 4, PAT_HG = 5, PAT_MODES = 6 };
constexpr int PAT_MAX_ORDER = POLY_MAX_DEG;     // p, n, m <= 20

constexpr double PAT_TWO_PI = 6.283185307179586476925286766559;
constexpr double PAT_PI = 3.141592653589793238462643383279;

// one window's grating: kx = 2 pi vx, ky = 2 pi vy (binary counting pixels: 2 pi / period), and binary's two levels
struct PatSet { double kx, ky, a, b; };

template <typename G, typename O> struct PatArgs {
    O* out;                // [S]
    const G* x;            // PROD: [W], else [S]
    const G* y;            // PROD: [H], else [S]
    size_t S;
    int W, H;
    int quad;              // grating modes: four windows, set[0 .. 3]; else set[0] everywhere
    int round_g;           // the value is rounded to G before it is stored
    int dec_double;        // PAT_BINARY: d is formed in double (else in G)
    int pixel_mask;        // PAT_BINARY: bit i -- set i takes the pixel indices (within its window) for coordinates
    int l, p, n, m;        // PAT_LG: l, p;  PAT_HG: n, m
    double shift;          // gratings
    double off;            // PAT_BINARY: 2 pi (1 - duty_cycle)
    double half, base;     // PAT_SINUSOID
    double kx, ky;         // PAT_AXICON: w / fx / 2, w / fy / 2
    double s;              // PAT_LG: 16 / w^2;  PAT_HG: 4 / w
    PatSet set[4];
};

// NumPy's mod for b > 0: fmod is exact; a negative remainder moves up by b, rounded in D
template <typename D> __device__ __forceinline__ D pattern_mod(D a, D b) {
#pragma clang fp contract(off)
    D m = sizeof(D) == 4 ? (D)::fmodf((float)a, (float)b) : (D)::fmod((double)a, (double)b);
    if (m != (D)0) {
        if (m < (D)0) m = m + b;
    } else {
        m = (D)0;
    }
    return m;
}

// binary(): d = mod(kx x + ky y + shift, 2 pi); d = 0 where isclose(d, 2 pi); d -= 2 pi (1 - duty); on where d > 0 or
// isclose(d, 0) -- in D with the roundings of NumPy's array expression: the Python scalars meet the array in ITS type, the
// in-place subtraction of the float64 scalar is formed in double and rounded back
template <typename D> __device__ __forceinline__ bool pattern_binary_on(D x, D y, double kx, double ky, double shift, double off) {
#pragma clang fp contract(off)
    const D tx = (D)kx * x;
    const D ty = (D)ky * y;
    D d = tx + ty;
    d = d + (D)shift;
    d = pattern_mod<D>(d, (D)PAT_TWO_PI);
    D gap = d - (D)PAT_TWO_PI;
    gap = gap < (D)0 ? -gap : gap;
    if (gap <= (D)(1e-8 + 1e-5 * PAT_TWO_PI) || d == (D)PAT_TWO_PI) d = (D)0;
    d = (D)((double)d - off);
    const D mag = d < (D)0 ? -d : d;
    return d > (D)0 || mag <= (D)1e-8;
}

// generalised Laguerre L_p^alpha(t): (k + 1) L_{k+1} = (2k + 1 + alpha - t) L_k - (k + alpha) L_{k-1}
__device__ __forceinline__ double pattern_laguerre(int p, int alpha, double t) {
    double lm = 1.0, lk = 1.0 + alpha - t;
    if (p == 0) return lm;
    for (int k = 1; k < p; ++k) {
        const double ln = ((2 * k + 1 + alpha - t) * lk - (k + alpha) * lm) / (double)(k + 1);
        lm = lk; lk = ln;
    }
    return lk;
}

// physicists' Hermite H_n(t): H_{k+1} = 2 t H_k - 2 k H_{k-1}
__device__ __forceinline__ double pattern_hermite(int n, double t) {
    double hm = 1.0, hk = 2.0 * t;
    if (n == 0) return hm;
    for (int k = 1; k < n; ++k) {
        const double hn = 2.0 * t * hk - 2.0 * k * hm;
        hm = hk; hk = hn;
    }
    return hk;
}

// member `get` of set[i]: selects over constant indices, not an indexed read -- the sets stay in scalar registers
#define HGS_PAT_PICK(a, i, get) ((i) == 3 ? (a).set[3].get : (i) == 2 ? (a).set[2].get : (i) == 1 ? (a).set[1].get : (a).set[0].get)

// one value, in double; row and col: the pixel
template <typename G, typename O, int MODE>
__device__ __forceinline__ double pattern_value(const PatArgs<G, O>& a, G xg, G yg, unsigned row, unsigned col) {
    const double x = (double)xg, y = (double)yg;
    if (MODE == PAT_BLAZE || MODE == PAT_SINUSOID || MODE == PAT_BINARY) {
        int which = 0;
        unsigned wr = row, wc = col;                     // pixel within its window
        if (a.quad) {
            const unsigned hh = (unsigned)a.H / 2, hw = (unsigned)a.W / 2;
            if (row + 1 >= (unsigned)a.H || col + 1 >= (unsigned)a.W) return 0.0;      // (the clipped end of the windows)
            const bool right = col >= hw, bottom = row >= hh;
            which = (right ? 0 : 2) + (bottom ? 1 : 0);
            if (right) wc -= hw;
            if (bottom) wr -= hh;
        }
        const double gkx = HGS_PAT_PICK(a, which, kx), gky = HGS_PAT_PICK(a, which, ky);
        if (MODE == PAT_BLAZE) return ::fma(gkx, x, gky * y);
        if (MODE == PAT_SINUSOID) return a.half * (1.0 + ::sin(::fma(gkx, x, gky * y) + a.shift)) + a.base;
        const bool pixels = (a.pixel_mask >> which) & 1;
        bool on;
        if (sizeof(G) == 8 || a.dec_double || pixels)
            on = pattern_binary_on<double>(pixels ? (double)wc : x, pixels ? (double)wr : y, gkx, gky, a.shift, a.off);
        else
            on = pattern_binary_on<G>(xg, yg, gkx, gky, a.shift, a.off);
        return on ? HGS_PAT_PICK(a, which, a) : HGS_PAT_PICK(a, which, b);
    }
    if (MODE == PAT_AXICON) {
        if (a.kx == 0.0) return (PAT_TWO_PI * a.ky) * ::fabs(y);
        if (a.ky == 0.0) return (PAT_TWO_PI * a.kx) * ::fabs(x);
        const double u = x * a.kx, v = y * a.ky;
        return PAT_TWO_PI * ::sqrt(::fma(u, u, v * v));
    }
    if (MODE == PAT_LG) {
        double v = 0.0;
        if (a.l != 0) v = (double)a.l * ::atan2(x, y);
        if (a.p != 0) {
            const double q = pattern_laguerre(a.p, a.l < 0 ? -a.l : a.l, a.s * ::fma(y, y, x * x));
            if (q < 0.0) v += PAT_PI;
        }
        return v;
    }
    const double q = pattern_hermite(a.n, a.s * x) * pattern_hermite(a.m, a.s * y);
    return q > 0.0 ? PAT_PI : 0.0;
}

// pixel p of the grid, its row and column, and through next() the ones after it: one division per lane
template <typename G, bool PROD> struct PatCursor {
    const G* xp;
    const G* yp;
    size_t p;
    unsigned W, col, row;
    __device__ __forceinline__ PatCursor(const G* x, const G* y, int W_, size_t p0) : xp(x), yp(y), p(p0), W((unsigned)W_) {
        const size_t r = p0 <= 0xffffffffull ? (size_t)((unsigned)p0 / W) : p0 / W;
        col = (unsigned)(p0 - r * W);
        row = (unsigned)r;
    }
    __device__ __forceinline__ G x() const { return PROD ? xp[col] : xp[p]; }
    __device__ __forceinline__ G y() const { return PROD ? yp[row] : yp[p]; }
    __device__ __forceinline__ void next() {
        ++p;
        if (++col == W) { col = 0; ++row; }
    }
};

template <typename G, typename O, bool PROD, int MODE>
__device__ __forceinline__ O pattern_at(const PatArgs<G, O>& a, const PatCursor<G, PROD>& at) {
    const double v = pattern_value<G, O, MODE>(a, at.x(), at.y(), at.row, at.col);
    return a.round_g ? (O)(G)v : (O)v;
}

// grid ceil(poly_lanes(S) / POLY_WG): lane i < nq forms quad i, lane nq the loose pixels (no loop over the grid: one trip)
template <typename G, typename O, bool PROD, int MODE> __global__ __launch_bounds__(POLY_WG) void pattern_kernel(PatArgs<G, O> a) {
    typedef O o2 __attribute__((ext_vector_type(2)));
    typedef O o4 __attribute__((ext_vector_type(4)));
    O* out = a.out;
    const PolySpan sp = poly_span<O>(out, a.S);
    const size_t i = (size_t)blockIdx.x * POLY_WG + threadIdx.x;
    if (i < sp.nq) {
        const size_t k = sp.head + POLY_PIX * i;
        PatCursor<G, PROD> at(a.x, a.y, a.W, k);
        O r[POLY_PIX];
#pragma unroll
        for (int j = 0; j < POLY_PIX; ++j) {
            r[j] = pattern_at<G, O, PROD, MODE>(a, at);
            if (j + 1 < POLY_PIX) at.next();
        }
        if (sizeof(O) == 4) {
            o4 q;
            q.x = r[0]; q.y = r[1]; q.z = r[2]; q.w = r[3];
            *reinterpret_cast<o4*>(out + k) = q;
        } else {
            o2 q0, q1;
            q0.x = r[0]; q0.y = r[1]; q1.x = r[2]; q1.y = r[3];
            *reinterpret_cast<o2*>(out + k) = q0;
            *reinterpret_cast<o2*>(out + k + 2) = q1;
        }
    } else if (i == sp.nq) {
        for (size_t k = 0; k < a.S; ++k) {
            if (k == sp.head) k += POLY_PIX * sp.nq;          // skip the quads
            if (k >= a.S) break;
            const PatCursor<G, PROD> at(a.x, a.y, a.W, k);
            out[k] = pattern_at<G, O, PROD, MODE>(a, at);
        }
    }
}

// launch front-ends (launch_pattern_f32.hip / launch_pattern_f64.hip hold the instances of one grid type G); they note the
// instance in the dispatch record (quad as a flag) and return hipError_t as int.  PatArgs<G, void> is what the engine fills
template <typename G> int launch_pattern(int mode, bool product, int out_bytes, hipStream_t s, const PatArgs<G, void>& a);

}  // namespace hgs
