// Kernel of hgs_poly_eval / hgs_set_array_poly: SLM-sized phase masks rastered from a few polynomial coefficients -- what
// toolbox.phase.polynomial (phase.py:1672-1795) and zernike_sum (:964-1166) of the reference form on the host.  For N stacked
// masks over S = H * W pixels
//     out[n][p] = sum_m w[m][n] xs(p)^a_m ys(p)^b_m  (+ v[n] atan2(ys, xs), the vortex plate, where v[n] > 0),
//     xs = x * x_scale,  ys = y * y_scale.
// The host folds terms and weights into a dense triangle c[n][b][a], a + b <= deg (row b holds deg - b + 1 coefficients),
// and the kernel runs Horner's scheme over it -- in x within a row, in y over the rows -- in double whatever the grid's type:
// (deg + 1)(deg + 2) / 2 multiply-adds per value, rounded ONCE to the grid's type G and stored as O (G itself, or the type of
// the engine array the mask fills: a double correction from a float grid holds the float values widened, as the host route
// through a NumPy array does).  The triangle is the same for every lane: the compiler reads it through the scalar cache.
//
// The pupil predicate  square(x * x_scale) + square(y * y_scale) <= 1  decides a SET that has to equal the reference's, so it
// is evaluated in G with NumPy's roundings: the product, each square and the sum round on their own, the scales rounded to G
// first (a Python float meets a float32 array as float32).  No contraction there: poly_inside says so itself.
//
// Coordinates come as two axis vectors xs[W], ys[H] (PROD: a product grid, nothing SLM-sized is read) or as the two full [S]
// arrays (rotated or calibrated grids).  A mask's S values start at element n * S of the output, which is 16-byte aligned
// only for some shapes and some caller pointers: the lanes store quads aligned by ADDRESS (one 16-byte store of float, two of
// double); the up to three values before a mask's first aligned quad and the up to three after its last one are taken one
// by one by a single lane, as in display_kernels.hpp.  S = 1 and W < 4 are nothing special: pixels are indexed flat.
#pragma once
#include <cstdint>
#include "kernels.hpp"

namespace hgs {

constexpr int POLY_WG = 256;
constexpr int POLY_PIX = 4;          // values per lane
constexpr int POLY_MAX_DEG = 20;     // a + b <= 20: 231 coefficients per mask (radial order 10 of the Zernike basis needs 10)

enum { POLY_MASK_NONE = 0, POLY_MASK_ZERO = 1, POLY_MASK_NAN = 2 };

__host__ __device__ inline int poly_table_len(int deg) { return (deg + 1) * (deg + 2) / 2; }

template <typename G, typename O> struct PolyArgs {
    O* out;                // [N][S]
    const G* x;            // PROD: [W], else [S]
    const G* y;            // PROD: [H], else [S]
    const double* table;   // [N][T] c[n][b][a], T = poly_table_len(deg); row b starts at b * (deg + 1) - b * (b - 1) / 2
    const double* vortex;  // [N] weights of the vortex plate (only positive ones act), or nullptr
    size_t S;
    int W;
    int deg;
    int mask_mode;
    double x_scale, y_scale;
};

// the reference's  np.square(x * sx) + np.square(y * sy) <= 1  in the grid's own precision, every operation rounded
template <typename G> __device__ __forceinline__ bool poly_inside(G x, G y, G sx, G sy) {
#pragma clang fp contract(off)
    const G xs = x * sx;
    const G ys = y * sy;
    const G xx = xs * xs;
    const G yy = ys * ys;
    const G r2 = xx + yy;
    return r2 <= (G)1;
}

// one value: c the mask's triangle, v its vortex weight (0: none)
template <typename G> __device__ __forceinline__ G poly_value(const double* __restrict__ c, int deg, double v, int mask_mode,
                                                              G x, G y, double x_scale, double y_scale) {
    if (mask_mode != POLY_MASK_NONE && !poly_inside<G>(x, y, (G)x_scale, (G)y_scale))
        return mask_mode == POLY_MASK_NAN ? (G)NAN : (G)0;
    const double xs = (double)x * x_scale, ys = (double)y * y_scale;
    double acc = 0.0;
    int row = poly_table_len(deg) - 1;                 // row b = deg holds one coefficient, the last of the triangle
    for (int b = deg; b >= 0; --b) {
        const int na = deg - b;                        // highest power of x in this row
        double inner = c[row + na];
        for (int a = na - 1; a >= 0; --a) inner = ::fma(inner, xs, c[row + a]);
        acc = ::fma(acc, ys, inner);
        row -= na + 2;                                 // row b - 1 is one longer
    }
    if (v > 0.0) acc = ::fma(v, ::atan2(ys, xs), acc);
    return (G)acc;
}

// pixel p of the grid and, through next(), the ones after it: a product grid is read by (row, column), one division per lane
template <typename G, bool PROD> struct PolyCursor {
    const G* xp;
    const G* yp;
    size_t p;
    unsigned W, col;
    __device__ __forceinline__ PolyCursor(const G* x, const G* y, int W_, size_t p0) : xp(x), yp(y), p(p0), W((unsigned)W_), col(0) {
        if (PROD) {
            const size_t r = p0 <= 0xffffffffull ? (size_t)((unsigned)p0 / W) : p0 / W;
            col = (unsigned)(p0 - r * W);
            p = r;                                     // (PROD: p is the row)
        }
    }
    __device__ __forceinline__ G x() const { return PROD ? xp[col] : xp[p]; }
    __device__ __forceinline__ G y() const { return yp[p]; }
    __device__ __forceinline__ void next() {
        if (PROD) { if (++col == W) { col = 0; ++p; } }
        else ++p;
    }
};

// where mask n's aligned quads start and how many there are: pixels [0, head) and [head + 4 nq, S) are the loose ones
struct PolySpan { size_t head, nq; };
template <typename O> __device__ __forceinline__ PolySpan poly_span(const O* base, size_t S) {
    PolySpan d;
    const size_t el = ((uintptr_t)base / sizeof(O)) & (POLY_PIX - 1);     // (16 bytes hold four floats; a double quad starts on 32)
    d.head = (POLY_PIX - el) & (POLY_PIX - 1);
    if (d.head > S) d.head = S;
    d.nq = (S - d.head) / POLY_PIX;
    return d;
}
inline size_t poly_lanes(size_t S) { return S / POLY_PIX + 1; }          // every quad a mask can hold, and the loose-pixel lane

// grid (ceil(poly_lanes(S) / POLY_WG), N): lane i < nq forms quad i of mask blockIdx.y, lane nq the loose pixels
template <typename G, typename O, bool PROD> __global__ __launch_bounds__(POLY_WG) void poly_kernel(PolyArgs<G, O> a) {
    typedef O o2 __attribute__((ext_vector_type(2)));
    typedef O o4 __attribute__((ext_vector_type(4)));
    const int n = blockIdx.y;
    const double* c = a.table + (size_t)n * poly_table_len(a.deg);
    const double v = a.vortex ? a.vortex[n] : 0.0;
    O* out = a.out + (size_t)n * a.S;
    const PolySpan sp = poly_span<O>(out, a.S);
    const size_t i = (size_t)blockIdx.x * POLY_WG + threadIdx.x;
    if (i < sp.nq) {
        const size_t k = sp.head + POLY_PIX * i;
        PolyCursor<G, PROD> at(a.x, a.y, a.W, k);
        O r[POLY_PIX];
#pragma unroll
        for (int j = 0; j < POLY_PIX; ++j) {
            r[j] = (O)poly_value<G>(c, a.deg, v, a.mask_mode, at.x(), at.y(), a.x_scale, a.y_scale);
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
            const PolyCursor<G, PROD> at(a.x, a.y, a.W, k);
            out[k] = (O)poly_value<G>(c, a.deg, v, a.mask_mode, at.x(), at.y(), a.x_scale, a.y_scale);
        }
    }
}

// launch front-ends (launch_poly_f32.hip / launch_poly_f64.hip hold the instances of one grid type G); they note the
// instance in the dispatch record and return hipError_t as int.  PolyArgs<G, void> is what the engine fills (out as void*);
// out_bytes: sizeof(O), 4 or 8
template <typename G> int launch_poly(int n_masks, bool product, int out_bytes, hipStream_t s, const PolyArgs<G, void>& a);

}  // namespace hgs
