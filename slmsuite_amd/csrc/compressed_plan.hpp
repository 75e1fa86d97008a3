// What the host decides about a compressed (CompressedSpotHologram) problem, each decision spelled once: the canonical
// slot of a term, what a term list allows, whether the uploaded grids are a product of two axes and whether the x axis is
// regular, how the run kernels chunk the spots, and which kernel form transforms.  Pure host C++ -- no HIP, no engine
// state, no device -- so that the choices can be read here and tested without a GPU (tests/test_compressed_plan.py);
// CompressedBackend (compressed_backend.hpp) fills the facts and executes what comes out.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hgs {

// ---- terms ---------------------------------------------------------------------------------------------------------
// slot of the term x^px y^py, px + py <= 2, in the canonical order [1, x, y, x2, xy, y2] of the degree-specialised
// kernels; the coefficients of repeated terms accumulate in their slot
inline int canonical_slot(int px, int py) {
    return (px == 0 && py == 0) ? 0 : (px == 1 && py == 0) ? 1 : (px == 0 && py == 1) ? 2 : (px == 2) ? 3 : (px == 1) ? 4 : 5;
}

// canonical coefficients of spot n from its [M][N] term weights: out[slot * stride] += coeff[m][n]; out starts zeroed
template <typename Tc, typename To>
inline void canonical_coeffs(const int32_t* mono, int M, const Tc* coeff, int N, int n, To* out, size_t stride = 1) {
    for (int m = 0; m < M; ++m) out[canonical_slot(mono[2 * m], mono[2 * m + 1]) * stride] += (To)coeff[(size_t)m * N + n];
}

struct TermClass {
    int degree = 0;          // what the kernels are chosen by: max(px + py), at least 3 with a vortex plate (general kernels)
    int bad = -1;            // index of the first unrecognised term (a negative exponent other than the vortex plate's), or -1
    bool separable = true;   // phi_n(x, y) = fx_n(x) + fy_n(y): no negative exponent, no cross term, each exponent <= sep_maxdeg
    int dx = 0, dy = 0;      // ... and the degrees of fx, fy
};
// mono: [M][2] (px, py).  The only pseudo-term is the vortex plate (-1, 0).  With an unrecognised term, `degree` is what
// the terms before it give.
inline TermClass classify_terms(const int32_t* mono, int M, int sep_maxdeg) {
    TermClass t;
    for (int m = 0; m < M; ++m) t.degree = std::max(t.degree, (int)(mono[2 * m] + mono[2 * m + 1]));
    for (int m = 0; m < M; ++m) {
        const int px = mono[2 * m], py = mono[2 * m + 1];
        if (px < 0 || py < 0 || (px > 0 && py > 0) || px > sep_maxdeg || py > sep_maxdeg) t.separable = false;
        t.dx = std::max(t.dx, px);
        t.dy = std::max(t.dy, py);
    }
    for (int m = 0; m < M; ++m) {
        const int px = mono[2 * m], py = mono[2 * m + 1];
        if (px == -1 && py == 0) { t.degree = std::max(t.degree, 3); continue; }
        if (px < 0 || py < 0) { t.bad = m; break; }
    }
    return t;
}

// ---- grids ---------------------------------------------------------------------------------------------------------
// Product grid?  The uploaded [H][W] x grid (axis 0) must depend on the column only, the y grid (axis 1) on the row only;
// values are compared exactly.  `out` gets the axis either way: row 0 of x, column 0 of y.
template <typename T> inline bool product_grid_axis(const T* h, int H, int W, int axis, std::vector<double>& out) {
    bool sep = true;
    if (axis == 0) {
        for (int y = 1; y < H && sep; ++y)
            for (int x = 0; x < W; ++x)
                if (h[(size_t)y * W + x] != h[x]) { sep = false; break; }
        out.assign(W, 0.0);
        for (int x = 0; x < W; ++x) out[x] = (double)h[x];
    } else {
        for (int y = 0; y < H && sep; ++y)
            for (int x = 1; x < W; ++x)
                if (h[(size_t)y * W + x] != h[(size_t)y * W]) { sep = false; break; }
        out.assign(H, 0.0);
        for (int y = 0; y < H; ++y) out[y] = (double)h[(size_t)y * W];
    }
    return sep;
}

// The run kernels step along x by a recurrence: x_k = x0 + k * hx.  The uploaded values are fp32 roundings of the grid,
// half an ulp of the largest coordinate each; fewer than two columns define no step.
struct RegularAxis { bool ok = false; double x0 = 0, hx = 0; };
inline RegularAxis regular_axis(const double* xs, int W) {
    RegularAxis r;
    if (W < 2) return r;
    r.x0 = xs[0];
    r.hx = (xs[W - 1] - r.x0) / (double)(W - 1);
    double xmax = 0;
    for (int x = 0; x < W; ++x) xmax = std::max(xmax, std::fabs(xs[x]));
    for (int x = 0; x < W; ++x)
        if (std::fabs(xs[x] - (r.x0 + x * r.hx)) > 2.5e-7 * xmax + 1e-30) return r;
    r.ok = true;
    return r;
}

// ---- run kernels: spot chunks (grid.z) -----------------------------------------------------------------------------
// about eight waves per SIMD over run_blocks workgroups of one wave, at most eight chunks, whole groups of 64 spots
struct RunChunks { int nper = 0, chunks = 1; };
inline RunChunks run_chunking(int N, int n_cu, int run_blocks) {
    int want = std::max(1, (8 * 4 * n_cu + run_blocks - 1) / run_blocks);
    want = std::min(want, 8);
    RunChunks c;
    c.nper = std::max(64, ((N + want - 1) / want + 63) / 64 * 64);
    c.chunks = (N + c.nper - 1) / c.nper;
    return c;
}

// ---- the kernel form -----------------------------------------------------------------------------------------------
enum class CForm {
    sep_gemm,   // separable basis on a product grid: two stream-K GEMMs on the matrix cores (compressed_sep.hpp, cgemm.hpp)
    run,        // regular x axis, degree <= 2: recurrence along runs of a row (c_n2f_run / c_f2n_run)
    pixel,      // every pixel evaluates every spot's polynomial (c_n2f_partial / c_f2n)
};
struct CFormFacts {
    int elem = 4;                  // sizeof(R): the separable and the run form are fp32 only
    bool sep_valid = false;        // the separable tables match the uploaded grids, terms and coefficients
    bool run_valid = false;        // ... and so do the run records
    int opt_separable = 1;         // HGS_OPT_SEPARABLE
    int opt_sep_min = 96;          // HGS_OPT_SEPARABLE_MIN_SPOTS: smallest spot count the matrix-core form is used for
    int opt_run = 1;               // HGS_OPT_RUN_KERNELS
    int n_spots = 0, n_monomials = 0;
    int degree = 0;                // TermClass::degree
    int mono_tab = 1, c_mtab = 16; // Tuning::mono_tab; C_MTAB, the terms the monomial table of DEG 3 holds
};
// deg: the DEG of the instance.  run: 1 | 2; pixel: 1 | 2, 3 = monomial table, 0 = any degree; sep_gemm: unused (0)
struct CFormChoice { CForm form = CForm::pixel; int deg = 0; };
inline bool operator==(const CFormChoice& a, const CFormChoice& b) { return a.form == b.form && a.deg == b.deg; }

// Precedence: separable, then run, then per-pixel by degree.  Both directions of the transform take this one choice.
inline CFormChoice choose_form(const CFormFacts& f) {
    if (f.elem == 4 && f.sep_valid && f.opt_separable && f.n_spots >= f.opt_sep_min) return {CForm::sep_gemm, 0};
    if (f.elem == 4 && f.run_valid && f.opt_run && f.degree >= 0 && f.degree <= 2) return {CForm::run, f.degree <= 1 ? 1 : 2};
    if (f.degree <= 1) return {CForm::pixel, 1};
    if (f.degree == 2) return {CForm::pixel, 2};
    if (f.n_monomials <= f.c_mtab && f.mono_tab) return {CForm::pixel, 3};
    return {CForm::pixel, 0};
}

}  // namespace hgs
