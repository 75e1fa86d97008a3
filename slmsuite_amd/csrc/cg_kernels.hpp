// Element-wise kernels of optimize(method="CG") (hgs_cg_iterate): the closed-form phase gradient of the reference's default
// loss and the Adam update (_hologram.py:6-14 ComplexMSELoss, :1664-1759 optimize_cg; torch.optim.Adam defaults).
//
// One loop body is  n2f -> cg_seed_kernel -> f2n_complex -> cg_adam_kernel  (DESIGN.md "Gradient refinement"):
//   F = U n (n2f), A = |F|, s = ||A||, M = F.size, r = A / s - t,  L = (1 / M) sum r^2   (the engine reduces sum r^2)
//   G = (2 / (M s)) r F / A   (0 where A = 0)        -- the adjoint seed; the derivative through s pulls back to
//   g = U^H G over the SLM window (f2n_complex)         c Im(conj(n) n) = 0 and is dropped
//   dL/dphi = Im(conj(n) g) = amp (cos(phi + kappa) Im g - sin(phi + kappa) Re g)
// Both kernels are bandwidth bound.  A lane takes four pixels per step: a real array moves as one four-element vector (16
// bytes of float, 2 x 16 of double), a complex one as two vectors of two complex numbers; the up to three elements that
// an element count leaves over are taken one by one by a single lane.
#pragma once
#include "kernels.hpp"

namespace hgs {

template <typename R> struct CgVec {
    typedef R r4 __attribute__((ext_vector_type(4)));   // four reals
    typedef R c2 __attribute__((ext_vector_type(4)));   // two complex numbers (x0, y0, x1, y1)
};

constexpr int CG_WG = 256;

template <typename R> struct CgSeedArgs {
    Cx<R>* ff;           // [P] in: the farfield F of this body; out: the adjoint seed G (column-major like every P-sized array)
    const R* t;          // [P] target, same layout; finite (a NaN target is refused on the host side)
    const double* fsum;  // sum |F|^2 as n2f reduced it (device resident: no host round trip)
    double* partial;     // [gridDim.x] partial sums of r^2
    size_t P;
};

// r = A / s - t and G = coef * r * F / A for one pixel; returns r^2
template <typename R> __device__ __forceinline__ double cg_seed_one(R& x, R& y, R t, R inv_s, R coef) {
    const R a = Math<R>::sqrt(x * x + y * y);
    const R r = a * inv_s - t;
    const R q = a > (R)0 ? coef * r / a : (R)0;
    x *= q;
    y *= q;
    return (double)r * (double)r;
}

template <typename R> __global__ __launch_bounds__(CG_WG) void cg_seed_kernel(CgSeedArgs<R> a) {
    using C2 = typename CgVec<R>::c2;
    using R4 = typename CgVec<R>::r4;
    __shared__ double scratch[16];
    const double s2 = a.fsum[0];
    const double inv_sd = s2 > 0 ? 1.0 / ::sqrt(s2) : 0.0;
    const R inv_s = (R)inv_sd;
    const R coef = (R)(2.0 * inv_sd / (double)a.P);
    const size_t quads = a.P / 4, stride = (size_t)gridDim.x * blockDim.x;
    C2* ff2 = reinterpret_cast<C2*>(a.ff);
    const R4* t4 = reinterpret_cast<const R4*>(a.t);
    double acc = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < quads; i += stride) {
        const C2 fa = ff2[2 * i], fb = ff2[2 * i + 1];
        const R4 t = t4[i];
        R x0 = fa.x, y0 = fa.y, x1 = fa.z, y1 = fa.w, x2 = fb.x, y2 = fb.y, x3 = fb.z, y3 = fb.w;
        acc += cg_seed_one<R>(x0, y0, t.x, inv_s, coef);
        acc += cg_seed_one<R>(x1, y1, t.y, inv_s, coef);
        acc += cg_seed_one<R>(x2, y2, t.z, inv_s, coef);
        acc += cg_seed_one<R>(x3, y3, t.w, inv_s, coef);
        ff2[2 * i] = (C2){x0, y0, x1, y1};
        ff2[2 * i + 1] = (C2){x2, y2, x3, y3};
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (size_t k = 4 * quads; k < a.P; ++k) {         // at most three elements
            const Cx<R> f = a.ff[k];
            R x0 = f.x, y0 = f.y;
            acc += cg_seed_one<R>(x0, y0, a.t[k], inv_s, coef);
            a.ff[k] = mk<R>(x0, y0);
        }
    }
    const double s = block_sum(acc, scratch);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = s;
}

template <typename R> struct CgAdamArgs {
    const Cx<R>* g;   // [S] U^H G over the SLM window (nfbuf of f2n_complex)
    R* phase;         // [S] in/out, never wrapped
    const R* amp;     // [S] source amplitude, or nullptr: amp_scalar
    const R* kern;    // [S] propagation kernel, or nullptr
    R* m;             // [S] first moment
    R* v;             // [S] second moment
    R* grad;          // [S] dL/dphi of this body, or nullptr (keep-gradient flag off)
    R amp_scalar;
    R beta1, beta2, eps;
    R step_size;      // lr / (1 - beta1^t)               bias corrections come from the host: t is a host counter
    R inv_bc2_sqrt;   // 1 / sqrt(1 - beta2^t)
    size_t S;
};

template <typename R>
__device__ __forceinline__ void cg_adam_one(const CgAdamArgs<R>& a, R gx, R gy, R am, R kn, R& ph, R& m, R& v, R& grad) {
    R sn, cs;
    Math<R>::sincos(ph + kn, &sn, &cs);
    grad = am * (cs * gy - sn * gx);
    m = a.beta1 * m + ((R)1 - a.beta1) * grad;
    v = a.beta2 * v + ((R)1 - a.beta2) * grad * grad;
    ph -= a.step_size * m / (Math<R>::sqrt(v) * a.inv_bc2_sqrt + a.eps);
}

// one lane per four SLM pixels, plus one lane for the up to three left over (launch_cg_adam sizes the grid)
template <typename R> __global__ __launch_bounds__(CG_WG) void cg_adam_kernel(CgAdamArgs<R> a) {
    using C2 = typename CgVec<R>::c2;
    using R4 = typename CgVec<R>::r4;
    const size_t quads = a.S / 4;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < quads) {
        const C2 ga = reinterpret_cast<const C2*>(a.g)[2 * i], gb = reinterpret_cast<const C2*>(a.g)[2 * i + 1];
        const R4 ph = reinterpret_cast<const R4*>(a.phase)[i];
        const R4 m = reinterpret_cast<const R4*>(a.m)[i];
        const R4 v = reinterpret_cast<const R4*>(a.v)[i];
        R4 am = {a.amp_scalar, a.amp_scalar, a.amp_scalar, a.amp_scalar}, kn = {(R)0, (R)0, (R)0, (R)0};
        if (a.amp) am = reinterpret_cast<const R4*>(a.amp)[i];
        if (a.kern) kn = reinterpret_cast<const R4*>(a.kern)[i];
        R p0 = ph.x, p1 = ph.y, p2 = ph.z, p3 = ph.w, m0 = m.x, m1 = m.y, m2 = m.z, m3 = m.w;
        R v0 = v.x, v1 = v.y, v2 = v.z, v3 = v.w, g0, g1, g2, g3;
        cg_adam_one<R>(a, ga.x, ga.y, am.x, kn.x, p0, m0, v0, g0);
        cg_adam_one<R>(a, ga.z, ga.w, am.y, kn.y, p1, m1, v1, g1);
        cg_adam_one<R>(a, gb.x, gb.y, am.z, kn.z, p2, m2, v2, g2);
        cg_adam_one<R>(a, gb.z, gb.w, am.w, kn.w, p3, m3, v3, g3);
        reinterpret_cast<R4*>(a.phase)[i] = (R4){p0, p1, p2, p3};
        reinterpret_cast<R4*>(a.m)[i] = (R4){m0, m1, m2, m3};
        reinterpret_cast<R4*>(a.v)[i] = (R4){v0, v1, v2, v3};
        if (a.grad) reinterpret_cast<R4*>(a.grad)[i] = (R4){g0, g1, g2, g3};
    } else if (i == quads) {
        for (size_t k = 4 * quads; k < a.S; ++k) {         // at most three elements
            const Cx<R> g = a.g[k];
            R ph = a.phase[k], m = a.m[k], v = a.v[k], gr;
            cg_adam_one<R>(a, g.x, g.y, a.amp ? a.amp[k] : a.amp_scalar, a.kern ? a.kern[k] : (R)0, ph, m, v, gr);
            a.phase[k] = ph;
            a.m[k] = m;
            a.v[k] = v;
            if (a.grad) a.grad[k] = gr;
        }
    }
}

// launch front-ends (launch_cg_f32.hip / launch_cg_f64.hip); they note their instance in the dispatch record and return
// hipError_t as int.  blocks: grid of the seed pass (its partial sums: one per block)
template <typename R> int launch_cg_seed(int blocks, hipStream_t s, const CgSeedArgs<R>& a);
template <typename R> int launch_cg_adam(hipStream_t s, const CgAdamArgs<R>& a);

}  // namespace hgs
