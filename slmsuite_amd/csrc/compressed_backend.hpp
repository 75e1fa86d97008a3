// The CompressedSpotHologram transforms (hgs_config::kind == 1) as one owner: the uploaded grids, terms and coefficients,
// the tables of the three kernel forms and the launches.  What is decided on the host -- what the terms allow, whether the
// grids are a product grid and regular, the spot chunks, which form runs -- is compressed_plan.hpp; this file executes it.
// The engine keeps what concerns the engine (EngineState, the lazily allocated farfield buffers, profiling, the size checks
// of hgs_set_array) and hands the backend a CompressedView of itself with every call.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "hgs_error.hpp"
#include "launch.hpp"
#include "devbuf.hpp"
#include "compressed_plan.hpp"
#include "compressed_kernels.hpp"
#include "cgemm.hpp"
#include "compressed_sep.hpp"

namespace hgs {

HGS_BIND_F32(KCn2fRun, c_n2f_run);
HGS_BIND_F32(KCf2nRun, c_f2n_run);
HGS_BIND(KCn2fPix, c_n2f_partial);
HGS_BIND(KCf2nPix, c_f2n);
HGS_BIND_F32(KCgemm, cgemm_streamk);

// what the backend sees of its engine, filled per call (ff / aff exist once the first transform asked for them)
template <typename R> struct CompressedView {
    hipStream_t stream;
    int B;
    size_t S, P;
    Geo g;
    int n_cu;
    R* phase;
    const R *amp, *kern;   // null: the scalar amplitude / no propagation kernel
    double amp_scalar;
    Cx<R>* ff;
    R* aff;
    double* sums;          // [3][B]: fsum first
};

template <typename R> struct CompressedBackend {
    using View = CompressedView<R>;
    int N = 0, M = 0;                      // hgs_config::n_spots, n_monomials
    int mono_tab = 1;                      // Tuning::mono_tab
    int opt_separable = 1;                 // HGS_OPT_SEPARABLE
    int opt_sep_min = 96;                  // smallest spot count the matrix-core form is used for (tools/sep_crossover.py)
    int opt_sep_wg = 0;                    // HGS_OPT_SEP_WORKGROUPS: cap on the workgroups of each stream-K GEMM (0 = 2 * #CU)
    int opt_run = 1;                       // HGS_OPT_RUN_KERNELS
    // what was uploaded: device copies for the per-pixel kernels, host copies for the tables of the other two forms
    DevBuf<R> xg, yg, coeff;
    DevBuf<int> mono;
    std::vector<double> xs_host, ys_host;
    std::vector<int32_t> mono_host;
    std::vector<R> coeff_host;
    bool has_grid[2] = {false, false}, grid_sep[2] = {false, false}, has_mono = false, has_coeff = false;
    // per-pixel kernels
    DevBuf<Cx<R>> cpartial;
    DevBuf<double> cnorm;
    int c_nblocks = 0, c_degree = -1;
    // separable (matrix-core) form, fp32 only (compressed_sep.hpp)
    bool c_sep = false;
    DevBuf<double> sep_c;        // [2][SEP_MAXDEG+1][N] polynomial coefficients of fx_n, fy_n
    DevBuf<double> sep_g;        // xs[W] then ys[H]
    DevBuf<float2> sep_ex;       // [N][W]
    DevBuf<float2> sep_exT;      // [W][N]
    DevBuf<float2> sep_ey;       // [N][H]
    DevBuf<float2> sep_nfT;      // [B][W][H]
    DevBuf<float2> sep_b2;       // [B][N][H]
    DevBuf<float2> sep_c1;       // [B][tiles_n1 * 2 * split1][Np] partial y contractions of the n2f GEMM epilogue
    DevBuf<float2> sep_c2;       // [B][split2][H][W]
    DevBuf<double> sep_norm;     // [B][ceil(N/4)]
    // stream-K schedule of the two GEMMs (cgemm_streamk): sep_split1 / sep_split2 are the partial planes of C
    int sep_split1 = 1, sep_split2 = 1;
    unsigned sk_flag1 = 0, sk_flag2 = 0;   // DF_SK_CAP where the option holds G below min(2 * #CU, steps)
    int sk_G1 = 0, sk_G2 = 0, sk_kt1 = 0, sk_kt2 = 0, sk_tm1 = 0, sk_tn1 = 0, sk_tm2 = 0, sk_tn2 = 0;
    DevBuf<int> sk_tab;          // [first_wg 1][nseg 1][first_wg 2][nseg 2]
    int sep_Np = 0, sep_Hp = 0, sep_Wp = 0, sep_Wk = 0, sep_Nk = 0;   // padded leading dimensions / row counts
    // run kernels of the direct transforms (compressed_kernels.hpp: regular grid, degree <= 2, fp32)
    bool run_ok = false;
    DevBuf<CRunRec> run_rec;            // [N]
    DevBuf<double> run_ys;              // [H]
    DevBuf<Cx<float>> run_nf;           // [B][run_chunks][S]
    double run_x0 = 0, run_hx = 0;
    int run_rpr = 0, run_blocks = 0, run_chunks = 1, run_nper = 0, run_nf_chunks = 0;

    static int h2d(const View& v, void* dst, const void* src, size_t nbytes) {
        HIPCHK(hipMemcpyAsync(dst, src, nbytes, hipMemcpyHostToDevice, v.stream));
        HIPCHK(hipStreamSynchronize(v.stream));
        return 0;
    }
    static unsigned bflag(const View& v) { return v.B > 1 ? DF_BATCH : 0u; }

    int init(const View& v, int n_spots, int n_monomials, int mono_tab_) {
        N = n_spots; M = n_monomials; mono_tab = mono_tab_;
        c_nblocks = (int)((v.S + (size_t)C_WG * C_PT - 1) / ((size_t)C_WG * C_PT));
        run_rpr = (v.g.Sw + CR_RUN - 1) / CR_RUN;
        run_blocks = (v.g.Sh * run_rpr + 63) / 64;
        const size_t c_rows = std::max(6, M);      // the canonical six slots or the M terms
        HIPCHK(xg.alloc_zeroed(v.S, v.stream));
        HIPCHK(yg.alloc_zeroed(v.S, v.stream));
        HIPCHK(mono.alloc_zeroed((size_t)2 * M, v.stream));
        HIPCHK(coeff.alloc_zeroed(c_rows * v.P, v.stream));
        HIPCHK(cpartial.alloc_zeroed((size_t)v.B * std::max(c_nblocks, run_blocks) * v.P, v.stream));
        HIPCHK(cnorm.alloc_zeroed((size_t)v.B * ((v.P + C_RED_SPOTS - 1) / C_RED_SPOTS), v.stream));
        return 0;
    }

    // ---- uploads (hgs_set_array; sizes checked by the engine) ----
    bool uploaded() const { return has_grid[0] && has_grid[1] && has_mono && has_coeff; }
    bool product_grids() const { return grid_sep[0] && grid_sep[1]; }
    int set_grid(const View& v, int axis, const R* h) {
        if (int e_ = h2d(v, axis == 0 ? xg : yg, h, v.S * sizeof(R))) return e_;
        has_grid[axis] = true;
        grid_sep[axis] = product_grid_axis(h, v.g.Sh, v.g.Sw, axis, axis == 0 ? xs_host : ys_host);
        return refresh(v);
    }
    bool same_monomials(const int32_t* h) const { return has_mono && std::equal(mono_host.begin(), mono_host.end(), h); }
    int set_monomials(const View& v, const int32_t* h) {
        mono_host.assign(h, h + 2 * M);
        if (int e_ = h2d(v, mono, h, (size_t)2 * M * sizeof(int32_t))) return e_;
        has_mono = true;
        return pack_coeff(v);
    }
    int set_coeff(const View& v, const R* h) {
        coeff_host.assign(h, h + (size_t)M * N);
        has_coeff = true;
        return pack_coeff(v);
    }

    // repack the monomial weights for the degree-specialised kernels (canonical [1,x,y,x2,xy,y2])
    int pack_coeff(const View& v) {
        if (!has_mono || !has_coeff) return 0;
        const TermClass tc = classify_terms(mono_host.data(), M, SEP_MAXDEG);
        c_degree = tc.degree;
        if (tc.bad >= 0)
            return fail(HGS_ERR_ARG, "unrecognized term (%d, %d): the only pseudo-term is the vortex plate (-1, 0)",
                        mono_host[2 * tc.bad], mono_host[2 * tc.bad + 1]);
        if (c_degree <= 2) {
            std::vector<R> c6((size_t)6 * N, (R)0);
            for (int n = 0; n < N; ++n) canonical_coeffs(mono_host.data(), M, coeff_host.data(), N, n, &c6[n], (size_t)N);
            if (int e_ = h2d(v, coeff, c6.data(), c6.size() * sizeof(R))) return e_;
        } else {
            if (int e_ = h2d(v, coeff, coeff_host.data(), (size_t)M * N * sizeof(R))) return e_;
        }
        return refresh(v);
    }
    // called whenever the grids, the term set or the coefficients changed: the tables of the separable and the run form
    int refresh(const View& v) {
        if (int e = sep_refresh(v)) return e;
        return run_refresh(v);
    }

    // ---- which form transforms (both directions) ----
    CFormChoice form() const {
        CFormFacts f;
        f.elem = (int)sizeof(R); f.sep_valid = c_sep; f.run_valid = run_ok;
        f.opt_separable = opt_separable; f.opt_sep_min = opt_sep_min; f.opt_run = opt_run;
        f.n_spots = N; f.n_monomials = M; f.degree = c_degree; f.mono_tab = mono_tab; f.c_mtab = C_MTAB;
        return choose_form(f);
    }
    // instance <RR, deg> of a family whose only template argument after the element type is the degree, among those listed
    template <typename Fam, typename RR, int... DEG, typename A> static int launch_deg(const View& v, int deg, dim3 grid, dim3 block, const A& a) {
        int e = (int)hipErrorInvalidValue;
        ((deg == DEG ? (void)(e = launch_instance<Fam, RR, DEG>(grid, block, 0, v.stream, bflag(v), a)) : (void)0), ...);
        return e;
    }
    CArgs<R> cargs(const View& v) const {
        CArgs<R> a{};
        a.S = (int)v.S; a.N = N; a.M = M; a.batch = v.B; a.xg = xg; a.yg = yg; a.mono = mono;
        a.coeff = coeff; a.phase = v.phase; a.amp = v.amp; a.kern = v.kern;
        a.amp_scalar = (R)v.amp_scalar; a.ff = v.ff; a.amp_ff = v.aff; a.partial = cpartial; a.nblocks = c_nblocks;
        a.fsum = v.sums; a.degree = c_degree;
        return a;
    }
    int n2f(const View& v) {
        const CFormChoice c = form();
        if (c.form == CForm::sep_gemm) return sep_n2f(v);
        CArgs<R> a = cargs(v);
        if (c.form == CForm::run) { if (int e = run_n2f(v, a, c.deg)) return e; }
        else LCHK((launch_deg<KCn2fPix, R, 1, 2, 3, 0>(v, c.deg, dim3(c_nblocks, v.B), dim3(C_WG), a)));
        const int nred = (int)((v.P + C_RED_SPOTS - 1) / C_RED_SPOTS);
        hipLaunchKernelGGL(c_n2f_reduce<R>, dim3(nred, v.B), dim3(C_RED_SPOTS * C_RED_SLICES), 0, v.stream, a, cnorm.get());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(c_n2f_finish<R>, dim3(v.B), dim3(1024), 0, v.stream, a, (const double*)cnorm, nred);
        HIPCHK(hipGetLastError());
        return 0;
    }
    // nf_out: null extracts the phase; else the complex nearfield goes there and the phase stays (f2n_complex)
    int f2n(const View& v, Cx<R>* nf_out) {
        const CFormChoice c = form();
        if (c.form == CForm::sep_gemm) return sep_f2n(v, nf_out);
        CArgs<R> a = cargs(v);
        a.nf_out = nf_out;
        if (c.form == CForm::run) return run_f2n(v, a, c.deg);
        LCHK((launch_deg<KCf2nPix, R, 1, 2, 3, 0>(v, c.deg, dim3(c_nblocks, v.B), dim3(C_WG), a)));
        return 0;
    }

    // ---- run kernels ----
    // x must be a regular grid over the columns (checked against the uploaded values), y a function of the row, the
    // polynomial of degree <= 2.  Per spot: canonical coefficients in double and the constant factor of the recurrence
    // (degree 2: C_n = exp(i 2 c3 h^2); degree 1: D_n = exp(i c1 h)).
    int run_refresh(const View& v) {
        run_ok = false;
        if constexpr (sizeof(R) != 4) return 0;
        if (!(uploaded() && product_grids())) return 0;
        if (c_degree < 0 || c_degree > 2) return 0;
        const int H = v.g.Sh, W = v.g.Sw;
        const RegularAxis ax = regular_axis(xs_host.data(), W);
        if (!ax.ok) return 0;
        std::vector<CRunRec> rec((size_t)N);
        for (int n = 0; n < N; ++n) {
            CRunRec& r = rec[n];
            for (double& c : r.c) c = 0;
            canonical_coeffs(mono_host.data(), M, coeff_host.data(), N, n, r.c);
            const double ang = c_degree == 2 ? 2.0 * r.c[3] * ax.hx * ax.hx : r.c[1] * ax.hx;
            r.cr = (float)std::cos(ang);
            r.ci = (float)std::sin(ang);
            r.pad0 = r.pad1 = 0;
        }
        HIPCHK(run_rec.ensure((size_t)N));
        HIPCHK(run_ys.ensure((size_t)H));
        if (int e_ = h2d(v, run_rec, rec.data(), rec.size() * sizeof(CRunRec))) return e_;
        if (int e_ = h2d(v, run_ys, ys_host.data(), (size_t)H * sizeof(double))) return e_;
        run_x0 = ax.x0;
        run_hx = ax.hx;
        const RunChunks ch = run_chunking(N, v.n_cu, run_blocks);
        run_nper = ch.nper;
        run_chunks = ch.chunks;
        run_ok = true;
        return 0;
    }
    CRunArgs run_args(const View& v, const CArgs<R>& a) {
        CRunArgs ra{};
        if constexpr (sizeof(R) == 4) ra.a = a;
        ra.a.nblocks = run_blocks;
        ra.rec = run_rec; ra.ys = run_ys; ra.x0 = run_x0; ra.hx = run_hx; ra.H = v.g.Sh; ra.W = v.g.Sw; ra.rpr = run_rpr;
        ra.n_per = run_nper; ra.nf_part = run_nf;
        return ra;
    }
    int run_n2f(const View& v, CArgs<R>& a, int deg) {
        CRunArgs ra = run_args(v, a);
        a.nblocks = run_blocks;                       // what c_n2f_reduce sums over
        LCHK((launch_deg<KCn2fRun, float, 1, 2>(v, deg, dim3(run_blocks, v.B, run_chunks), dim3(64), ra)));
        return 0;
    }
    int run_f2n(const View& v, const CArgs<R>& a, int deg) {
        if (!run_nf || run_nf_chunks < run_chunks) {
            HIPCHK(run_nf.release(v.stream));
            HIPCHK(run_nf.alloc((size_t)v.B * run_chunks * v.S));
            run_nf_chunks = run_chunks;
        }
        CRunArgs ra = run_args(v, a);
        LCHK((launch_deg<KCf2nRun, float, 1, 2>(v, deg, dim3(run_blocks, v.B, run_chunks), dim3(64), ra)));
        hipLaunchKernelGGL(c_f2n_run_finish, dim3((unsigned)((v.S + 255) / 256), v.B), dim3(256), 0, v.stream, ra.a,
                           (const Cx<float>*)run_nf, run_chunks);
        HIPCHK(hipGetLastError());
        return 0;
    }

    // ---- separable / matrix-core form (compressed_sep.hpp) ----
    // stream-K: the (tile, k tile) steps of each GEMM in G = min(HGS_OPT_SEP_WORKGROUPS or 2 * #CU, 2 * #CU, steps) equal shares
    // (at most one workgroup per step: every workgroup owns work, the owners of a tile are consecutive); per tile the first
    // workgroup and the number of partial planes it is spread over (consumers add exactly those), and the two buffers of
    // partial results, whose size follows the planes.  Called when the tables are first made and when the option changes.
    int sk_retable(const View& v) {
        const int H = v.g.Sh, W = v.g.Sw;
        const int t1 = sk_tm1 * sk_tn1, t2 = sk_tm2 * sk_tn2;
        const long long full = 2 * v.n_cu, want = opt_sep_wg > 0 ? std::min<long long>(opt_sep_wg, full) : full;
        const long long steps1 = (long long)t1 * sk_kt1, steps2 = (long long)t2 * sk_kt2;
        sk_G1 = (int)std::min(want, steps1);
        sk_G2 = (int)std::min(want, steps2);
        sk_flag1 = sk_G1 < std::min(full, steps1) ? DF_SK_CAP : 0u;
        sk_flag2 = sk_G2 < std::min(full, steps2) ? DF_SK_CAP : 0u;
        std::vector<int> tab((size_t)2 * (t1 + t2));
        sep_split1 = sk_fill(t1, sk_kt1, sk_G1, tab.data(), tab.data() + t1);
        sep_split2 = sk_fill(t2, sk_kt2, sk_G2, tab.data() + 2 * t1, tab.data() + 2 * t1 + t2);
        // (launches on the stream may still read what a change of the option replaces)
        HIPCHK(sk_tab.release(v.stream));
        HIPCHK(sep_c1.release(v.stream));
        HIPCHK(sep_c2.release(v.stream));
        HIPCHK(sk_tab.alloc(tab.size()));
        if (int e_ = h2d(v, sk_tab, tab.data(), tab.size() * sizeof(int))) return e_;
        HIPCHK(sep_c1.alloc(sk_part_elems(v.B, sk_tn1, sep_split1, (size_t)sep_Np)));
        HIPCHK(sep_c2.alloc(sk_c_elems(v.B, sep_split2, (size_t)H, (size_t)W)));
        return 0;
    }
    // HGS_OPT_SEP_WORKGROUPS (value >= 0): where the tables exist already, rebuild them and the plane buffers they size
    int set_sep_workgroups(const View& v, int value) {
        if (value == opt_sep_wg) return 0;
        opt_sep_wg = value;
        if (sep_c)
            if (int e_ = sk_retable(v)) { c_sep = false; return e_; }
        return 0;
    }
    int sep_refresh(const View& v) {
        c_sep = false;
        if (sizeof(R) != 4) return 0;
        if (!(uploaded() && product_grids())) return 0;
        const int H = v.g.Sh, W = v.g.Sw, B = v.B;
        const TermClass tc = classify_terms(mono_host.data(), M, SEP_MAXDEG);
        if (!tc.separable) return 0;
        std::vector<double> c((size_t)2 * (SEP_MAXDEG + 1) * N, 0.0);
        for (int m = 0; m < M; ++m) {
            const int px = mono_host[2 * m], py = mono_host[2 * m + 1];
            double* dst = (py == 0) ? &c[(size_t)px * N] : &c[((size_t)(SEP_MAXDEG + 1) + py) * N];
            for (int n = 0; n < N; ++n) dst[n] += (double)coeff_host[(size_t)m * N + n];
        }
        if (!sep_c) {
            // operands of the matrix-core GEMM are padded to whole tiles (zero filled once, never rewritten)
            auto up = [](int x, int q) { return (x + q - 1) / q * q; };
            sk_tm1 = (N + CG_BM - 1) / CG_BM; sk_tn1 = (H + CG_BN - 1) / CG_BN; sk_kt1 = (W + CG_BK - 1) / CG_BK;
            sk_tm2 = (H + CG_BM - 1) / CG_BM; sk_tn2 = (W + CG_BN - 1) / CG_BN; sk_kt2 = (N + CG_BK - 1) / CG_BK;
            sep_Np = up(N, CG_BM); sep_Hp = up(H, CG_BN); sep_Wp = up(W, CG_BN);
            if (int e_ = sk_retable(v)) return e_;
            sep_Wk = sk_kt1 * CG_BK;
            sep_Nk = sk_kt2 * CG_BK;
            HIPCHK(sep_c.alloc(c.size()));
            HIPCHK(sep_g.alloc((size_t)(W + H)));
            HIPCHK(sep_ex.alloc_zeroed((size_t)sep_Nk * sep_Wp, v.stream));       // [Nk][Wp]  (B of the f2n GEMM)
            HIPCHK(sep_exT.alloc_zeroed((size_t)sep_Wk * sep_Np, v.stream));      // [Wk][Np]  (A of the n2f GEMM)
            HIPCHK(sep_ey.alloc_zeroed((size_t)N * H, v.stream));
            HIPCHK(sep_nfT.alloc_zeroed((size_t)B * sep_Wk * sep_Hp, v.stream));  // [B][Wk][Hp]
            HIPCHK(sep_b2.alloc_zeroed((size_t)B * sep_Nk * sep_Hp, v.stream));   // [B][Nk][Hp]
            HIPCHK(sep_norm.alloc((size_t)B * ((N + 255) / 256)));
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(cgemm_streamk<0>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)CG_LDS_BYTES));
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(cgemm_streamk<1>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)CG_LDS_BYTES));
        } else if (!sk_tab || !sep_c1 || !sep_c2) {      // (a change of HGS_OPT_SEP_WORKGROUPS that the device could not follow)
            if (int e_ = sk_retable(v)) return e_;
        }
        HIPCHK(hipMemcpyAsync(sep_c, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice, v.stream));
        HIPCHK(hipMemcpyAsync(sep_g, xs_host.data(), (size_t)W * sizeof(double), hipMemcpyHostToDevice, v.stream));
        HIPCHK(hipMemcpyAsync(sep_g + W, ys_host.data(), (size_t)H * sizeof(double), hipMemcpyHostToDevice, v.stream));
        hipLaunchKernelGGL(sep_build_table, dim3((W + 255) / 256, N), dim3(256), 0, v.stream, (const double*)sep_c, tc.dx, N,
                           (const double*)sep_g, W, sep_ex.get(), sep_Wp, (size_t)sep_Nk * sep_Wp, sep_exT.get(), sep_Np, (size_t)sep_Wk * sep_Np);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(sep_build_table, dim3((H + 255) / 256, N), dim3(256), 0, v.stream,
                           (const double*)(sep_c + (size_t)(SEP_MAXDEG + 1) * N), tc.dy, N, (const double*)(sep_g + W), H, sep_ey.get(),
                           H, (size_t)0, (float2*)nullptr, 0, (size_t)0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(v.stream));   // c / xs_host are host temporaries
        c_sep = true;
        return 0;
    }
    // operands planar: real array at A / Bm, imaginary one planeA / planeB floats on.  E != nullptr: the epilogue contracts
    // the result with E over its columns into `part` instead of storing it (n2f)
    int launch_cgemm(const View& v, const float* A, size_t planeA, const float* Bm, size_t planeB, float2* C, int M_, int N_, int KT, int lda,
                     int ldb, int tiles_m, int tiles_n, int planes, const int* first_wg, int G, size_t strideA, size_t strideB,
                     unsigned cap_flag, const float2* E = nullptr, int ldE = 0, float2* part = nullptr, int ldP = 0) {
        CgemmSkArgs a{A, A + planeA, Bm, Bm + planeB, C, M_, N_, KT, lda, ldb, tiles_m, tiles_n, planes, first_wg, strideA, strideB,
                      E, ldE, part, ldP};
        // (sep_refresh allowed both instances CG_LDS_BYTES of LDS when it made the tables)
        const dim3 grid(G, v.B), block(256);
        if (E) LCHK((launch_noted<KCgemm, float, 1>(grid, block, CG_LDS_BYTES, v.stream, bflag(v) | cap_flag, a)));
        else LCHK((launch_noted<KCgemm, float, 0>(grid, block, CG_LDS_BYTES, v.stream, bflag(v) | cap_flag, a)));
        return 0;
    }
    // n2f: T = Ex^T-table x nf^T on the matrix cores, contracted with Ey over y in the GEMM's epilogue
    int sep_n2f(const View& v) {
        const int H = v.g.Sh, W = v.g.Sw, B = v.B;
        hipLaunchKernelGGL(sep_build_nft<R>, dim3((W + 31) / 32, (H + 31) / 32, B), dim3(32, 8), 0, v.stream, (const R*)v.phase,
                           v.amp, v.kern, (R)v.amp_scalar, H, W, reinterpret_cast<float*>(sep_nfT.get()), sep_Hp, (size_t)sep_Wk * sep_Hp);
        HIPCHK(hipGetLastError());
        const int t1 = sk_tm1 * sk_tn1;
        if (int e = launch_cgemm(v, reinterpret_cast<const float*>(sep_exT.get()), (size_t)sep_Wk * sep_Np,
                                 reinterpret_cast<const float*>(sep_nfT.get()), (size_t)sep_Wk * sep_Hp, nullptr, N, H, sk_kt1, sep_Np, sep_Hp,
                                 sk_tm1, sk_tn1, sep_split1, sk_tab, sk_G1, 0, (size_t)2 * sep_Wk * sep_Hp, sk_flag1,
                                 (const float2*)sep_ey, H, sep_c1, sep_Np)) return e;
        const int nred = (N + 255) / 256;
        hipLaunchKernelGGL(sep_n2f_sum<R>, dim3(nred, B), dim3(256), 0, v.stream, (const float2*)sep_c1, sep_Np, sep_split1,
                           (const int*)(sk_tab + t1), sk_tm1, sk_tn1, N, 1.0 / std::sqrt((double)v.S), v.ff, sep_norm.get());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(c_n2f_finish<R>, dim3(B), dim3(1024), 0, v.stream, cargs(v), (const double*)sep_norm, nred);
        HIPCHK(hipGetLastError());
        return 0;
    }
    // f2n: conj(nf) = (conj(ff) Ey)^T x Ex on the matrix cores, then phase extraction (or the complex field)
    int sep_f2n(const View& v, Cx<R>* nf_out) {
        const int H = v.g.Sh, W = v.g.Sw, B = v.B;
        hipLaunchKernelGGL(sep_build_b2<R>, dim3((H + 255) / 256, N, B), dim3(256), 0, v.stream, (const Cx<R>*)v.ff,
                           (const float2*)sep_ey, N, H, reinterpret_cast<float*>(sep_b2.get()), sep_Hp, (size_t)sep_Nk * sep_Hp);
        HIPCHK(hipGetLastError());
        const int t1 = sk_tm1 * sk_tn1, t2 = sk_tm2 * sk_tn2;
        if (int e = launch_cgemm(v, reinterpret_cast<const float*>(sep_b2.get()), (size_t)sep_Nk * sep_Hp,
                                 reinterpret_cast<const float*>(sep_ex.get()), (size_t)sep_Nk * sep_Wp, sep_c2, H, W, sk_kt2, sep_Hp, sep_Wp,
                                 sk_tm2, sk_tn2, sep_split2, sk_tab + 2 * t1, sk_G2, (size_t)2 * sep_Nk * sep_Hp, 0, sk_flag2)) return e;
        hipLaunchKernelGGL(sep_f2n_finish<R>, dim3((unsigned)((v.S + 255) / 256), B), dim3(256), 0, v.stream, (const float2*)sep_c2,
                           sep_split2, (const int*)(sk_tab + 2 * t1 + t2), sk_tm2, W, v.S, v.kern, v.phase, nf_out);
        HIPCHK(hipGetLastError());
        return 0;
    }
};

}  // namespace hgs
