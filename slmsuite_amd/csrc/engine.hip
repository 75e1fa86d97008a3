// Host side of the hologram engine: device state, kernel sequencing, the C ABI of include/hgs.h.
// One engine = one HIP stream + all device buffers of a batch of equally-shaped holograms.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hgs.h"
#include "hgs_error.hpp"
#include "launch.hpp"
#include "column_plan.hpp"
#include "devbuf.hpp"
#include "engine_state.hpp"
#include "compressed_backend.hpp"
#include "bluestein.hpp"
#include "cg_kernels.hpp"
#include "vortex_kernels.hpp"
#include "display_kernels.hpp"
#include "poly_kernels.hpp"
#include "pattern_kernels.hpp"
#include <complex>
#include <dlfcn.h>

namespace hgs {

// roctx ranges around the operators (HGS_OPT_ROCTX): resolved at run time so that the library keeps its single
// link dependency (libamdhip64); rocprofv3 --marker-trace shows them.  librocprofiler-sdk-roctx first (rocprofv3),
// then the legacy libroctx64.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    bool tried = false;
    bool load() {
        if (tried) return push != nullptr;
        tried = true;
        for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            if (void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {
                push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
                pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                if (push && pop) return true;
                push = nullptr;
                pop = nullptr;
            }
        }
        return false;
    }
};
static Roctx g_roctx;
struct RoctxRange {
    bool on;
    RoctxRange(bool enabled, const char* name) : on(enabled && g_roctx.push != nullptr) { if (on) g_roctx.push(name); }
    ~RoctxRange() { if (on) g_roctx.pop(); }
};

thread_local DispatchLog* g_dispatch = nullptr;
// one line per (kernel instance, run-time flags): "family<P0=v0,...> flag ...\tcount\n".  The argument values come from
// __PRETTY_FUNCTION__ of dispatch_site<Fam, R, V...>: "... [Fam = hgs::KTile, R = float, V = <4096, 1, 6, false, false, 1, 0>]"
std::string DispatchLog::text() const {
    static const char* flag_names[] = {"list", "load_mask", "store_mask", "xmap", "batch", "stats", "nf_out", "col_flags", "sk_cap", "zero_inv", "zero_fwd", "quad", "prezero", "zero_mask", "tile_list"};
    std::string out;
    for (const Ent& e : v) {
        std::vector<std::string> vals;
        const std::string p = e.site->pretty;
        size_t r0 = p.find("R = ");
        if (r0 != std::string::npos) {
            r0 += 4;
            const size_t r1 = p.find_first_of(",]", r0);
            vals.push_back(p.substr(r0, r1 - r0));
        }
        size_t v0 = p.find("V = <");
        if (v0 != std::string::npos) {
            v0 += 5;
            const size_t v1 = p.find('>', v0);
            std::string list = p.substr(v0, v1 - v0);
            size_t a = 0;
            while (a <= list.size()) {
                size_t b = list.find(", ", a);
                if (b == std::string::npos) b = list.size();
                if (b > a) vals.push_back(list.substr(a, b - a));
                a = b + 2;
            }
        }
        out += e.site->family;
        out += '<';
        const std::string names = e.site->params;
        size_t a = 0;
        for (size_t i = 0; i < vals.size(); ++i) {
            size_t b = names.find(',', a);
            if (b == std::string::npos) b = names.size();
            if (i) out += ',';
            out += (a < names.size() ? names.substr(a, b - a) : std::string("?")) + "=" + vals[i];
            a = b + 1;
        }
        out += '>';
        for (unsigned bit = 0; bit < sizeof flag_names / sizeof flag_names[0]; ++bit)
            if (e.flags & (1u << bit)) { out += ' '; out += flag_names[bit]; }
        out += '\t' + std::to_string(e.count) + '\n';
    }
    return out;
}

static bool is_pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }
static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

// A compacted list of columns: those whose flag byte (scan_active_cols, dilate_active_cols) has one of the bits of `bit`
// set.  Whether a list still matches the scan it was built from is the EngineState's business, not the list's.
struct ColList {
    DevBuf<int> list;               // [B][Pw] compacted
    DevBuf<int> n_dev;              // [B] how many of them
    DevBuf<unsigned short> mask;    // [B][Pw/16] row-kernel view of the same columns
    int n_max = 0, n_min = 0;       // over the holograms of the batch
    int build(const unsigned char* flags, int bit, int B, int Pw, hipStream_t stream) {
        HIPCHK(list.ensure((size_t)B * Pw)); HIPCHK(n_dev.ensure((size_t)B)); HIPCHK(mask.ensure((size_t)B * (Pw / 16)));
        hipLaunchKernelGGL(compact_active_cols, dim3(B), dim3(256), 0, stream, flags, Pw, list.get(), n_dev.get(), mask.get(), bit);
        HIPCHK(hipGetLastError());
        std::vector<int> h(B);
        HIPCHK(hipMemcpyAsync(h.data(), n_dev, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        n_max = *std::max_element(h.begin(), h.end());
        n_min = *std::min_element(h.begin(), h.end());
        return 0;
    }
};

// ---- polynomial phase masks (include/hgs.h, poly_kernels.hpp) ------------------------------------------------------------
// the launches of hgs_poly_eval, which has no engine to keep them
static thread_local DispatchLog g_poly_log;

static int poly_check(const hgs_poly_params* p) {
    if (!p) return fail(HGS_ERR_ARG, "null parameters");
    if (p->h < 1 || p->w < 1 || p->n < 1) return fail(HGS_ERR_ARG, "polynomial mask: h, w and n must be positive (got %d, %d, %d)", p->h, p->w, p->n);
    if (p->degree < 0) return fail(HGS_ERR_ARG, "polynomial mask: negative degree %d", p->degree);
    if (p->degree > HGS_POLY_MAX_DEGREE)
        return fail(HGS_ERR_UNSUPPORTED, "polynomial mask: degree %d is beyond the limit of %d", p->degree, HGS_POLY_MAX_DEGREE);
    if (p->grid_bytes != 4 && p->grid_bytes != 8) return fail(HGS_ERR_ARG, "polynomial mask: grid_bytes must be 4 or 8 (got %d)", p->grid_bytes);
    if (p->mask_mode < HGS_POLY_MASK_NONE || p->mask_mode > HGS_POLY_MASK_NAN) return fail(HGS_ERR_ARG, "polynomial mask: unknown mask mode %d", p->mask_mode);
    if (!std::isfinite(p->x_scale) || !std::isfinite(p->y_scale)) return fail(HGS_ERR_ARG, "polynomial mask: the scales must be finite");
    if (!p->table) return fail(HGS_ERR_ARG, "polynomial mask: null coefficient table");
    const bool axes = p->x_axis && p->y_axis, grids = p->x_grid && p->y_grid;
    if (!axes && !grids) return fail(HGS_ERR_ARG, "polynomial mask: needs both axis vectors or both grid arrays");
    return 0;
}

// the coordinates of a mask on the device: the two axis vectors of a product grid (given, or found in full arrays), else the
// two full arrays; complete on return
template <typename G> struct GridDevice {
    DevBuf<G> x, y;
    bool product = false;
    int upload(const void* x_axis, const void* y_axis, const void* x_grid, const void* y_grid, int h, int w, hipStream_t stream) {
        const size_t S = (size_t)h * w;
        std::vector<G> ax, ay;          // axes found in full arrays; alive until the copies below have landed
        const G* hx = static_cast<const G*>(x_axis);
        const G* hy = static_cast<const G*>(y_axis);
        product = hx && hy;
        if (!product) {
            std::vector<double> dx, dy;
            product = product_grid_axis(static_cast<const G*>(x_grid), h, w, 0, dx) &&
                      product_grid_axis(static_cast<const G*>(y_grid), h, w, 1, dy);
            if (product) {
                ax.assign(dx.begin(), dx.end()); ay.assign(dy.begin(), dy.end());     // (exact: they were widened from G)
                hx = ax.data(); hy = ay.data();
            } else {
                hx = static_cast<const G*>(x_grid); hy = static_cast<const G*>(y_grid);
            }
        }
        const size_t nx = product ? (size_t)w : S, ny = product ? (size_t)h : S;
        HIPCHK(x.alloc(nx)); HIPCHK(y.alloc(ny));
        HIPCHK(hipMemcpyAsync(x, hx, nx * sizeof(G), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(y, hy, ny * sizeof(G), hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
};

// what a launch reads, on the device: the triangle, the vortex weights, the coordinates
template <typename G> struct PolyDevice {
    DevBuf<double> table, vortex;
    GridDevice<G> grid;
    int upload(const hgs_poly_params* p, hipStream_t stream) {
        const size_t T = (size_t)poly_table_len(p->degree);
        HIPCHK(table.alloc((size_t)p->n * T));
        HIPCHK(hipMemcpyAsync(table, p->table, (size_t)p->n * T * sizeof(double), hipMemcpyHostToDevice, stream));
        bool any_vortex = false;
        for (int k = 0; p->vortex && k < p->n; ++k) any_vortex = any_vortex || p->vortex[k] > 0;
        if (any_vortex) {
            HIPCHK(vortex.alloc((size_t)p->n));
            HIPCHK(hipMemcpyAsync(vortex, p->vortex, (size_t)p->n * sizeof(double), hipMemcpyHostToDevice, stream));
        }
        return grid.upload(p->x_axis, p->y_axis, p->x_grid, p->y_grid, p->h, p->w, stream);
    }
    int launch(const hgs_poly_params* p, void* dev_out, int out_bytes, hipStream_t stream) const {
        PolyArgs<G, void> a{};
        a.out = dev_out; a.x = grid.x; a.y = grid.y; a.table = table; a.vortex = vortex;
        a.S = (size_t)p->h * p->w; a.W = p->w; a.deg = p->degree; a.mask_mode = p->mask_mode;
        // the scales meet the grid in ITS type (a Python float times a float32 array is a float32 product)
        a.x_scale = (double)(G)p->x_scale; a.y_scale = (double)(G)p->y_scale;
        LCHK(launch_poly<G>(p->n, grid.product, out_bytes, stream, a));
        return 0;
    }
};

// checked parameters -> dev_out ([n][h][w] of out_bytes-sized reals, aligned to out_bytes); wrap(launch) runs the launch
// (the engine times it there); complete on return
template <typename G, typename W> static int poly_run_as(const hgs_poly_params* p, void* dev_out, int out_bytes, hipStream_t stream, W&& wrap) {
    PolyDevice<G> d;
    if (int e = d.upload(p, stream)) return e;
    if (int e = wrap([&]() -> int { return d.launch(p, dev_out, out_bytes, stream); })) return e;
    HIPCHK(hipStreamSynchronize(stream));        // (the buffers of d go with this scope)
    return 0;
}
template <typename W> static int poly_run(const hgs_poly_params* p, void* dev_out, int out_bytes, hipStream_t stream, W&& wrap) {
    return p->grid_bytes == 4 ? poly_run_as<float>(p, dev_out, out_bytes, stream, wrap)
                              : poly_run_as<double>(p, dev_out, out_bytes, stream, wrap);
}

// ---- grating, axicon and Gaussian-mode masks (include/hgs.h, pattern_kernels.hpp) ----------------------------------------------
static int pattern_check(const hgs_pattern_params* p) {
    if (!p) return fail(HGS_ERR_ARG, "null parameters");
    if (p->h < 1 || p->w < 1) return fail(HGS_ERR_ARG, "pattern mask: h and w must be positive (got %d, %d)", p->h, p->w);
    if (p->grid_bytes != 4 && p->grid_bytes != 8) return fail(HGS_ERR_ARG, "pattern mask: grid_bytes must be 4 or 8 (got %d)", p->grid_bytes);
    if (p->mode < 0 || p->mode >= PAT_MODES) return fail(HGS_ERR_ARG, "pattern mask: unknown mode %d", p->mode);
    if (p->quad && p->mode > HGS_PATTERN_BINARY) return fail(HGS_ERR_ARG, "pattern mask: only the grating modes fill quadrants (mode %d)", p->mode);
    if (!p->quad && p->mode == HGS_PATTERN_BLAZE) return fail(HGS_ERR_ARG, "pattern mask: a plain blaze is a polynomial mask (hgs_poly_eval)");
    for (int i = 0; i < (p->quad ? 8 : 2); ++i)
        if (!std::isfinite(p->vec[i])) return fail(HGS_ERR_ARG, "pattern mask: the vectors must be finite");
    if (!std::isfinite(p->shift) || !std::isfinite(p->a) || !std::isfinite(p->b) || std::isnan(p->duty))
        return fail(HGS_ERR_ARG, "pattern mask: shift, a, b and duty must be finite");
    if (p->mode == HGS_PATTERN_LG || p->mode == HGS_PATTERN_HG) {
        const int lo = p->mode == HGS_PATTERN_LG ? p->p : std::min(p->n, p->m), hi = p->mode == HGS_PATTERN_LG ? p->p : std::max(p->n, p->m);
        if (lo < 0) return fail(HGS_ERR_ARG, "pattern mask: negative order %d", lo);
        if (hi > HGS_PATTERN_MAX_ORDER) return fail(HGS_ERR_UNSUPPORTED, "pattern mask: order %d is beyond the limit of %d", hi, HGS_PATTERN_MAX_ORDER);
        const bool scaled = p->mode == HGS_PATTERN_HG || p->p != 0;          // (a vortex alone has no radius)
        if (scaled && (!std::isfinite(p->radius) || p->radius == 0)) return fail(HGS_ERR_ARG, "pattern mask: the source radius must be finite and not 0");
    }
    const bool axes = p->x_axis && p->y_axis, grids = p->x_grid && p->y_grid;
    if (!axes && !grids) return fail(HGS_ERR_ARG, "pattern mask: needs both axis vectors or both grid arrays");
    return 0;
}

// NumPy's mod of a double by b > 0
static double numpy_mod(double a, double b) {
    double m = std::fmod(a, b);
    if (m != 0) { if (m < 0) m += b; } else m = 0;
    return m;
}

// the kernel's parameters from the call's: 2 pi folded into the vectors, binary's pixel-period and zero-vector rules per window
template <typename G> static void pattern_args(const hgs_pattern_params* p, PatArgs<G, void>& a) {
    const double two_pi = 2 * M_PI;
    a.S = (size_t)p->h * p->w; a.W = p->w; a.H = p->h;
    a.quad = p->quad != 0; a.round_g = p->round_grid != 0; a.dec_double = p->decision_double != 0; a.pixel_mask = 0;
    a.l = p->l; a.p = p->p; a.n = p->n; a.m = p->m;
    const double duty = std::min(1.0, std::max(0.0, p->duty));
    a.shift = p->shift; a.off = two_pi * (1 - duty);
    a.half = (p->a - p->b) / 2; a.base = p->b;
    a.kx = p->vec[0]; a.ky = p->vec[1];
    a.s = p->mode == HGS_PATTERN_LG && p->p != 0 ? 16.0 / p->radius / p->radius : p->mode == HGS_PATTERN_HG ? 4.0 / p->radius : 0.0;
    for (int i = 0; i < 4; ++i) {
        const int from = a.quad ? i : 0;
        double vx = p->vec[2 * from], vy = p->vec[2 * from + 1];
        PatSet& g = a.set[i];
        g.a = p->a; g.b = p->b;
        if (p->mode == HGS_PATTERN_BINARY) {
            if (std::fabs(vx) > 1 || std::fabs(vy) > 1) {               // a period in pixels
                a.pixel_mask |= 1 << i;
                vx = vx == 0 ? 0.0 : 1.0 / vx;
                vy = vy == 0 ? 0.0 : 1.0 / vy;
            }
            if (vx == 0 && vy == 0) {                                   // no grating: one level everywhere
                const bool high = p->shift != 0 && numpy_mod(p->shift, two_pi) > two_pi * duty;
                g.a = g.b = high ? p->a : p->b;
            }
        }
        g.kx = two_pi * vx; g.ky = two_pi * vy;
    }
}

// checked parameters -> dev_out ([h][w] of out_bytes-sized reals, aligned to out_bytes); wrap as in poly_run; complete on return
template <typename G, typename W> static int pattern_run_as(const hgs_pattern_params* p, void* dev_out, int out_bytes, hipStream_t stream, W&& wrap) {
    GridDevice<G> grid;
    if (int e = grid.upload(p->x_axis, p->y_axis, p->x_grid, p->y_grid, p->h, p->w, stream)) return e;
    PatArgs<G, void> a{};
    pattern_args<G>(p, a);
    a.out = dev_out; a.x = grid.x; a.y = grid.y;
    if (int e = wrap([&]() -> int { LCHK(launch_pattern<G>(p->mode, grid.product, out_bytes, stream, a)); return 0; })) return e;
    HIPCHK(hipStreamSynchronize(stream));        // (the buffers of grid go with this scope)
    return 0;
}
template <typename W> static int pattern_run(const hgs_pattern_params* p, void* dev_out, int out_bytes, hipStream_t stream, W&& wrap) {
    return p->grid_bytes == 4 ? pattern_run_as<float>(p, dev_out, out_bytes, stream, wrap)
                              : pattern_run_as<double>(p, dev_out, out_bytes, stream, wrap);
}

struct EngineBase {
    int device = 0;      // HIP device ordinal of this engine; every C-ABI entry makes it current first
    DispatchLog dispatch;    // kernel instances launched since the last hgs_dispatch_read
    virtual ~EngineBase() {}
    virtual int init(const hgs_config& c) = 0;
    virtual int set_array(int which, const void* src, size_t nbytes, bool src_device) = 0;
    // device-resident phase of another engine (same SLM shape, precision and batch); PhaseRef: see phase_ref()
    struct PhaseRef { const void* ptr; size_t S; int B; int real_bytes; int device; hipStream_t stream; };
    virtual int phase_ref(PhaseRef* out) = 0;
    virtual int copy_phase_from(const PhaseRef& src) = 0;
    virtual int get_array(int which, void* dst, size_t nbytes, bool dst_device) = 0;
    virtual int reset_weights() = 0;
    virtual int reset_state() = 0;
    virtual int set_array_sparse(int which, const int32_t* xy, const void* values, int n) = 0;
    virtual int n2f(int store_pff) = 0;
    virtual int constraint(hgs_step* st) = 0;
    virtual int f2n() = 0;
    // MultiplaneHologram support: inverse transform without phase extraction, and the cross-engine combine
    struct MpInfo { void* nf; const void* kern; void* phase; size_t S; int B; int real_bytes; int device; hipStream_t stream; };
    virtual int f2n_complex() = 0;
    virtual int mp_info(MpInfo* out) = 0;
    virtual int mp_combine(const MpInfo* infos, const double* weights, int n) = 0;
    virtual int iterate(hgs_step* st, int n, uint8_t* hist) = 0;
    virtual int iterate_stats(hgs_step* st, int n, uint8_t* hist, int groups, int width, const double* xy,
                              double* out) = 0;
    virtual int stats(int group, int width, const double* xy, double* out) = 0;
    virtual int sync() = 0;
    virtual int set_option(int option, int value) = 0;
    virtual int profile_enable(int on) = 0;
    virtual int profile_read(double* out) = 0;
    virtual int iterate_timed(hgs_step* st, int n, double* ms) = 0;
    virtual int cg_iterate(const hgs_cg_params* p, int n, double* loss_out) = 0;
    virtual int remove_vortices(int32_t* n_removed) = 0;
    virtual int get_display(const hgs_display_params* p, void* dst, size_t nbytes, bool dst_device) = 0;
    virtual int set_array_poly(int which, const hgs_poly_params* p) = 0;
    virtual int set_array_pattern(int which, const hgs_pattern_params* p) = 0;
};

template <typename R> struct Engine : EngineBase {
    using C = Cx<R>;
    hgs_config cfg{};
    Geo g{};
    hipStream_t stream = nullptr;
    size_t S = 0, P = 0;  // elements per hologram
    int B = 1;
    // device buffers
    DevBuf<R> phase, amp, kern, w, t, pff, aff, wscale;
    DevBuf<C> gh, ff, zw;
    DevBuf<C> gh2;         // single-pass MRAF: the noise-region part of the field between the column and the row kernel
    DevBuf<char> staging;  // B*P complex, natural-layout bounce buffer for set/get
    DevBuf<C> tw_row, tw_col_own;     // square pads share one table: tw_col is tw_row then, else tw_col_own
    C* tw_col = nullptr;
    DevBuf<double> wpartial, fpartial;
    DevBuf<double> dpartial;  // partials of col_presum_kernel (single-inverse MRAF), sized like wpartial
    DevBuf<double> epartial;  // elementwise partials
    DevBuf<double> sums;      // [3][B]: fsum, nogsum, wsum
    DevBuf<int> spot_xy;
    DevBuf<double> spot_amp, ext_amp;
    DevBuf<R> spot_fb;
    DevBuf<C> nfbuf;               // [B][Sh][Sw] complex nearfield of f2n_complex (MultiplaneHologram)
    DevBuf<R> nog_dev;             // [B] -1/mean(fc) of the fused WGS-Nogrette pass
    // sparse targets (spot arrays): columns that hold a non-zero weight or target
    DevBuf<unsigned char> col_active;   // [B][Pw]
    DevBuf<unsigned short> sig_rows;    // [B][Pw] register slots of a column that hold signal pixels (scan_active_cols; col_presum_kernel)
    ColList active;                     // any bit of col_active
    // col_tile2_kernel, flag-reading instances: the ascending tiles that hold anything per hologram and how many (built with the
    // scan, refresh_sparse), and the weight-norm slots per (hologram, tile, half, wave) of their updating launches (ColLaunch::wslots).
    // A slot of an EMPTY half tile reads +0 for as long as the scan is current: the buffer is cleared where it is made and with
    // every scan, a launch that walks past the half tile never writes it, and one that visits it (no flags, an option off)
    // sums the squares of weights that are all zero -- every pixel of such a column leaves the rule at wave_all_zero.
    DevBuf<int> tile_list, tile_list_n;       // [B][Pw/4], [B]
    DevBuf<double> wslots;                    // [B][tile2_wslots(Pw)]
    DevBuf<unsigned short> lane_mask_noise;   // row-kernel view of its bit 4: columns with a NaN target (noise part of single-pass MRAF)
    // the same for the columns the spot integration windows touch (spot feedback / spot statistics)
    DevBuf<unsigned char> col_active_d;
    ColList dilated;
    bool sparse_tiles = false;             // the active set is whole 4-column tiles (the tile-resident kernel walks the list)
    // engine policy (hgs_set_option) and the developer switches, read from the environment once, in init() (read_tuning)
    Tuning tun;
    int opt_stepwise = 0;                  // HGS_OPT_FORCE_STEPWISE
    int opt_roctx = 0;                     // HGS_OPT_ROCTX: roctx ranges around the operators
    // what the buffers currently hold (G left behind, farfield, phase_ff, the weights' norm, the column lists): engine_state.hpp
    EngineState state;
    // HGS_OPT_KEEP_PREV_PHASE: the phase a one-iteration fused call started from (what its farfield phase describes)
    DevBuf<R> phase_prev;
    int opt_prev_phase = 0;
    // hgs_cg_iterate (optimize(method="CG")): Adam moments and the last gradient over the SLM window, the partial sums of the
    // seed pass and one loss per body of the running call; all allocated by the first call.  cg_t: Adam's step counter
    DevBuf<R> cg_m, cg_v, cg_grad;
    DevBuf<double> cg_partial;      // [ew_blocks]
    DevBuf<double> cg_loss;         // [cg_loss_cap] sum r^2 of each body
    int cg_loss_cap = 0, cg_t = 0;
    // hgs_remove_vortices: per-block counts / offsets of the search, the list (x, y, w) of the last call (grown to the
    // count the host reads once per call) and that count, device resident for the removal; vx_n: the host's copy, -1 = no call yet
    DevBuf<unsigned> vx_counts;
    DevBuf<int32_t> vx_list, vx_count;
    unsigned vx_cap = 0;
    int vx_n = -1;
    // hgs_get_display: the wavefront correction (HGS_DISPLAY_CORRECTION, double in either precision), the (max, min) pairs of
    // the range pass and the gray levels before they leave (the kernels store packed quads: an address of the engine's own)
    DevBuf<double> disp_corr, disp_partial;
    DevBuf<char> disp_out;
    bool has_disp_corr = false;
    // per-column kernel (float64; float32 where the tile-resident kernel does not run) single-pass MRAF: noise part as farfield
    // values, the columns that hold it, their inverse pass
    DevBuf<C> ffb;                      // [B][P], layout of ff; only NaN-target pixels are ever written, the rest stays zero
    ColList noise;                      // columns with a NaN target (bit 4 of col_active); its mask is not used
    ColList signal;                     // columns with a finite non-zero target (bit 1 of col_active): the per-column pre-pass of
                                        // the single-inverse MRAF update walks them; its mask is not used
    int row_blocks_pref = 0;               // its grid: two workgroups per CU, whole XCD line groups
    // statistics of the fused path (hgs_iterate_stats)
    DevBuf<double> stats_scratch;  // hgs_stats group 0: per-block partials of the two passes
    DevBuf<int> stats_dxy;         // hgs_stats group 1: floor(spot_knm)
    DevBuf<double> stat_partial;   // [B][blocks][STAT_WAVES][STAT_N]
    DevBuf<double> stat_tsum;      // [B] sum T^2
    struct StatCtx { int groups = 0, width = 1; DevBuf<double> dev_out; DevBuf<int> dxy; };
    StatCtx* stat_ctx = nullptr;      // non-null while hgs_iterate_stats drives the fused loop
    size_t stat_nslots = 0;
    // padded shapes that are not powers of two in [64, 8192]: Bluestein path (bluestein.hpp)
    bool general = false;
    int blue_M[2] = {0, 0};            // convolution lengths for x (rows, N = Pw) and y (columns, N = Ph)
    bool blue_plain[2] = {false, false};   // the axis is a power of two: M = N, no convolution
    DevBuf<C> blue_tab[2][2][3];       // [x|y][forward|inverse][A, Bf, Cc]
    DevBuf<C> blue_tw_own[2];          // equal convolution lengths share one table: blue_tw[1] is blue_tw[0] then
    C* blue_tw[2] = {nullptr, nullptr};
    // kind 1 (compressed): the uploaded problem, the tables of its kernel forms and their launches (compressed_backend.hpp);
    // ext_r: the external feedback amplitudes, converted for the constraint kernels
    CompressedBackend<R> comp;
    DevBuf<R> ext_r;
    // host state
    double amp_scalar = 0, amp_norm2 = 1.0;
    bool has_amp = false, has_kern = false, has_target = false, has_spots = false;
    int row_blocks = 0, col_blocks = 0, ew_blocks = 0, n_cu = 256, row_xcd = 0, tile_blocks = 0, col_xmap = 0;
    // profiling
    bool prof = false;
    struct Ev { int kind; hipEvent_t a, b; };
    std::vector<Ev> evs;
    double prof_ms[HGS_K_COUNT] = {0};
    double prof_n[HGS_K_COUNT] = {0};

    // The buffers are DevBuf members: they free themselves after this body, i.e. after hipStreamDestroy.  The stream is
    // drained first, so nothing uses them any more, and hipFree does not depend on the current device (hgs_destroy sets none).
    ~Engine() override {
        if (stream) hipStreamSynchronize(stream);
        for (auto& e : evs) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
        for (hipEvent_t ev : timed_ev) if (ev) hipEventDestroy(ev);
        if (stream) hipStreamDestroy(stream);
    }

    // host -> device on the engine stream, complete on return (ordered against in-flight kernels of this
    // engine; the caller's buffer may be reused immediately)
    int h2d(void* dst, const void* src, size_t nbytes, bool src_device = false) {
        HIPCHK(hipMemcpyAsync(dst, src, nbytes, src_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    // device -> host (or device), complete on return
    int d2h(void* dst, const void* src, size_t nbytes, bool dst_device = false) {
        HIPCHK(hipMemcpyAsync(dst, src, nbytes, dst_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    // n zeroed elements (the memset on the engine stream); need / need_zeroed: by the first call that uses the buffer
    template <typename T> int dalloc(DevBuf<T>& b, size_t n) { HIPCHK(b.alloc_zeroed(n, stream)); return 0; }
    template <typename T> int need(DevBuf<T>& b, size_t n) { HIPCHK(b.ensure(n)); return 0; }
    template <typename T> int need_zeroed(DevBuf<T>& b, size_t n) { HIPCHK(b.ensure_zeroed(n, stream)); return 0; }

    int make_twiddles(DevBuf<C>& dev, int N) {
        std::vector<C> h(N);
        for (int i = 0; i < N; ++i) {
            const double a = -2.0 * M_PI * (double)i / (double)N;
            h[i].x = (R)cos(a);
            h[i].y = (R)sin(a);
        }
        // exact values on the axes (cos(pi/2) is 6e-17 in double, rounds fine, but keep them exact)
        h[0].x = 1; h[0].y = 0;
        h[N / 4].x = 0; h[N / 4].y = -1;
        h[N / 2].x = -1; h[N / 2].y = 0;
        h[3 * N / 4].x = 0; h[3 * N / 4].y = 1;
        HIPCHK(dev.alloc(N));
        return h2d(dev, h.data(), N * sizeof(C));
    }

    // the developer switches, in the order include/hgs.h lists them: the one place the environment is read
    static Tuning read_tuning(int n_cu, int pad_h) {
        Tuning t;
        t.row_blocks = env_int("HGS_ROW_BLOCKS", n_cu * 64);
        t.col_blocks = env_int("HGS_COL_BLOCKS", n_cu * 3);
        // (8192 rows: one workgroup fits a CU, so 2 x #CU workgroups run as two rounds whose first tile each comes without
        //  the LDS staging of the previous one; one round of #CU workgroups with twice the tiles: cfg5pad 213.2 -> 209.6 us)
        t.tile_blocks = env_int("HGS_TILE_BLOCKS", pad_h >= 8192 ? n_cu : n_cu * 2);
        t.tile2_blocks = env_int("HGS_TILE2_BLOCKS", 0);
        t.row_pref_blocks = env_int("HGS_ROW_PREF_BLOCKS", 2 * n_cu);
        t.row_xcd = env_int("HGS_ROW_XCD", 1);
        t.col_xmap = env_int("HGS_COL_XMAP", 1);
        t.row_shift = env_int("HGS_ROW_SHIFT", 1);
        t.row_shift64 = env_int("HGS_ROW_SHIFT64", 1);
        t.row_pref = env_int("HGS_ROW_PREF", 1);
        t.row_pref_batch = env_int("HGS_ROW_PREF_BATCH", 0);
        t.tile_rule = env_int("HGS_TILE_RULE", 1);
        t.mraf_split = env_int("HGS_MRAF_SPLIT", 1);
        t.mraf_split64 = env_int("HGS_MRAF_SPLIT64", 1);
        t.gh2_mask = env_int("HGS_GH2_MASK", 1);
        t.tile_list = env_int("HGS_TILE_LIST", 1);
        t.tile_shift16 = env_int("HGS_TILE_SHIFT16", 1);
        t.tile_nr4 = env_int("HGS_TILE_NR4", 1);
        t.tile2 = env_int("HGS_TILE2", 1);
        t.tile2_min_batch = env_int("HGS_TILE2_MIN_BATCH", 1);
        t.tile2_phase2 = env_int("HGS_TILE2_PHASE2", 1);
        t.keep_g = env_int("HGS_KEEP_G", 1);
        t.fused_shift = env_int("HGS_FUSED_SHIFT", 1);
        t.mono_tab = env_int("HGS_MONO_TAB", 1);
        t.mraf_presum = env_int("HGS_MRAF_PRESUM", 1);
        t.presum_rows = env_int("HGS_PRESUM_ROWS", 1);
        t.presum_blocks = env_int("HGS_PRESUM_BLOCKS", 0);
        t.empty_col_loads = env_int("HGS_EMPTY_COL_LOADS", 1);
        t.empty_col_inverse = env_int("HGS_EMPTY_COL_INVERSE", 1);
        t.empty_col_forward = env_int("HGS_EMPTY_COL_FORWARD", 1);
        t.empty_col_prezero = env_int("HGS_EMPTY_COL_PREZERO", 1);
        t.empty_col_list = env_int("HGS_EMPTY_COL_LIST", 1);
        return t;
    }

    int init(const hgs_config& c) override {
        cfg = c;
        device = c.device;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            return fail(HGS_ERR_DEVICE, "no HIP device available (the engine has no CPU fallback)");
        if (c.device < 0 || c.device >= ndev) return fail(HGS_ERR_ARG, "device %d out of range", c.device);
        HIPCHK(hipSetDevice(c.device));
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, c.device));
        n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        tun = read_tuning(n_cu, c.pad_h);
        if (c.kind == 1) return init_compressed(c);
        if (c.kind != 0) return fail(HGS_ERR_ARG, "unknown engine kind %d", c.kind);
        const bool fast = is_pow2(c.pad_h) && is_pow2(c.pad_w) && c.pad_h >= 64 && c.pad_w >= 64 && c.pad_h <= 8192 &&
                          c.pad_w <= 8192;
        if (!fast) {
            // any other shape runs axis by axis on the workgroup transforms: a power-of-two axis up to 16384 (fp64:
            // 8192) directly, any other length up to 8192 (fp64: 4096) through Bluestein's identity
            if (!axis_ok(c.pad_h) || !axis_ok(c.pad_w))
                return fail(HGS_ERR_UNSUPPORTED, "padded shape (%d, %d): per axis a power of two up to %d or any length "
                            "in [2, %d] (%s)", c.pad_h, c.pad_w, max_line(), max_line() / 2, sizeof(R) == 4 ? "float32" : "float64");
            general = true;
        }
        if (c.slm_h < 1 || c.slm_w < 1 || c.slm_h > c.pad_h || c.slm_w > c.pad_w)
            return fail(HGS_ERR_ARG, "slm shape (%d, %d) does not fit the padded shape (%d, %d)", c.slm_h,
                        c.slm_w, c.pad_h, c.pad_w);
        if (c.batch < 1) return fail(HGS_ERR_ARG, "batch must be >= 1");
        g.Ph = c.pad_h; g.Pw = c.pad_w; g.Sh = c.slm_h; g.Sw = c.slm_w;
        g.r0 = (c.pad_h - c.slm_h) / 2;  // floor((P-S)/2)  toolbox.unpad
        g.c0 = (c.pad_w - c.slm_w) / 2;
        g.batch = B = c.batch;
        g.lane_T = general ? 0 : g.Ph / 16;
        S = (size_t)g.Sh * g.Sw;
        P = (size_t)g.Ph * g.Pw;
        // HGS_TRACE_INIT=1: where hgs_create spends its time (developer aid, stderr)
        const bool trace_init = env_int("HGS_TRACE_INIT", 0) != 0;
        auto t_prev = std::chrono::steady_clock::now();
        auto lap = [&](const char* what) {
            if (!trace_init) return;
            const auto t_now = std::chrono::steady_clock::now();
            fprintf(stderr, "hgs_create: %-28s %8.1f us\n", what, std::chrono::duration<double, std::micro>(t_now - t_prev).count());
            t_prev = t_now;
        };
        HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        lap("stream");
        if (general) return init_general(c);

        // grid sizes: enough workgroups to fill the chip a few times over, balanced over the work
        const int fpw = row_fpw(g.Pw);
        const int row_units = (g.Sh + fpw - 1) / fpw;
        // one-row workgroups balance best (the hardware dispatcher hands a free slot the next row); a batch keeps them up
        // to 64 workgroups per CU (cfg 3, 8 x 1152 rows: 187.6 -> 171.4 us per row launch against 256 per hologram)
        int cap = tun.row_blocks;
        cap = cap / B > 0 ? cap / B : 1;
        int per = (row_units + cap - 1) / cap;
        row_blocks = (row_units + per - 1) / per;
        // XCD-aware row mapping (row_kernel): the 4 / fpw workgroups of a 128-byte line group on one XCD together
        const int grp = fpw <= 4 ? 4 / fpw : 1;
        row_xcd = (grp > 1 && row_blocks >= 8 * grp && tun.row_xcd) ? 1 : 0;
        if (row_xcd) row_blocks = (row_blocks + 8 * grp - 1) / (8 * grp) * (8 * grp);
        // prefetching row kernel (one hologram; a batch keeps the one-row workgroups): 2 workgroups per CU
        // (round 5: a batch walks too where every workgroup gets at least four rows -- 8 x 1152 rows over 2 x #CU workgroups
        //  are 18 rows each, no partial round at all; HGS_ROW_PREF_BATCH=0 keeps its one-row workgroups)
        row_blocks_pref = 0;
        if (sizeof(R) == 4 && g.Pw == 4096 && fpw == 1 && row_xcd && (B == 1 || tun.row_pref_batch)) {
            const int want = tun.row_pref_blocks / B;
            row_blocks_pref = std::max(8 * grp, want / (8 * grp) * (8 * grp));
        }
        const int tiles = g.Pw / 4;
        cap = tun.col_blocks;
        cap = cap / B > 0 ? cap / B : 1;
        per = (tiles + cap - 1) / cap;
        col_blocks = (tiles + per - 1) / per;
        // per-column fused kernel with several passes per tile (ColCfg: fewer than four columns side by side): a grid that
        // is a multiple of 8 * passes lets the passes of a tile run on one XCD at a time (ColArgs::col_xmap); among those
        // the one that wastes the least of its last sweep, the larger on a tie
        col_xmap = 0;
        {
            const int Tc = g.Ph / 16, cpar = Tc >= 256 ? 1 : std::min(4, 256 / Tc), passes = 4 / cpar, q = 8 * passes;
            if (passes > 1 && tun.col_xmap) {
                double best = 0;
                int best_g = 0;
                for (int G = q; G <= cap && G / passes <= tiles; G += q) {
                    const int gp = G / passes, sweeps = (tiles + gp - 1) / gp;
                    const double eff = (double)tiles / ((double)sweeps * gp);
                    if (eff >= best - 1e-9) { best = eff; best_g = G; }
                }
                if (best_g > 0 && best >= 0.9) { col_blocks = best_g; col_xmap = 1; }
            }
        }
        tile_blocks = std::max(1, std::min(tiles, tun.tile_blocks / B));
        ew_blocks = (int)std::min<size_t>((P + 255) / 256, (size_t)std::max(1, n_cu * 8 / B));

        if (dalloc(phase, B * S)) return HGS_ERR_DEVICE;
        lap("phase");
        if (dalloc(gh, (size_t)B * g.Sh * g.Pw)) return HGS_ERR_DEVICE;
        lap("gh");
        if (dalloc(w, B * P) || dalloc(t, B * P)) return HGS_ERR_DEVICE;
        lap("weights + target");
        if (int e = alloc_partials((size_t)B * std::max(std::max(col_blocks, tile_blocks), n_cu * 3), (size_t)B * std::max(col_blocks, n_cu * 3))) return e;
        lap("partials");
        if (int e = make_twiddles(tw_row, g.Pw)) return e;
        if (g.Ph != g.Pw) { if (int e = make_twiddles(tw_col_own, g.Ph)) return e; }
        tw_col = g.Ph == g.Pw ? tw_row : tw_col_own;          // square pads: one table
        lap("twiddles");
        if (int e = alloc_spots(c.n_spots)) return e;
        lap("spots");
        HIPCHK(hipStreamSynchronize(stream));
        lap("sync");
        return 0;
    }
    // the partial sums every kind of engine folds, and wscale = 1; the source amplitude starts as the scalar 1 / sqrt(S)
    // (Hologram.__init__ :401-402)
    int alloc_partials(size_t n_wpartial, size_t n_fpartial) {
        if (dalloc(wpartial, n_wpartial) || dalloc(fpartial, n_fpartial) || dalloc(epartial, (size_t)B * ew_blocks) ||
            dalloc(sums, (size_t)4 * B) || dalloc(wscale, (size_t)B)) return HGS_ERR_DEVICE;
        amp_scalar = 1.0 / std::sqrt((double)S);
        amp_norm2 = 1.0;
        return fill_wscale_one();
    }
    int alloc_spots(int n_spots) {
        if (n_spots <= 0) return 0;
        if (dalloc(spot_xy, (size_t)2 * n_spots) || dalloc(spot_amp, (size_t)n_spots) || dalloc(ext_amp, (size_t)n_spots) ||
            dalloc(spot_fb, (size_t)B * n_spots)) return HGS_ERR_DEVICE;
        return 0;
    }

    // ---- general padded shapes (Bluestein) ----------------------------------------------------------
    // the longest line one workgroup transforms: 1024 lanes x 16 elements, LDS image (17/16) * 16384 * sizeof(C)
    static constexpr int max_line() { return sizeof(R) == 4 ? 16384 : 8192; }
    static bool axis_plain(int N) { return is_pow2(N) && N >= 256 && N <= max_line(); }
    static bool axis_ok(int N) { return N >= 2 && (axis_plain(N) || 2 * N - 1 <= max_line()); }
    static void host_fft(std::vector<std::complex<double>>& a) {      // in-place radix-2, forward sign
        const size_t n = a.size();
        for (size_t i = 1, j = 0; i < n; ++i) {
            size_t bit = n >> 1;
            for (; j & bit; bit >>= 1) j ^= bit;
            j ^= bit;
            if (i < j) std::swap(a[i], a[j]);
        }
        for (size_t len = 2; len <= n; len <<= 1) {
            const double ang = -2.0 * M_PI / (double)len;
            for (size_t i = 0; i < n; i += len)
                for (size_t k = 0; k < len / 2; ++k) {
                    const std::complex<double> w(std::cos(ang * (double)k), std::sin(ang * (double)k));
                    const std::complex<double> u = a[i + k], v = a[i + k + len / 2] * w;
                    a[i + k] = u + v;
                    a[i + k + len / 2] = u - v;
                }
        }
    }
    // tables of one centred transform of length N (bluestein.hpp): dir = -1 forward, +1 inverse
    // plain: no chirp (A = pre, Cc = post / sqrt(N), Bf unused but allocated as one element)
    int make_blue_tables(int N, int M, int dir, bool plain, DevBuf<C>* out3) {
        using cd = std::complex<double>;
        const long long h = N / 2;
        const double sg = dir < 0 ? -1.0 : 1.0;
        auto unit = [&](long long num, long long den, double sign) {     // exp(sign * 2 pi i * num / den), num reduced first
            long long r = num % den;
            if (r < 0) r += den;
            const double a = sign * 2.0 * M_PI * (double)r / (double)den;
            return cd(std::cos(a), std::sin(a));
        };
        std::vector<cd> chirp(N), A(N), Cc(N), bt(plain ? 1 : M, cd(0, 0));
        for (long long n = 0; n < N; ++n) chirp[n] = plain ? cd(1, 0) : unit(n * n, 2LL * N, sg);   // W^(n^2/2), W = exp(sg 2 pi i / N)
        const double sc = 1.0 / std::sqrt((double)N);
        for (long long n = 0; n < N; ++n) {
            // forward: pre = W^(-n h), post = W^(h (k - h));  inverse (W -> conj W): pre = Wc^(n h), post = Wc^(-h (i + h))
            const cd pre = dir < 0 ? unit(-n * h, N, -1.0) : unit(n * h, N, 1.0);
            const cd post = dir < 0 ? unit(h * (n - h), N, -1.0) : unit(-h * (n + h), N, 1.0);
            A[n] = pre * chirp[n];
            Cc[n] = post * chirp[n] * sc;
        }
        if (!plain) {
            bt[0] = std::conj(chirp[0]);
            for (int d = 1; d < N; ++d) bt[d] = bt[M - d] = std::conj(chirp[d]);
            host_fft(bt);
            for (auto& v : bt) v /= (double)M;
        }
        auto up = [&](const std::vector<cd>& src, DevBuf<C>& dst) -> int {
            std::vector<C> hbuf(src.size());
            for (size_t i = 0; i < src.size(); ++i) { hbuf[i].x = (R)src[i].real(); hbuf[i].y = (R)src[i].imag(); }
            HIPCHK(dst.alloc(hbuf.size()));
            return h2d(dst, hbuf.data(), hbuf.size() * sizeof(C));
        };
        if (int e = up(A, out3[0])) return e;
        if (int e = up(bt, out3[1])) return e;
        return up(Cc, out3[2]);
    }
    int init_general(const hgs_config& c) {
        auto conv_len = [](int N) { if (axis_plain(N)) return N; int M = 256; while (M < 2 * N - 1) M <<= 1; return M; };
        blue_M[0] = conv_len(g.Pw);
        blue_M[1] = conv_len(g.Ph);
        blue_plain[0] = axis_plain(g.Pw);
        blue_plain[1] = axis_plain(g.Ph);
        {   // one workgroup holds a whole line in LDS ((17/16) M complex numbers): fail here, with a message, rather
            // than at the first transform with a raw HIP error
            int lds_max = 0;
            HIPCHK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, c.device));
            const size_t need = (size_t)(std::max(blue_M[0], blue_M[1]) / 16 * 17) * sizeof(C);
            if (need > (size_t)lds_max)
                return fail(HGS_ERR_UNSUPPORTED, "padded shape (%d, %d) needs %zu bytes of LDS per workgroup, the device offers %d",
                            c.pad_h, c.pad_w, need, lds_max);
        }
        ew_blocks = (int)std::min<size_t>((P + 255) / 256, (size_t)std::max(1, n_cu * 8 / B));
        col_blocks = tile_blocks = row_blocks = 1;
        if (dalloc(phase, B * S) || dalloc(gh, (size_t)B * g.Sh * g.Pw) || dalloc(nfbuf, B * S) || dalloc(w, B * P) || dalloc(t, B * P))
            return HGS_ERR_DEVICE;
        if (int e = alloc_partials((size_t)B * n_cu * 3, (size_t)B * std::max(ew_blocks, n_cu * 3))) return e;
        for (int d = 0; d < 2; ++d) {
            const int N = d == 0 ? g.Pw : g.Ph;
            if (d == 1 && blue_M[1] == blue_M[0]) blue_tw[1] = blue_tw[0];
            else if (int e = make_twiddles(blue_tw_own[d], blue_M[d])) return e;
            else blue_tw[d] = blue_tw_own[d];
            if (int e = make_blue_tables(N, blue_M[d], -1, blue_plain[d], blue_tab[d][0])) return e;
            if (int e = make_blue_tables(N, blue_M[d], +1, blue_plain[d], blue_tab[d][1])) return e;
        }
        if (int e = alloc_spots(c.n_spots)) return e;
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    int blue_pass(int dim, int dir, const C* in, size_t in_line, size_t in_batch, int in_stride, int in_start, int in_len,
                  C* out, size_t out_line, size_t out_batch, int out_stride, int out_start, int out_len, int lines) {
        BlueArgs<R> a{};
        a.in = in; a.out = out; a.in_line = in_line; a.out_line = out_line; a.in_batch = in_batch; a.out_batch = out_batch;
        a.in_stride = in_stride; a.out_stride = out_stride; a.in_start = in_start; a.in_len = in_len;
        a.out_start = out_start; a.out_len = out_len; a.N = dim == 0 ? g.Pw : g.Ph;
        const DevBuf<C>* t3 = blue_tab[dim][dir < 0 ? 0 : 1];
        a.A = t3[0]; a.Bf = t3[1]; a.Cc = t3[2]; a.tw = blue_tw[dim];
        a.plain = blue_plain[dim] ? (dir < 0 ? 1 : 2) : 0;
        LCHK(launch_bluestein<R>(blue_M[dim], dim3(lines, B), stream, a));
        return 0;
    }
    int n2f_general(int store_pff) {
        if (int e = need_ff()) return e;
        if (store_pff) { if (int e = need_pff()) return e; }
        int r = timed(HGS_K_ROW, [&]() -> int {
            hipLaunchKernelGGL(gen_build_nearfield<R>, dim3((unsigned)((S + 255) / 256), B), dim3(256), 0, stream, (const R*)phase,
                               has_amp ? (const R*)amp : (const R*)nullptr, has_kern ? (const R*)kern : (const R*)nullptr,
                               (R)amp_scalar, S, nfbuf);
            HIPCHK(hipGetLastError());
            // rows: nearfield block (zero outside the SLM columns) -> G[r][kx]
            return blue_pass(0, -1, nfbuf, g.Sw, S, 1, g.c0, g.Sw, gh, g.Pw, (size_t)g.Sh * g.Pw, 1, 0, g.Pw, g.Sh);
        });
        if (r) return r;
        r = timed(HGS_K_COL_FWD, [&]() -> int {
            // columns: G[:, kx] (zero outside the SLM rows) -> farfield, column-major
            if (int e = blue_pass(1, -1, gh, 1, (size_t)g.Sh * g.Pw, g.Pw, g.r0, g.Sh, ff, g.Ph, P, 1, 0, g.Ph, g.Pw)) return e;
            hipLaunchKernelGGL(gen_amp_store<R>, dim3(ew_blocks, B), dim3(256), 0, stream, (const C*)ff, aff,
                               store_pff ? pff : (R*)nullptr, P, fpartial);
            HIPCHK(hipGetLastError());
            return 0;
        });
        if (r) return r;
        if (int e = reduce(fpartial, ew_blocks, sums + 0 * B)) return e;
        state.farfield_materialised(store_pff != 0);
        return 0;
    }
    int f2n_general(bool complex_only) {
        if (!ff || !state.farfield_valid()) return fail(HGS_ERR_STATE, "no farfield to transform back");
        int r = timed(HGS_K_COL_INV, [&]() -> int {
            return blue_pass(1, +1, ff, g.Ph, P, 1, 0, g.Ph, gh, 1, (size_t)g.Sh * g.Pw, g.Pw, g.r0, g.Sh, g.Pw);
        });
        if (r) return r;
        state.farfield_consumed();
        return timed(HGS_K_ROW, [&]() -> int {
            if (int e = blue_pass(0, +1, gh, g.Pw, (size_t)g.Sh * g.Pw, 1, 0, g.Pw, nfbuf, g.Sw, S, 1, g.c0, g.Sw, g.Sh)) return e;
            if (!complex_only) {
                hipLaunchKernelGGL(gen_extract_phase<R>, dim3((unsigned)((S + 255) / 256), B), dim3(256), 0, stream, (const C*)nfbuf,
                                   has_kern ? (const R*)kern : (const R*)nullptr, S, phase);
                HIPCHK(hipGetLastError());
            }
            return 0;
        });
    }

    // ---- kind 1: CompressedSpotHologram (the transforms themselves: compressed_backend.hpp) -------
    CompressedView<R> cview() const {
        return {stream, B, S, P, g, n_cu, phase.get(), has_amp ? amp.get() : nullptr, has_kern ? kern.get() : nullptr, amp_scalar,
                ff.get(), aff.get(), sums.get()};
    }
    int init_compressed(const hgs_config& c) {
        if (c.n_spots < 1 || c.n_monomials < 1 || c.slm_h < 1 || c.slm_w < 1 || c.batch < 1)
            return fail(HGS_ERR_ARG, "compressed engine needs n_spots, n_monomials, slm shape and batch >= 1");
        g.Sh = c.slm_h; g.Sw = c.slm_w; g.r0 = g.c0 = 0;
        g.Ph = c.n_spots; g.Pw = 1;      // farfield-sized arrays are N-vectors; the transposes degenerate
        g.batch = B = c.batch;
        S = (size_t)g.Sh * g.Sw;
        P = (size_t)c.n_spots;
        HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        col_blocks = 1; tile_blocks = 1; row_blocks = 1;
        ew_blocks = (int)std::min<size_t>((P + 255) / 256, (size_t)std::max(1, n_cu * 8 / B));
        if (dalloc(phase, B * S) || dalloc(w, B * P) || dalloc(t, B * P)) return HGS_ERR_DEVICE;
        if (int e = comp.init(cview(), c.n_spots, c.n_monomials, tun.mono_tab)) return e;
        if (dalloc(ext_amp, P) || dalloc(ext_r, B * P)) return HGS_ERR_DEVICE;
        if (int e = alloc_partials((size_t)B, (size_t)B)) return e;
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    int compressed_ready() {
        if (!comp.uploaded())
            return fail(HGS_ERR_STATE, "compressed engine needs HGS_XGRID, HGS_YGRID, HGS_MONOMIALS and HGS_SPOT_COEFF");
        return 0;
    }
    int n2f_compressed(int store_pff) {
        if (int e = compressed_ready()) return e;
        if (int e = need_ff()) return e;
        if (store_pff) { if (int e = need_pff()) return e; }
        int r = timed(HGS_K_COL_FWD, [&]() -> int { return comp.n2f(cview()); });
        if (r) return r;
        if (store_pff) {
            EwArgs<R> a{};
            a.P = P; a.batch = B; a.ff = ff; a.pff = pff;
            hipLaunchKernelGGL(ew_store_phase<R>, dim3(ew_blocks, B), dim3(256), 0, stream, a);
            HIPCHK(hipGetLastError());
        }
        state.farfield_materialised(store_pff != 0);
        return 0;
    }
    // nf_out: null extracts the phase; else the complex nearfield goes there and the phase stays (f2n_complex)
    int f2n_compressed(Cx<R>* nf_out = nullptr) {
        if (!ff || !state.farfield_valid()) return fail(HGS_ERR_STATE, "no farfield to transform back");
        int r = timed(HGS_K_COL_INV, [&]() -> int { return comp.f2n(cview(), nf_out); });
        state.farfield_consumed();
        return r;
    }

    // wscale = 1: the launch alone; what it means for the weights is the caller's event (weights_written, scale_folded)
    int fill_wscale_one() {
        hipLaunchKernelGGL(set_scalar<R>, dim3((B + 63) / 64), dim3(64), 0, stream, wscale.get(), B, (R)1);
        HIPCHK(hipGetLastError());
        return 0;
    }
    // the weights were written from outside the fused loop: whatever scale was pending is void
    int weights_written() {
        if (int e = fill_wscale_one()) return e;
        state.weights_written();
        return 0;
    }

    // ---- lazily allocated farfield-sized buffers ----
    int need_ff() { if (int e = need_zeroed(ff, B * P)) return e; return need_aff(); }
    int need_aff() { return need_zeroed(aff, B * P); }
    int need_pff() { return need_zeroed(pff, B * P); }
    int need_staging() { return need(staging, B * P * sizeof(C)); }
    int need_zw() { return need_zeroed(zw, B * P); }

    // ---- profiling wrapper ----
    template <typename F> int timed(int kind, F&& f) {
        if (!prof) return f();
        Ev e;
        e.kind = kind;
        HIPCHK(hipEventCreate(&e.a));
        HIPCHK(hipEventCreate(&e.b));
        HIPCHK(hipEventRecord(e.a, stream));
        int r = f();
        HIPCHK(hipEventRecord(e.b, stream));
        evs.push_back(e);
        return r;
    }
    int profile_enable(int on) override { prof = on != 0; return 0; }
    int profile_read(double* out) override {
        HIPCHK(hipStreamSynchronize(stream));
        for (auto& e : evs) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, e.a, e.b));
            prof_ms[e.kind] += ms;
            prof_n[e.kind] += 1;
            hipEventDestroy(e.a);
            hipEventDestroy(e.b);
        }
        evs.clear();
        for (int k = 0; k < HGS_K_COUNT; ++k) {
            out[2 * k] = prof_ms[k];
            out[2 * k + 1] = prof_n[k];
            prof_ms[k] = prof_n[k] = 0;
        }
        return 0;
    }

    // ---- natural <-> column-major moves through the staging buffer ----
    template <typename E> int upload_T(E* dst, const void* host, size_t nbytes, bool src_device = false) {
        // host natural [B][Ph][Pw] -> device column-major [B][Pw][Ph]
        const size_t one = P * sizeof(E);
        if (nbytes != one * B && nbytes != one) return fail(HGS_ERR_ARG, "array size %zu does not match %zu x {1,%d}", nbytes, one, B);
        if (int e = need_staging()) return e;
        E* st = reinterpret_cast<E*>(staging.get());
        for (int b = 0; b < B; ++b) {
            const char* src = (const char*)host + (nbytes == one ? 0 : (size_t)b * one);
            HIPCHK(hipMemcpyAsync(st + (size_t)b * P, src, one, src_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
        }
        dim3 grid((g.Pw + 31) / 32, (g.Ph + 31) / 32, B);
        hipLaunchKernelGGL((transpose_scale<E, R>), grid, dim3(32, 8), 0, stream, (const E*)st, dst, g.Ph, g.Pw,
                           (const R*)nullptr, cfg.kind == 0 ? g.lane_T : 0, 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    template <typename E> int download_T(const E* src, void* dst, size_t nbytes, bool dst_device, const R* scale) {
        const size_t all = P * sizeof(E) * B;
        if (nbytes != all) return fail(HGS_ERR_ARG, "array size %zu does not match %zu", nbytes, all);
        if (int e = need_staging()) return e;
        E* st = reinterpret_cast<E*>(staging.get());
        dim3 grid((g.Ph + 31) / 32, (g.Pw + 31) / 32, B);
        hipLaunchKernelGGL((transpose_scale<E, R>), grid, dim3(32, 8), 0, stream, src, st, g.Pw, g.Ph, scale,
                           cfg.kind == 0 ? g.lane_T : 0, 0);
        HIPCHK(hipGetLastError());
        return d2h(dst, st, all, dst_device);
    }

    int set_array(int which, const void* host, size_t nbytes, bool src_device) override {
        const bool nearfield_input = which == HGS_PHASE || which == HGS_AMP || which == HGS_AMP_SCALAR || which == HGS_PROP_KERNEL;
        if (nearfield_input) state.nearfield_upload_begins();
        if (which == HGS_PROP_KERNEL && nbytes == 0) {       // "no kernel" (Hologram.propagation_kernel = None / 0)
            has_kern = false;
            state.nearfield_input_changed();
            return 0;
        }
        if (which == HGS_DISPLAY_CORRECTION) {               // not a nearfield input: the loop never sees it
            if (src_device) return fail(HGS_ERR_UNSUPPORTED, "the display correction is uploaded with hgs_set_array");
            if (nbytes == 0) { has_disp_corr = false; return 0; }
            if (!host) return fail(HGS_ERR_ARG, "null source pointer");
            if (nbytes != S * sizeof(double)) return fail(HGS_ERR_ARG, "display correction: bad size %zu (%zu doubles expected)", nbytes, S);
            HIPCHK(disp_corr.ensure(S));
            has_disp_corr = false;
            if (int e_ = h2d(disp_corr, host, nbytes)) return e_;
            has_disp_corr = true;
            return 0;
        }
        if (!host) return fail(HGS_ERR_ARG, "null source pointer");
        const hipMemcpyKind kind = src_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        if (src_device && (which == HGS_XGRID || which == HGS_YGRID || which == HGS_MONOMIALS || which == HGS_SPOT_COEFF ||
                           which == HGS_SPOT_INDEX || which == HGS_AMP_SCALAR))
            return fail(HGS_ERR_UNSUPPORTED, "array selector %d is parsed on the host: upload it with hgs_set_array", which);
        switch (which) {
            case HGS_PHASE: {
                const size_t one = S * sizeof(R);
                if (nbytes != one * B && nbytes != one) return fail(HGS_ERR_ARG, "phase: bad size %zu", nbytes);
                for (int b = 0; b < B; ++b)
                    HIPCHK(hipMemcpyAsync(phase + (size_t)b * S, (const char*)host + (nbytes == one ? 0 : b * one), one, kind, stream));
                HIPCHK(hipStreamSynchronize(stream));
                state.nearfield_input_changed();
                return 0;
            }
            case HGS_AMP: {
                if (nbytes != S * sizeof(R)) return fail(HGS_ERR_ARG, "amp: bad size %zu", nbytes);
                HIPCHK(amp.ensure(S));
                if (int e_ = h2d(amp, host, nbytes, src_device)) return e_;
                has_amp = true;
                double s = 0;
                if (src_device) {         // ||amp||^2 on the device: per-block partials (double), folded here
                    const int nb = (int)std::min<size_t>((S + 255) / 256, 1024);
                    DevBuf<double> part;
                    HIPCHK(part.alloc((size_t)nb));
                    hipLaunchKernelGGL(ew_sumsq<R>, dim3(nb, 1), dim3(256), 0, stream, (const R*)amp, S, part.get());
                    if (hipGetLastError() != hipSuccess) return fail(HGS_ERR_DEVICE, "amplitude norm launch failed");
                    std::vector<double> hp(nb);
                    if (d2h(hp.data(), part, (size_t)nb * sizeof(double))) return fail(HGS_ERR_DEVICE, "amplitude norm failed");
                    for (double v : hp) s += v;
                } else {
                    const R* h = (const R*)host;
                    // (NaN entries skipped, like ew_sumsq on the device path and the reference's nansum normalisation)
                    for (size_t i = 0; i < S; ++i) { const double v = (double)h[i]; if (v == v) s += v * v; }
                }
                amp_norm2 = s;
                state.nearfield_input_changed();
                return 0;
            }
            case HGS_AMP_SCALAR: {
                if (nbytes != sizeof(R)) return fail(HGS_ERR_ARG, "amp scalar: bad size %zu", nbytes);
                amp_scalar = (double)*(const R*)host;
                has_amp = false;
                amp_norm2 = amp_scalar * amp_scalar * (double)S;
                state.nearfield_input_changed();
                return 0;
            }
            case HGS_PROP_KERNEL: {
                if (nbytes != S * sizeof(R)) return fail(HGS_ERR_ARG, "propagation kernel: bad size %zu", nbytes);
                HIPCHK(kern.ensure(S));
                if (int e_ = h2d(kern, host, nbytes, src_device)) return e_;
                has_kern = true;
                state.nearfield_input_changed();
                return 0;
            }
            case HGS_TARGET:
                has_target = true;
                state.target_written();
                return upload_T<R>(t.get(), host, nbytes, src_device);
            case HGS_WEIGHTS: {
                state.weights_write_begins();
                if (int e = upload_T<R>(w.get(), host, nbytes, src_device)) return e;
                return weights_written();
            }
            case HGS_PHASE_FF: {
                if (int e = need_pff()) return e;
                state.phase_ff_stored();
                return upload_T<R>(pff.get(), host, nbytes, src_device);
            }
            case HGS_ZERO_WEIGHTS: {
                if (int e = need_zw()) return e;
                return upload_T<C>(zw.get(), host, nbytes, src_device);
            }
            case HGS_XGRID:
            case HGS_YGRID: {
                if (cfg.kind != 1) return fail(HGS_ERR_STATE, "grids belong to the compressed engine");
                if (nbytes != S * sizeof(R)) return fail(HGS_ERR_ARG, "grid: bad size %zu", nbytes);
                state.geometry_changed();
                return comp.set_grid(cview(), which == HGS_XGRID ? 0 : 1, (const R*)host);
            }
            case HGS_MONOMIALS: {
                if (cfg.kind != 1) return fail(HGS_ERR_STATE, "monomials belong to the compressed engine");
                if (nbytes != (size_t)2 * cfg.n_monomials * sizeof(int32_t)) return fail(HGS_ERR_ARG, "monomials: bad size");
                if (comp.same_monomials((const int32_t*)host)) return 0;   // unchanged term set
                state.geometry_changed();
                return comp.set_monomials(cview(), (const int32_t*)host);
            }
            case HGS_SPOT_COEFF: {
                if (cfg.kind != 1) return fail(HGS_ERR_STATE, "spot coefficients belong to the compressed engine");
                if (nbytes != (size_t)cfg.n_monomials * cfg.n_spots * sizeof(R)) return fail(HGS_ERR_ARG, "spot coefficients: bad size");
                state.geometry_changed();
                return comp.set_coeff(cview(), (const R*)host);
            }
            case HGS_SPOT_INDEX: {
                if (cfg.n_spots <= 0) return fail(HGS_ERR_STATE, "engine was created with n_spots = 0");
                if (nbytes != (size_t)2 * cfg.n_spots * sizeof(int32_t)) return fail(HGS_ERR_ARG, "spot index: bad size");
                const int32_t* h = (const int32_t*)host;
                const int hw = 0;  // bounds are checked against the window at constraint time
                for (int n = 0; n < cfg.n_spots; ++n)
                    if (h[n] < hw || h[n] >= g.Pw || h[cfg.n_spots + n] < 0 || h[cfg.n_spots + n] >= g.Ph)
                        return fail(HGS_ERR_ARG, "spot %d outside the computational grid", n);
                if (int e_ = h2d(spot_xy, host, nbytes)) return e_;
                spot_xy_host.assign(h, h + 2 * cfg.n_spots);
                has_spots = true;
                return 0;
            }
            case HGS_SPOT_AMP:
            case HGS_EXTERNAL_AMP: {
                if (cfg.kind == 1 && which == HGS_SPOT_AMP) return fail(HGS_ERR_ARG, "compressed targets are set with HGS_TARGET");
                if (cfg.n_spots <= 0) return fail(HGS_ERR_STATE, "engine was created with n_spots = 0");
                if (nbytes != (size_t)cfg.n_spots * sizeof(double)) return fail(HGS_ERR_ARG, "spot amplitudes: bad size");
                return h2d(which == HGS_SPOT_AMP ? spot_amp : ext_amp, host, nbytes, src_device);
            }
        }
        return fail(HGS_ERR_ARG, "unknown array selector %d", which);
    }
    std::vector<int32_t> spot_xy_host;

    int phase_ref(PhaseRef* o) override {
        o->ptr = phase; o->S = S; o->B = B; o->real_bytes = (int)sizeof(R); o->device = cfg.device; o->stream = stream;
        return 0;
    }
    // phase <- the phase another engine holds, device to device (no host bounce); one source hologram broadcasts
    int copy_phase_from(const PhaseRef& src) override {
        if (src.S != S || src.real_bytes != (int)sizeof(R) || (src.B != B && src.B != 1))
            return fail(HGS_ERR_ARG, "hgs_copy_phase: engines differ in SLM shape, precision or batch");
        if (hipStreamSynchronize(src.stream) != hipSuccess) return fail(HGS_ERR_DEVICE, "hgs_copy_phase: source stream sync failed");
        for (int b = 0; b < B; ++b) {
            const char* from = (const char*)src.ptr + (src.B == 1 ? 0 : (size_t)b * S * sizeof(R));
            if (src.device == cfg.device) HIPCHK(hipMemcpyAsync(phase + (size_t)b * S, from, S * sizeof(R), hipMemcpyDeviceToDevice, stream));
            else HIPCHK(hipMemcpyPeerAsync(phase + (size_t)b * S, cfg.device, from, src.device, S * sizeof(R), stream));
        }
        HIPCHK(hipStreamSynchronize(stream));
        state.nearfield_input_changed();
        return 0;
    }

    int normalize_weights_now() {
        // fold the pending 1/||w|| into the stored weights (general path keeps them normalised)
        if (!state.w_pending()) return 0;
        hipLaunchKernelGGL(scale_weights_kernel<R>, dim3(ew_blocks, B), dim3(256), 0, stream, w.get(), (const R*)wscale, P);
        HIPCHK(hipGetLastError());
        if (int e = fill_wscale_one()) return e;
        state.scale_folded();
        return 0;
    }
    int get_array(int which, void* dst, size_t nbytes, bool dst_device) override {
        if (!dst) return fail(HGS_ERR_ARG, "null destination pointer");
        switch (which) {
            case HGS_PHASE:
                if (nbytes != S * sizeof(R) * B) return fail(HGS_ERR_ARG, "phase: bad size %zu", nbytes);
                return d2h(dst, phase, nbytes, dst_device);
            case HGS_PHASE_PREV:
                if (!phase_prev || !state.have_prev()) return fail(HGS_ERR_STATE, "no previous phase is held (HGS_OPT_KEEP_PREV_PHASE, one-iteration fused calls)");
                if (nbytes != S * sizeof(R) * B) return fail(HGS_ERR_ARG, "previous phase: bad size %zu", nbytes);
                return d2h(dst, phase_prev, nbytes, dst_device);
            case HGS_CG_GRAD:
                if (!cg_grad || !state.cg_have_grad()) return fail(HGS_ERR_STATE, "no gradient is held (hgs_cg_iterate with keep_grad has not run)");
                if (nbytes != S * sizeof(R)) return fail(HGS_ERR_ARG, "gradient: bad size %zu", nbytes);
                return d2h(dst, cg_grad, nbytes, dst_device);
            case HGS_VORTICES:
                if (vx_n < 0) return fail(HGS_ERR_STATE, "no vortex list is held (hgs_remove_vortices has not run)");
                if (nbytes != (size_t)vx_n * 3 * sizeof(int32_t)) return fail(HGS_ERR_ARG, "vortices: bad size %zu (the last call found %d)", nbytes, vx_n);
                if (vx_n == 0) return 0;
                return d2h(dst, vx_list, nbytes, dst_device);
            case HGS_TARGET: return download_T<R>(t.get(), dst, nbytes, dst_device, nullptr);
            case HGS_WEIGHTS: return download_T<R>(w.get(), dst, nbytes, dst_device, state.w_pending() ? wscale.get() : nullptr);
            case HGS_PHASE_FF:
                if (!pff || !state.have_pff()) return fail(HGS_ERR_STATE, "phase_ff has not been computed");
                return download_T<R>(pff.get(), dst, nbytes, dst_device, nullptr);
            case HGS_FARFIELD:
                if (!ff || !state.farfield_valid()) return fail(HGS_ERR_STATE, "farfield is not materialised (call hgs_nearfield2farfield)");
                return download_T<C>(ff.get(), dst, nbytes, dst_device, nullptr);
            case HGS_AMP_FF:
                if (!aff || !state.farfield_valid()) return fail(HGS_ERR_STATE, "amp_ff is not materialised (call hgs_nearfield2farfield)");
                return download_T<R>(aff.get(), dst, nbytes, dst_device, nullptr);
            case HGS_ZERO_WEIGHTS:
                if (!zw) return fail(HGS_ERR_STATE, "zero_weights not allocated");
                return download_T<C>(zw.get(), dst, nbytes, dst_device, nullptr);
        }
        return fail(HGS_ERR_ARG, "array selector %d cannot be read back", which);
    }

    int reset_weights() override {
        state.weights_write_begins();
        hipLaunchKernelGGL(reset_weights_kernel<R>, dim3(ew_blocks * B), dim3(256), 0, stream, w.get(), (const R*)t, zw.get(), B * P);
        HIPCHK(hipGetLastError());
        return weights_written();
    }
    // Hologram.reset (:442-478): weights from the target, phase_ff / farfield / amp_ff back to "None"
    int reset_state() override {
        state.reset_state();
        cg_t = 0;               // Adam starts over (hgs_cg_iterate zeroes the moments at step 0)
        return reset_weights();
    }
    // n values at listed pixels, `0` everywhere else (SpotHologram targets: n_spots numbers instead of P)
    int set_array_sparse(int which, const int32_t* xy, const void* values, int n) override {
        if (cfg.kind != 0) return fail(HGS_ERR_UNSUPPORTED, "sparse uploads are for the padded-grid holograms");
        if (which != HGS_TARGET && which != HGS_WEIGHTS) return fail(HGS_ERR_ARG, "sparse upload: HGS_TARGET or HGS_WEIGHTS only");
        if (n < 0 || (n > 0 && (!xy || !values))) return fail(HGS_ERR_ARG, "sparse upload: null list");
        // duplicates: the last entry wins (NumPy fancy assignment); resolved here so that the scatter is order-free
        std::vector<uint32_t> pos;
        std::vector<R> val;
        pos.reserve(n); val.reserve(n);
        {
            std::vector<std::pair<uint32_t, int>> key(n);
            for (int k = 0; k < n; ++k) {
                const int x = xy[k], y = xy[n + k];
                if (x < 0 || x >= g.Pw || y < 0 || y >= g.Ph) return fail(HGS_ERR_ARG, "sparse upload: pixel %d outside the grid", k);
                const int yd = col_pos(y, g.lane_T);
                key[k] = {(uint32_t)((size_t)x * g.Ph + yd), k};
            }
            std::stable_sort(key.begin(), key.end(), [](const std::pair<uint32_t, int>& a, const std::pair<uint32_t, int>& b) { return a.first < b.first; });
            for (int k = 0; k < n; ++k)
                if (k + 1 == n || key[k + 1].first != key[k].first) {
                    pos.push_back(key[k].first);
                    val.push_back(static_cast<const R*>(values)[key[k].second]);
                }
        }
        R* dst = which == HGS_TARGET ? t : w;
        HIPCHK(hipMemsetAsync(dst, 0, (size_t)B * P * sizeof(R), stream));
        const int m = (int)pos.size();
        if (m > 0) {
            DevBuf<uint32_t> dpos;
            DevBuf<R> dval;
            HIPCHK(dpos.alloc((size_t)m));
            HIPCHK(dval.alloc((size_t)m));
            hipError_t e1 = hipMemcpyAsync(dpos, pos.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, stream);
            hipError_t e2 = hipMemcpyAsync(dval, val.data(), (size_t)m * sizeof(R), hipMemcpyHostToDevice, stream);
            if (e1 == hipSuccess && e2 == hipSuccess) {
                hipLaunchKernelGGL(scatter_values<R>, dim3((m + 255) / 256, B), dim3(256), 0, stream, dst, (const uint32_t*)dpos,
                                   (const R*)dval, m, P);
                e1 = hipGetLastError();
            }
            hipStreamSynchronize(stream);       // (pos / val and the two device lists go out of scope)
            if (e1 != hipSuccess || e2 != hipSuccess) return fail(HGS_ERR_DEVICE, "sparse upload failed");
        } else {
            HIPCHK(hipStreamSynchronize(stream));
        }
        if (which == HGS_TARGET) { has_target = true; state.target_written(); return 0; }
        return weights_written();
    }

    // ---- operator launches ----
    RowArgs<R> row_args(bool finalize, int n_wpartial = 0) {
        RowArgs<R> a{};
        a.g = g; a.phase = phase; a.amp = has_amp ? amp : nullptr; a.kern = has_kern ? kern : nullptr;
        a.amp_scalar = (R)amp_scalar; a.gh = gh; a.tw = tw_row; a.scale = (R)(1.0 / std::sqrt((double)g.Pw));
        a.wpartial = finalize ? wpartial : nullptr; a.n_wpartial = n_wpartial; a.wscale = wscale;
        a.xcd_map = row_xcd;
        a.n_row_blocks = row_blocks;
        {   // shifted form of the row kernel: fp32, one-row workgroups, the SLM columns within eight register slots
            const int T = g.Pw / 16;
            const int s0 = g.c0 / T, s1 = (g.c0 + g.Sw - 1) / T;
            a.shifted = ((sizeof(R) == 4 || tun.row_shift64) && g.Pw >= 4096 && s1 - s0 + 1 <= 8 && tun.row_shift) ? 1 : 0;
            a.m0 = s0;
        }
        return a;
    }
    // a row launch outside a loop body: nothing folded, every column read (store: as RowClose::store_sparse)
    static RowClose plain_row(int mode, int store_sparse = 0) {
        RowClose rc;
        rc.mode = mode; rc.store_sparse = store_sparse;
        return rc;
    }
    // rc: what the launch does (column_plan.hpp, plan_row_close)
    // cp: the column pass this launch closes (the partials it folds, the join of a single-pass MRAF body), or null
    int run_row(const RowClose& rc, const ColumnPlan* cp = nullptr) {
        state.row_launch_begins();
        int r_ = run_row_impl(rc, cp);
        // gh holds G of the columns this launch stored -- of none that a later call may count on where it stored zeros instead
        // (an error return in mid-loop must not leave a G behind that is none)
        if (r_ == 0) state.row_stored_g(rc.mode, rc.zero_par >= 0 ? -1 : rc.store_sparse);
        return r_;
    }
    // (fused loops only; p = the plan of the call's first iteration)
    int keep_prev_phase(const Plan& p, int n) {
        if (!opt_prev_phase) return 0;
        if (n != 1) { state.prev_phase_dropped(); return 0; }      // the phases in between are never materialised
        if (p.use_fixed) return 0;                          // phase_ff is not rewritten: what is held stays what describes it
        if (need_zeroed(phase_prev, (size_t)B * S)) return HGS_ERR_DEVICE;
        HIPCHK(hipMemcpyAsync(phase_prev, phase, (size_t)B * S * sizeof(R), hipMemcpyDeviceToDevice, stream));
        state.prev_phase_kept();
        return 0;
    }
    bool gh_holds(int need) const { return state.gh_holds(need, tun.keep_g != 0); }
    int run_row_impl(const RowClose& rc, const ColumnPlan* cp) {
        const int mode = rc.mode, zero_par = rc.zero_par;
        const bool finalize = rc.finalize;
        return timed(HGS_K_ROW, [&]() -> int {
            RowArgs<R> a = row_args(finalize, cp ? cp->wpartial_n : 0);
            // the partials of a launch that left them per half tile: the row-less block folds the hologram's WHOLE slot range
            if (rc.wslot_fold) { a.wpartial = wslots; a.n_wpartial = tile2_wslots(g.Pw); a.wslot_fold = 1; }
            a.load_mask = rc.load_sparse == 1 ? active.mask.get() : rc.load_sparse == 2 ? dilated.mask.get() : nullptr;
            a.store_mask = rc.store_sparse == 1 ? active.mask.get() : rc.store_sparse == 2 ? dilated.mask.get() : nullptr;
            if (zero_par >= 0) {
                if (sizeof(R) != 4 || mode != 2 || a.load_mask || a.store_mask || (cp && cp->join != RowJoin::none))
                    return fail(HGS_ERR_STATE, "zero-masked row launch outside a plain fp32 MODE 2 launch");
                // bit 0 of the scan, per lane and register slot.  The mask of the active-column list IS that: it is built
                // from "any bit of the scan byte" (ColList::build with 0xff), the scan sets bit 1 (a finite non-zero target)
                // and bit 2 (a NaN target) only where it sets bit 0 (either is a target that is not zero), and the rounding
                // to whole tiles ORs bit 0 itself into the bytes of a tile -- so a byte is non-zero exactly when bit 0 is set.
                // Built once per scan, next to the other masks (refresh_sparse).
                a.zero_mask = active.mask.get();
                a.zero_par = zero_par;
            }
            // one extra (row-less) block folds the weight-norm partials when asked to
            // dense fp32 launches between iterations at 4096: workgroups walk several rows, next row prefetched into LDS
            int blocks = row_blocks;
            // (measured, tools/row_tail_probe.py: it pays where a one-row-per-workgroup launch ends in a partial round that the
            //  walk turns into a third row for a quarter to a half of the workgroups -- 1152 rows 28.1 -> 26.3 us, 1280 rows
            //  29.1 -> 27.5 us, 1040 / 1088 / 1200 / 1248 rows 1.0 - 1.7 us ahead; level at 1024 rows, behind at 1312 and 1536)
            if (sizeof(R) == 4 && g.Pw == 4096 && mode == 2 && tun.row_pref && row_blocks_pref > 0 && !a.load_mask && !a.store_mask &&
                (B == 1 ? (g.Sh > 2 * row_blocks_pref && 2 * g.Sh <= 5 * row_blocks_pref) : g.Sh >= 4 * row_blocks_pref)) {
                a.prefetch = 1;
                a.n_row_blocks = blocks = row_blocks_pref;
            }
            if (cp && cp->join != RowJoin::none) {          // single-pass MRAF: H = gh * wscale + gh2 (wscale final: scale_from_sum ran)
                a.prefetch = 0;
                a.n_row_blocks = blocks = row_blocks;
                a.gh2 = gh2;
                a.gh2_mask = cp->gh2_mask ? lane_mask_noise.get() : nullptr;
                LCHK(launch_row_split(g.Pw, mode, dim3(blocks, B), stream, a));
                return 0;
            }
            LCHK(launch_row<R>(g.Pw, mode, dim3(blocks + (finalize ? 1 : 0), B), stream, a));
            return 0;
        });
    }
    // active columns dilated by the offsets [lo, hi] of the spot integration window
    int refresh_dilated(int lo, int hi) {
        if (state.dilation_is(lo, hi)) return 0;
        state.dilation_rebuild_begins();
        HIPCHK(col_active_d.ensure((size_t)B * g.Pw));
        hipLaunchKernelGGL(dilate_active_cols, dim3((g.Pw + 255) / 256, B), dim3(256), 0, stream,
                           (const unsigned char*)col_active, g.Pw, lo, hi, col_active_d.get());
        HIPCHK(hipGetLastError());
        if (int e = dilated.build(col_active_d, 0xff, B, g.Pw, stream)) return e;
        state.dilation_rebuilt(lo, hi);
        return 0;
    }
    // what plan_column_pass() reads, as far as it does not depend on the iteration: geometry, switches, the last column scan
    PassFacts base_facts() const {
        PassFacts f;
        f.elem = (int)sizeof(R);
        f.Ph = g.Ph; f.Pw = g.Pw; f.B = B; f.n_cu = n_cu; f.col_blocks = col_blocks; f.tile_blocks = tile_blocks; f.r0 = g.r0; f.Sh = g.Sh;
        f.stat_groups = stat_ctx ? stat_ctx->groups : 0;
        f.w_unit = state.w_unit();
        f.sparse_tiles = sparse_tiles; f.sparse_dirty = state.sparse_dirty(); f.w_outside_scan = state.w_outside_scan();
        f.n_active_min = active.n_min; f.n_active_max = active.n_max; f.n_noise_max = noise.n_max; f.n_signal_max = signal.n_max;
        f.tun = tun;
        return f;
    }
    bool tile_geometry_ok() const { return hgs::tile_geometry_ok(base_facts()); }
    // the weight-norm slots, every one +0: when they are made and with every column scan (see the buffer's declaration)
    int clear_wslots() {
        const size_t n = (size_t)B * tile2_wslots(g.Pw);
        if (!wslots) { HIPCHK(wslots.alloc_zeroed(n, stream)); return 0; }
        HIPCHK(hipMemsetAsync(wslots.get(), 0, n * sizeof(double), stream));
        return 0;
    }
    // (re)build the active-column list when weights or target changed since the last scan
    int refresh_sparse() {
        if (!state.sparse_dirty()) return 0;
        state.scan_started();
        HIPCHK(col_active.ensure((size_t)B * g.Pw));
        HIPCHK(sig_rows.ensure((size_t)B * g.Pw));
        hipLaunchKernelGGL(scan_active_cols<R>, dim3(g.Pw, B), dim3(256), 0, stream, (const R*)w, (const R*)t, g.Ph, g.Pw,
                           col_active.get(), g.lane_T > 0 ? sig_rows.get() : (unsigned short*)nullptr);
        HIPCHK(hipGetLastError());
        // Where the tile-resident kernel can run the column pass and the active columns fill their 4-column tiles at least
        // half (images, MRAF noise boxes -- not spot arrays, whose columns sit alone in their tiles), the active set is
        // rounded to whole tiles and that kernel walks the tile list: 45 ns per column against 80 for the per-column
        // kernel at 8192 points, and the row kernel moves whole 32-byte tile rows.
        sparse_tiles = false;
        if (tile_geometry_ok() && tun.tile_list) {
            std::vector<unsigned char> act((size_t)B * g.Pw);
            if (int e = d2h(act.data(), col_active, act.size())) return e;
            bool dense = true;
            for (int b = 0; b < B && dense; ++b) {
                int n_col = 0, n_tile = 0;
                for (int c = 0; c < g.Pw; c += 4) {
                    const unsigned char* q = act.data() + (size_t)b * g.Pw + c;
                    const int k = (q[0] != 0) + (q[1] != 0) + (q[2] != 0) + (q[3] != 0);
                    n_col += k;
                    n_tile += k > 0;
                }
                dense = n_col > 0 && n_col >= 2 * n_tile;
            }
            if (dense) {
                for (size_t c = 0; c < act.size(); c += 4) {
                    const unsigned char on = (act[c] | act[c + 1] | act[c + 2] | act[c + 3]) ? 1 : 0;
                    for (int k = 0; k < 4; ++k) act[c + k] |= on;          // (bits 1, 2 of scan_active_cols stay per column)
                }
                if (int e = h2d(col_active, act.data(), act.size())) return e;
                sparse_tiles = true;
            }
        }
        if (int e = active.build(col_active, 0xff, B, g.Pw, stream)) return e;
        // the flag-reading instances of the half-width kernel (fp32, 4096 rows): the list of tiles that hold anything, on the
        // device and without a synchronisation of its own; the weight-norm slots of what the old scan called non-empty go back to +0
        if (sizeof(R) == 4 && g.Ph == 4096) {
            HIPCHK(tile_list.ensure((size_t)B * (g.Pw / 4)));
            HIPCHK(tile_list_n.ensure((size_t)B));
            hipLaunchKernelGGL(compact_active_tiles, dim3(B), dim3(256), 0, stream, (const unsigned char*)col_active, g.Pw,
                               tile_list.get(), tile_list_n.get());
            HIPCHK(hipGetLastError());
            if (int e = clear_wslots()) return e;
        }
        HIPCHK(lane_mask_noise.ensure((size_t)B * (g.Pw / 16)));
        hipLaunchKernelGGL(flag_lane_mask, dim3((g.Pw / 16 + 255) / 256, B), dim3(256), 0, stream, (const unsigned char*)col_active,
                           g.Pw, 4, lane_mask_noise.get());
        HIPCHK(hipGetLastError());
        state.scan_finished();
        return 0;
    }
    // the columns that hold a finite non-zero target as a list (the per-column pre-pass of the single-inverse MRAF update)
    int refresh_signal() {
        if (int e = refresh_sparse()) return e;
        if (state.signal_valid()) return 0;
        if (int e = signal.build(col_active, 2, B, g.Pw, stream)) return e;
        state.signal_list_rebuilt();
        return 0;
    }
    // per-column single-pass MRAF: the columns that hold a NaN target as a list (the buffer of the noise part is zeroed by the
    // caller once it decides for the single pass: its NaN-target pixels are rewritten by every pass, everything else must read
    // as zero, also after the target moved)
    int refresh_noise() {
        if (int e = refresh_sparse()) return e;
        if (state.noise_valid()) return 0;
        state.noise_list_rebuild_begins();
        if (int e = noise.build(col_active, 4, B, g.Pw, stream)) return e;
        state.noise_list_rebuilt();
        return 0;
    }
    ColArgs<R> col_args() {
        ColArgs<R> a{};
        a.g = g; a.gh = gh; a.ff = ff; a.amp_ff = aff; a.pff = pff; a.w = w; a.t = t; a.wscale = wscale;
        a.wpartial = wpartial; a.fpartial = fpartial; a.tw = tw_col; a.scale = (R)(1.0 / std::sqrt((double)g.Ph));
        a.col_xmap = col_xmap;
        // float64, 4096 / 8192 rows: col_fused_kernel in its shifted form (the SLM rows in the first fnr register slots)
        if (sizeof(R) == 8 && g.Ph >= 4096 && tun.fused_shift) {
            const int sh = (g.r0 / 16) * 16, Tc = g.Ph / 16, nr = (g.r0 - sh + g.Sh + Tc - 1) / Tc;
            if (nr <= 6) { a.fshift = sh; a.fnr = nr; }
        }
        return a;
    }
    int reduce(const double* partial, int n, double* out) {
        hipLaunchKernelGGL(reduce_partials, dim3(B), dim3(256), 0, stream, partial, n, out);
        HIPCHK(hipGetLastError());
        return 0;
    }

    int n2f(int store_pff) override {
        RoctxRange range(opt_roctx, "hgs_nearfield2farfield");
        if (cfg.kind == 1) return n2f_compressed(store_pff);
        if (general) return n2f_general(store_pff);
        if (int e = need_ff()) return e;
        if (store_pff) { if (int e = need_pff()) return e; }
        // (a fused loop that ended on its dense row launch left G of every column behind: the transform starts with its column pass)
        if (!gh_holds(0)) { if (int e = run_row(plain_row(0))) return e; }
        int r = timed(HGS_K_COL_FWD, [&]() -> int {
            ColArgs<R> a = col_args();
            a.store_pff = store_pff;
            LCHK(launch_col<R>(g.Ph, C_FWD | C_STORE, dim3(col_blocks, B), stream, a));
            return 0;
        });
        if (r) return r;
        if (int e = reduce(fpartial, col_blocks, sums + 0 * B)) return e;
        state.farfield_materialised(store_pff != 0);
        return 0;
    }

    int f2n() override {
        RoctxRange range(opt_roctx, "hgs_farfield2nearfield");
        if (cfg.kind == 1) return f2n_compressed();
        if (general) return f2n_general(false);
        if (!ff || !state.farfield_valid()) return fail(HGS_ERR_STATE, "no farfield to transform back");
        if (int e = inverse_columns()) return e;
        return run_row(plain_row(1));
    }
    // the column half of the inverse transform, every column: ff -> gh
    int inverse_columns() {
        int r = timed(HGS_K_COL_INV, [&]() -> int {
            state.column_pass_begins();
            LCHK(launch_col<R>(g.Ph, C_LOAD | C_INV, dim3(col_blocks, B), stream, col_args()));
            return 0;
        });
        if (r == 0) state.farfield_consumed();  // farfield now holds the constrained field, phase moves on
        return r;
    }

    // Hologram._farfield2nearfield(extract=False) (:1058-1073): the complex nearfield over the SLM,
    // kept on the device for MultiplaneHologram's weighted sum
    int f2n_complex() override {
        if (!ff || !state.farfield_valid()) return fail(HGS_ERR_STATE, "no farfield to transform back");
        if (need_zeroed(nfbuf, B * S)) return HGS_ERR_DEVICE;
        if (general) return f2n_general(true);
        if (cfg.kind == 1) return f2n_compressed(nfbuf);
        if (int e = inverse_columns()) return e;
        return timed(HGS_K_ROW, [&]() -> int {
            RowArgs<R> a = row_args(false);
            a.nf_out = nfbuf;
            LCHK(launch_row<R>(g.Pw, 1, dim3(row_blocks, B), stream, a));
            return 0;
        });
    }
    // n bodies of Hologram.optimize_cg (:1704-1735) with the default loss and Adam (include/hgs.h, cg_kernels.hpp).  Both
    // transforms are the engine's own, unchanged: n2f leaves F and sum |F|^2 on the device, the seed pass turns F into the
    // adjoint seed in place, f2n_complex brings it back over the SLM window, the Adam pass forms the gradient and moves
    // the phase.  Nothing is read by the host until the loop is over.
    int cg_iterate(const hgs_cg_params* p, int n, double* loss_out) override {
        RoctxRange range(opt_roctx, "hgs_cg_iterate");
        if (cfg.kind != 0) return fail(HGS_ERR_UNSUPPORTED, "hgs_cg_iterate: padded-grid holograms only (engine kind 0)");
        if (B != 1) return fail(HGS_ERR_UNSUPPORTED, "hgs_cg_iterate: one hologram per engine (batch is %d)", B);
        if (n < 0) return fail(HGS_ERR_ARG, "hgs_cg_iterate: n_iter must be >= 0");
        if (!(p->lr >= 0) || !std::isfinite(p->lr)) return fail(HGS_ERR_ARG, "Invalid learning rate: %g", p->lr);
        if (!(p->eps >= 0) || !std::isfinite(p->eps)) return fail(HGS_ERR_ARG, "Invalid epsilon value: %g", p->eps);
        if (!(p->beta1 >= 0 && p->beta1 < 1)) return fail(HGS_ERR_ARG, "Invalid beta parameter at index 0: %g", p->beta1);
        if (!(p->beta2 >= 0 && p->beta2 < 1)) return fail(HGS_ERR_ARG, "Invalid beta parameter at index 1: %g", p->beta2);
        if (!has_target) return fail(HGS_ERR_STATE, "target has not been set");
        // (each buffer on its own pointer: a call that failed half way allocates the rest next time.  The moments are
        //  zeroed by whoever starts Adam: a restart, or -- cg_t == 0 -- a first call and the first one after hgs_reset)
        if (!cg_m) { if (dalloc(cg_m, S)) return HGS_ERR_DEVICE; cg_t = 0; }
        if (!cg_v) { if (dalloc(cg_v, S)) return HGS_ERR_DEVICE; cg_t = 0; }
        if (need_zeroed(cg_partial, (size_t)ew_blocks)) return HGS_ERR_DEVICE;
        if (p->restart) cg_t = 0;
        if (cg_t == 0) {
            HIPCHK(hipMemsetAsync(cg_m, 0, S * sizeof(R), stream));
            HIPCHK(hipMemsetAsync(cg_v, 0, S * sizeof(R), stream));
        }
        if (p->keep_grad && !cg_grad) { if (dalloc(cg_grad, S)) return HGS_ERR_DEVICE; }
        if (n == 0) return 0;
        if (cg_loss_cap < n) {
            cg_loss_cap = 0;
            HIPCHK(cg_loss.release(stream));
            if (dalloc(cg_loss, (size_t)n)) return HGS_ERR_DEVICE;
            cg_loss_cap = n;
        }
        for (int it = 0; it < n; ++it) {
            if (int e = n2f(0)) return e;
            int r = timed(HGS_K_CG_SEED, [&]() -> int {
                CgSeedArgs<R> a{};
                a.ff = ff; a.t = t; a.fsum = sums + 0 * B; a.partial = cg_partial; a.P = P;
                LCHK(launch_cg_seed<R>(ew_blocks, stream, a));
                return reduce(cg_partial, ew_blocks, cg_loss + it);
            });
            if (r) return r;
            // (ff holds the seed now; the farfield stays valid for the inverse, which consumes it -- and drops G)
            if (int e = f2n_complex()) return e;
            ++cg_t;
            r = timed(HGS_K_CG_ADAM, [&]() -> int {
                CgAdamArgs<R> a{};
                a.g = nfbuf; a.phase = phase; a.amp = has_amp ? amp : nullptr; a.kern = has_kern ? kern : nullptr;
                a.m = cg_m; a.v = cg_v; a.grad = p->keep_grad ? cg_grad : nullptr;
                a.amp_scalar = (R)amp_scalar; a.beta1 = (R)p->beta1; a.beta2 = (R)p->beta2; a.eps = (R)p->eps;
                a.step_size = (R)(p->lr / (1.0 - std::pow(p->beta1, (double)cg_t)));
                a.inv_bc2_sqrt = (R)(1.0 / std::sqrt(1.0 - std::pow(p->beta2, (double)cg_t)));
                a.S = S;
                LCHK(launch_cg_adam<R>(stream, a));
                return 0;
            });
            if (r) return r;
            if (p->keep_grad) state.cg_gradient_stored();
        }
        state.prev_phase_dropped();      // (HGS_PHASE_PREV described the phase a fused body started from: it is no longer the previous one)
        if (loss_out) {
            if (int e = d2h(loss_out, cg_loss, (size_t)n * sizeof(double))) return e;
            for (int it = 0; it < n; ++it) loss_out[it] /= (double)P;      // mean reduction
        }
        return 0;
    }

    // Hologram._remove_vortices (:961-998) as its code intends: analysis.image_remove_vortices(phase_ff, target > 0) on the
    // stored farfield phase (vortex_kernels.hpp).  Search pass 0 counts, the scan leaves offsets and the total on the
    // device, the host reads the total once (it sizes the list and is the return value), pass 1 scatters, the removal
    // walks the list.  Nothing else of the engine's state is touched.
    int remove_vortices(int32_t* n_removed) override {
        RoctxRange range(opt_roctx, "hgs_remove_vortices");
        if (cfg.kind != 0) return fail(HGS_ERR_UNSUPPORTED, "hgs_remove_vortices: padded-grid holograms only (engine kind 0)");
        if (B != 1) return fail(HGS_ERR_UNSUPPORTED, "hgs_remove_vortices: one hologram per engine (batch is %d)", B);
        if (!pff || !state.have_pff()) return fail(HGS_ERR_STATE, "phase_ff has not been computed");
        if (!has_target) return fail(HGS_ERR_STATE, "target has not been set");
        const unsigned blocks = vortex_find_blocks(P);
        if (need_zeroed(vx_counts, (size_t)blocks)) return HGS_ERR_DEVICE;
        if (need_zeroed(vx_count, (size_t)1)) return HGS_ERR_DEVICE;
        vx_n = -1;
        VortexFindArgs<R> f{};
        f.pff = pff; f.t = t; f.counts = vx_counts; f.list = vx_list; f.cap = vx_cap; f.pass = 0; f.P = P;
        f.g = VxGeo{g.Ph, g.Pw, g.lane_T};
        int n = 0;
        int r = timed(HGS_K_ELEMENTWISE, [&]() -> int {
            LCHK(launch_vortex_find<R>(stream, f));
            LCHK(launch_vortex_scan(stream, vx_counts, blocks, vx_count));
            return 0;
        });
        if (r) return r;
        if (int e = d2h(&n, vx_count, sizeof(int32_t))) return e;
        if (n > 0) {
            if ((unsigned)n > vx_cap) {
                vx_cap = 0;
                HIPCHK(vx_list.release(stream));
                const size_t cap = std::max<size_t>(1024, (size_t)n + (size_t)n / 2);      // (a cleaned phase holds fewer the next time)
                if (dalloc(vx_list, 3 * cap)) return HGS_ERR_DEVICE;
                vx_cap = (unsigned)cap;
            }
            r = timed(HGS_K_ELEMENTWISE, [&]() -> int {
                f.list = vx_list; f.cap = vx_cap; f.pass = 1;
                LCHK(launch_vortex_find<R>(stream, f));
                VortexRemoveArgs<R> a{};
                a.pff = pff; a.list = vx_list; a.count = vx_count; a.P = P; a.g = f.g;
                LCHK(launch_vortex_remove<R>(stream, a));
                return 0;
            });
            if (r) return r;
        }
        vx_n = n;
        if (n_removed) *n_removed = n;
        return 0;
    }

    // SLM.set_phase(hologram) up to the hardware write, on the device (include/hgs.h, display_kernels.hpp): the range pass
    // leaves the extremes of the scaled phase per hologram, the convert pass applies the branch they select.  Reads the
    // phase, the kernel and the correction; writes nothing the loop knows of.
    int get_display(const hgs_display_params* p, void* dst, size_t nbytes, bool dst_device) override {
        RoctxRange range(opt_roctx, "hgs_get_display");
        if (!dst) return fail(HGS_ERR_ARG, "null destination pointer");
        if (p->bitdepth < 1 || p->bitdepth > 16) return fail(HGS_ERR_ARG, "hgs_get_display: bitdepth must be in 1..16 (got %d)", p->bitdepth);
        if (!(p->phase_scaling > 0) || !std::isfinite(p->phase_scaling))
            return fail(HGS_ERR_ARG, "hgs_get_display: phase_scaling must be positive and finite (got %g)", p->phase_scaling);
        const bool bits16 = p->bitdepth > 8;
        const size_t all = (size_t)B * S * (bits16 ? 2 : 1);
        if (nbytes != all) return fail(HGS_ERR_ARG, "hgs_get_display: bad size %zu (%zu expected: %d-bit levels)", nbytes, all, bits16 ? 16 : 8);
        DisplayArgs<R> a{};
        a.range_blocks = display_range_blocks(S);
        if (need(disp_partial, (size_t)2 * B * a.range_blocks)) return HGS_ERR_DEVICE;
        if (need(disp_out, (size_t)B * S * 2)) return HGS_ERR_DEVICE;      // (made once: room for 16-bit levels whatever this call asks for)
        // the reference's own expressions, in its order of evaluation, in double
        const double res = (double)(1 << p->bitdepth), s = p->phase_scaling;
        a.phase = phase;
        a.kern = p->include_propagation && has_kern ? kern.get() : nullptr;
        a.corr = p->phase_correct && has_disp_corr ? disp_corr.get() : nullptr;
        a.partial = disp_partial; a.out = disp_out.get(); a.S = S;
        a.unit = s == 1.0; a.fill = s > 1.0;
        a.f = a.unit ? -(res / 2 / M_PI) : -(res * s / 2 / M_PI);
        a.res = res; a.period = res * s; a.lift = res * (1 - s);
        int r = timed(HGS_K_ELEMENTWISE, [&]() -> int {
            LCHK(launch_display_range<R>(B, stream, a));
            LCHK(launch_display<R>(B, bits16, stream, a));
            return 0;
        });
        if (r) return r;
        return d2h(dst, disp_out, all, dst_device);
    }

    // one SLM-sized mask rastered into the kernel, the phase or the display correction, on the device: run(dst, out_bytes)
    // launches and completes it
    static bool raster_target(int which) { return which == HGS_PROP_KERNEL || which == HGS_PHASE || which == HGS_DISPLAY_CORRECTION; }
    template <typename Run> int raster_into(const char* fn, int which, int h, int w, Run&& run) {
        if (h != cfg.slm_h || w != cfg.slm_w)
            return fail(HGS_ERR_ARG, "%s: mask of shape (%d, %d) is not of the SLM shape (%d, %d)", fn, h, w, cfg.slm_h, cfg.slm_w);
        if (which == HGS_DISPLAY_CORRECTION) {               // not a nearfield input: the loop never sees it
            HIPCHK(disp_corr.ensure(S));
            has_disp_corr = false;
            if (int e_ = run(disp_corr.get(), (int)sizeof(double))) return e_;
            has_disp_corr = true;
            return 0;
        }
        state.nearfield_upload_begins();
        if (which == HGS_PROP_KERNEL) {
            HIPCHK(kern.ensure(S));
            if (int e_ = run(kern.get(), (int)sizeof(R))) return e_;
            has_kern = true;
        } else {
            if (int e_ = run(phase.get(), (int)sizeof(R))) return e_;
            for (int b = 1; b < B; ++b)
                HIPCHK(hipMemcpyAsync(phase + (size_t)b * S, phase.get(), S * sizeof(R), hipMemcpyDeviceToDevice, stream));
            HIPCHK(hipStreamSynchronize(stream));
        }
        state.nearfield_input_changed();
        return 0;
    }

    // hgs_set_array_poly: one polynomial mask
    int set_array_poly(int which, const hgs_poly_params* p) override {
        RoctxRange range(opt_roctx, "hgs_set_array_poly");
        if (!raster_target(which))
            return fail(HGS_ERR_ARG, "hgs_set_array_poly fills HGS_PROP_KERNEL, HGS_PHASE or HGS_DISPLAY_CORRECTION (got selector %d)", which);
        if (int e_ = poly_check(p)) return e_;
        if (p->n != 1) return fail(HGS_ERR_ARG, "hgs_set_array_poly: one mask expected (n = %d)", p->n);
        return raster_into("hgs_set_array_poly", which, p->h, p->w, [&](void* dst, int out_bytes) -> int {
            return poly_run(p, dst, out_bytes, stream, [&](auto&& launch) -> int { return timed(HGS_K_ELEMENTWISE, launch); });
        });
    }

    // hgs_set_array_pattern: one grating, axicon or Gaussian-mode mask
    int set_array_pattern(int which, const hgs_pattern_params* p) override {
        RoctxRange range(opt_roctx, "hgs_set_array_pattern");
        if (!raster_target(which))
            return fail(HGS_ERR_ARG, "hgs_set_array_pattern fills HGS_PROP_KERNEL, HGS_PHASE or HGS_DISPLAY_CORRECTION (got selector %d)", which);
        if (int e_ = pattern_check(p)) return e_;
        return raster_into("hgs_set_array_pattern", which, p->h, p->w, [&](void* dst, int out_bytes) -> int {
            return pattern_run(p, dst, out_bytes, stream, [&](auto&& launch) -> int { return timed(HGS_K_ELEMENTWISE, launch); });
        });
    }

    int mp_info(MpInfo* o) override {
        o->nf = nfbuf; o->kern = has_kern ? kern : nullptr; o->phase = phase; o->S = S; o->B = B;
        o->real_bytes = (int)sizeof(R); o->device = cfg.device; o->stream = stream;
        return 0;
    }
    int mp_combine(const MpInfo* infos, const double* weights, int n) override {
        MpArgs<R> a{};
        a.n = n; a.S = S; a.total = (size_t)B * S;
        for (int k = 0; k < n; ++k) {
            a.nf[k] = static_cast<const C*>(infos[k].nf);
            a.kern[k] = static_cast<const R*>(infos[k].kern);
            a.phase[k] = static_cast<R*>(infos[k].phase);
            a.w[k] = (R)weights[k];
        }
        hipLaunchKernelGGL(multiplane_combine<R>, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, stream, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }

    // flag evolution of _gs_farfield_routines (:1552-1585); returns what this iteration must do
    Plan plan_iteration(hgs_step* st, uint8_t* hist_slot) {
        Plan p{0, 0, 0};
        // _update_stats ran before the routines: the history sees the flag as it is now (:1479)
        if (hist_slot) *hist_slot = st->fixed_phase ? 1 : 0;
        if (st->false_run >= 0) st->false_run = st->fixed_phase ? 0 : st->false_run + 1;
        const bool wgs = st->method != HGS_GS;
        if (wgs && st->iter > 0) {
            p.do_update = 1;
            if (st->method == HGS_WGS_KIM) {
                const bool was_not_fixed = !st->fixed_phase;
                if (was_not_fixed && st->iter >= st->fix_phase_iteration - 1 &&
                    st->false_run >= st->fix_phase_iteration)
                    st->fixed_phase = 1;
                if ((st->fixed_phase && !state.have_pff()) || was_not_fixed) p.store_phase = 1;
            } else {
                st->fixed_phase = 0;
            }
        }
        // :1601  "if not fixed or phase_ff is None: phase_ff = atan2(F)".  A phase stored in this very
        // iteration equals atan2(F), so "store + rebuild from F" is the same thing as using it.
        if (st->fixed_phase && !state.have_pff()) p.store_phase = 1;
        p.use_fixed = (st->fixed_phase && state.have_pff() && !p.store_phase) ? 1 : 0;
        return p;
    }

    // WGS-Kim fixed by efficiency (_hologram.py:1560-1569).  In the reference the flag is raised inside the
    // routines of the iteration whose recorded efficiency exceeds the threshold; that iteration still takes its
    // phase from the current farfield and stores it (was_not_fixed, :1582), so raising the flag right AFTER the
    // iteration is the same thing -- and the statistics the fused pass accumulates are available by then.
    static bool eff_gate_set(const hgs_step* st) {
        return st->method == HGS_WGS_KIM && st->fix_phase_efficiency == st->fix_phase_efficiency;
    }
    // the efficiency recorded for the iteration that just ran (st->iter not yet advanced); eff_host: value already on
    // the host (general path) or null to read slot `dev` on the device
    int eff_gate_after(hgs_step* st, const double* eff_host, const double* dev) {
        if (!eff_gate_set(st) || st->fixed_phase || st->iter <= 0) return 0;
        double eff = 0;
        if (eff_host) eff = *eff_host;
        else {
            if (int e = d2h(&eff, dev, sizeof(double))) return e;
        }
        if (eff > st->fix_phase_efficiency) st->fixed_phase = 1;
        return 0;
    }
    int eff_gate_check(const hgs_step* st, int groups) {
        if (!eff_gate_set(st)) return 0;
        if (st->efficiency_group < 0 || st->efficiency_group > 1 || !(groups & (1 << st->efficiency_group)))
            return fail(HGS_ERR_ARG, "Must track statistics to fix phase based on efficiency!");
        if (B != 1) return fail(HGS_ERR_UNSUPPORTED, "fix_phase_efficiency needs one flag per hologram: batch must be 1");
        return 0;
    }

    CParams<R> cparams(const hgs_step* st, const Plan& p) {
        CParams<R> c{};
        c.method = st->method; c.do_update = p.do_update; c.use_fixed = p.use_fixed; c.store_phase = p.store_phase;
        c.mraf = st->mraf_enabled; c.has_mraf_factor = st->has_mraf_factor; c.zero_mode = st->zero_mode;
        c.p_exp = (R)st->feedback_exponent; c.p_fac = (R)st->feedback_factor;
        c.mraf_factor = (R)st->mraf_factor; c.zero_factor = (R)st->zero_factor;
        c.inv_fnorm = (R)(1.0 / std::sqrt(amp_norm2));  // Parseval: ||F|| = ||nearfield|| = ||amp||
        c.log2_inv_fnorm = (R)(-0.5 * std::log2(amp_norm2));
        return c;
    }

    // spot integration windows of `width` pixels around (x[k], y[k]), floored: each must stay on the grid.  ixy: the floored
    // coordinates, x then y (may be null); msg: the caller's wording, with one %d for the spot
    template <typename T> int check_windows(const T* x, const T* y, int n, int width, int32_t* ixy, const char* msg) {
        const int flo = (int)std::floor(-(width - 1) / 2.0), fhi = flo + width - 1;
        for (int k = 0; k < n; ++k) {
            const int32_t xk = (int32_t)std::floor(x[k]), yk = (int32_t)std::floor(y[k]);
            if (ixy) { ixy[k] = xk; ixy[n + k] = yk; }
            if (xk + flo < 0 || yk + flo < 0 || xk + fhi >= g.Pw || yk + fhi >= g.Ph) return fail(HGS_ERR_ARG, msg, k);
        }
        return 0;
    }

    int check_step(const hgs_step* st) {
        if (st->method < HGS_GS || st->method > HGS_WGS_TANH) return fail(HGS_ERR_ARG, "unknown method %d", st->method);
        if (st->feedback < HGS_FB_PIXEL || st->feedback > HGS_FB_EXTERNAL) return fail(HGS_ERR_ARG, "unknown feedback %d", st->feedback);
        if (!has_target) return fail(HGS_ERR_STATE, "target has not been set");
        if (cfg.kind == 0 && st->feedback != HGS_FB_PIXEL && st->method != HGS_GS) {
            if (!has_spots) return fail(HGS_ERR_STATE, "spot feedback needs HGS_SPOT_INDEX / HGS_SPOT_AMP");
            if (st->feedback == HGS_FB_SPOT_WINDOW) {
                if (st->spot_window < 1) return fail(HGS_ERR_ARG, "spot_window must be >= 1");
                if (int e = check_windows(spot_xy_host.data(), spot_xy_host.data() + cfg.n_spots, cfg.n_spots, st->spot_window, nullptr,
                                          "integration window of spot %d leaves the grid (IndexError in the reference)")) return e;
            }
        }
        return 0;
    }

    // general constraint on the materialised farfield
    int constraint_planned(hgs_step* st, const Plan& p) {
        if (!ff || !state.farfield_valid()) return fail(HGS_ERR_STATE, "farfield is not materialised");
        if (int e = need_pff()) return e;
        if (int e = normalize_weights_now()) return e;
        if (p.do_update) state.general_rule_updated_weights();
        if (st->mraf_enabled && st->zero_mode) { if (int e = need_zw()) return e; }
        if (st->mraf_enabled && st->fixed_phase && !state.have_pff() && !p.store_phase)
            return fail(HGS_ERR_STATE, "fixed_phase with MRAF needs a stored phase_ff (reference quirk A12)");
        CParams<R> cp = cparams(st, p);
        EwArgs<R> a{};
        a.P = P; a.batch = B; a.ff = ff; a.amp_ff = aff; a.pff = pff; a.w = w; a.t = t;
        a.fsum = sums + 0 * B; a.nogsum = sums + 1 * B; a.partial = epartial; a.wsum = nullptr; a.zero_weights = zw;
        a.cp = cp;
        const dim3 eg(ew_blocks, B), eb(256);
        return timed(HGS_K_ELEMENTWISE, [&]() -> int {
            bool pixel_update = false;
            if (p.do_update && cfg.kind == 1 && st->feedback == HGS_FB_EXTERNAL) {
                // CompressedSpotHologram "external_spot" (_spots.py:978-989): the N-vector rule with
                // external_spot_amp as the feedback amplitude
                hipLaunchKernelGGL(convert_d2r<R>, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream,
                                   (const double*)ext_amp, ext_r, (int)P, B);
                HIPCHK(hipGetLastError());
                hipLaunchKernelGGL(ew_sumsq<R>, eg, eb, 0, stream, (const R*)ext_r, P, epartial);
                HIPCHK(hipGetLastError());
                if (int e = reduce(epartial, ew_blocks, sums + 3 * B)) return e;
                a.amp_ff = ext_r;
                a.fsum = sums + 3 * B;
            }
            if (p.do_update) {
                if (st->feedback == HGS_FB_PIXEL || cfg.kind == 1) {
                    if (st->method == HGS_WGS_NOGRETTE) {
                        hipLaunchKernelGGL(ew_nogrette_sum<R>, eg, eb, 0, stream, a);
                        HIPCHK(hipGetLastError());
                        if (int e = reduce(epartial, ew_blocks, sums + 1 * B)) return e;
                    }
                    hipLaunchKernelGGL(ew_weight_update<R>, eg, eb, 0, stream, a);
                    HIPCHK(hipGetLastError());
                    if (int e = reduce(epartial, ew_blocks, sums + 2 * B)) return e;
                    pixel_update = true;
                } else {
                    SpotArgs<R> s{};
                    s.g = g; s.n_spots = cfg.n_spots; s.width = st->spot_window; s.feedback = st->feedback;
                    s.spot_xy = spot_xy; s.amp_ff = aff; s.ext_amp = ext_amp; s.spot_amp = spot_amp; s.w = w;
                    s.fb = spot_fb; s.cp = cp;
                    if (st->feedback == HGS_FB_SPOT_WINDOW) {
                        hipLaunchKernelGGL(spot_window<R>, dim3((cfg.n_spots + 127) / 128, B), dim3(128), 0, stream, s);
                        HIPCHK(hipGetLastError());
                    }
                    hipLaunchKernelGGL(spot_update<R>, dim3(B), dim3(256), 0, stream, s);
                    HIPCHK(hipGetLastError());
                }
            }
            a.wsum = pixel_update ? sums + 2 * B : nullptr;
            // the rebuild recomputes and stores phase_ff whenever it is not "use_fixed"
            hipLaunchKernelGGL(ew_rebuild<R>, eg, eb, 0, stream, a);
            HIPCHK(hipGetLastError());
            state.phase_ff_stored();
            return 0;
        });
    }

    int constraint(hgs_step* st) override {
        RoctxRange range(opt_roctx, "hgs_farfield_constraint");
        if (int e = check_step(st)) return e;
        if (eff_gate_set(st) && st->iter > 0)     // the stepwise caller evaluates the gate itself (it holds the statistics)
            return fail(HGS_ERR_ARG, "Must track statistics to fix phase based on efficiency!");
        Plan p = plan_iteration(st, nullptr);
        return constraint_planned(st, p);
    }

    bool fused_ok(const hgs_step* st) const {
        // MRAF rides the fused kernels unless the zero region carries zero_weights feedback (:1613-1616)
        return cfg.kind == 0 && !general && !(st->mraf_enabled && st->zero_mode) && st->feedback == HGS_FB_PIXEL;
    }

    // ---- spot feedback on sparse targets ("computational_spot" / "external_spot", _spots.py:1573-1624) ----
    // The N-vector weight rule needs |F|^2 only in the w x w windows around the spots, so the forward
    // transform runs on the spot columns dilated by the window (col_kernel FWD|STORE over a list), the
    // existing window-sum / N-vector kernels update the weights at the spot pixels, and the constrained
    // field is formed and transformed back by the fused kernel over the spot columns (weight update
    // off).  Everything else of the farfield is exactly zero and is neither computed nor moved.
    bool spot_sparse_ok(const hgs_step* st) {
        if (cfg.kind != 0 || general || st->mraf_enabled || st->method == HGS_GS || st->feedback == HGS_FB_PIXEL) return false;
        if (!tun.sparse || opt_stepwise) return false;
        if (refresh_sparse()) return false;
        return active.n_min > 0 && active.n_max * 4 <= g.Pw;
    }
    // ---- executors of a ColumnPlan (column_plan.hpp: what is launched is decided there) ----
    PassFacts pass_facts(const hgs_step* st, const Plan& p, bool sparse_enabled) const {
        PassFacts f = base_facts();
        f.it = p;
        f.method = st->method; f.mraf_enabled = st->mraf_enabled; f.zero_mode = st->zero_mode;
        f.sparse_enabled = sparse_enabled;
        return f;
    }
    // amp_ff on the spot columns dilated by the integration window (col_kernel FWD|STORE over that list)
    int launch_dilated_forward() {
        return timed(HGS_K_COL_FWD, [&]() -> int {
            ColArgs<R> a = col_args();
            a.col_list = dilated.list;
            a.n_active = dilated.n_dev;
            LCHK(launch_col<R>(g.Ph, C_FWD | C_STORE, dim3(list_blocks(base_facts(), dilated.n_max), B), stream, a));
            return 0;
        });
    }
    // the buffers a plan lists; f / cp: re-planned once where the device cannot give the farfield buffer of the float64 split form
    int acquire(ColumnPlan& cp, PassFacts& f) {
        if (cp.need_ffb && !state.ffb_zeroed()) {
            if (ffb.ensure((size_t)B * g.Ph * g.Pw) != hipSuccess) {      // (tolerated: the two-pass form needs no such buffer)
                f.ffb_unavailable = true;
                cp = plan_column_pass(f);
            }
            if (cp.need_ffb) {
                HIPCHK(hipMemsetAsync(ffb, 0, (size_t)B * g.Ph * g.Pw * sizeof(C), stream));
                state.ffb_was_zeroed();
            }
        }
        // (dpartial: sized like wpartial)
        if (cp.need_dpartial) { if (int e = need_zeroed(dpartial, (size_t)B * std::max(std::max(col_blocks, tile_blocks), n_cu * 3))) return e; }
        if (cp.need_gh2) { if (int e = need_zeroed(gh2, (size_t)B * g.Sh * g.Pw)) return e; }
        if (cp.need_nog_dev) { if (int e = need_zeroed(nog_dev, (size_t)B)) return e; }
        return 0;
    }
    // the pre-pass of the single-inverse MRAF update (its own profile slot: a forward-only column launch)
    int launch_prepass(const ColumnPlan& cp, const CParams<R>& cprm) {
        if (!cp.presum && !cp.presum_col) return 0;
        return timed(HGS_K_COL_FWD, [&]() -> int {
            ColArgs<R> pa = col_args();
            pa.cp = cprm;
            pa.wpartial = dpartial;
            const dim3 grid(cp.prepass_grid, B);
            if (cp.presum_col) {             // per-column, over the signal columns
                pa.cp.weights_only = 1;
                pa.cp.presum = 1;
                pa.col_list = signal.list;
                pa.n_active = signal.n_dev;
                pa.list_xmap = cp.prepass_list_xmap;
                LCHK(launch_fused<R>(g.Ph, 0, grid, stream, pa));
            } else if constexpr (sizeof(R) == 4) {
                pa.col_flags = col_active;
                pa.sig_rows = (g.lane_T > 0 && tun.presum_rows) ? sig_rows : nullptr;
                LCHK(launch_presum(g.Ph, cp.prepass_nr, grid, stream, pa, cp.prepass_shift));
            }
            return 0;
        });
    }
    int launch_family(const ColLaunch& l, const ColArgs<R>& a) {
        const int N = g.Ph;
        const dim3 grid(l.grid, B);
        switch (l.family) {
            case ColFamily::fused: return launch_fused<R>(N, l.phase_mode, grid, stream, a);
            case ColFamily::fused_stats: return launch_fused_stats<R>(N, l.phase_mode, grid, stream, a);
            case ColFamily::tile: return launch_tile<R>(N, l.phase_mode, grid, stream, a, l.shift);
            case ColFamily::tile_stats: return launch_tile_stats<R>(N, l.phase_mode, grid, stream, a, l.shift);
            case ColFamily::tile_extras: return launch_tile_extras<R>(N, l.phase_mode, grid, stream, a, l.shift);
            case ColFamily::tile_extras_stats: return launch_tile_extras_stats<R>(N, l.phase_mode, grid, stream, a, l.shift);
            default:            // the float32-only families (the plan names none of them for 8-byte elements)
                if constexpr (sizeof(R) == 4) switch (l.family) {
                    case ColFamily::fused_rule1: return launch_fused_rule1(N, l.phase_mode, grid, stream, a);
                    case ColFamily::fused_rule2: return launch_fused_rule2(N, l.phase_mode, grid, stream, a);
                    case ColFamily::tile_rule: return launch_tile_rule(N, l.phase_mode, l.rule, l.nr, grid, stream, a, l.shift);
                    case ColFamily::tile_rule_listed: return launch_tile_rule_listed(N, l.phase_mode, l.rule, l.nr, grid, stream, a, l.shift);
                    case ColFamily::tile_split: return launch_tile_split(N, l.phase_mode, l.nr, l.rule_ok, grid, stream, a, l.shift);
                    case ColFamily::tile_split_stats: return launch_tile_split_stats(N, l.phase_mode, l.nr, l.rule_ok, grid, stream, a, l.shift);
                    case ColFamily::tile_presum: return launch_tile_presum(N, l.phase_mode, l.nr, grid, stream, a, l.shift);
                    case ColFamily::tile2: return launch_tile2(N, l.phase_mode, l.rule, l.nr, grid, stream, a, l.shift, l.half_xmap ? 1 : 0);
                    default: break;
                }
                return (int)hipErrorInvalidValue;
        }
    }
    // one launch of the column pass; then_scale: wscale = 1/||w'|| from its partials right after it (reduce_to_scale)
    int launch_column(const ColLaunch& l, const CParams<R>& cprm, bool then_scale = false) {
        return timed(HGS_K_COL_FUSED, [&]() -> int {
            ColArgs<R> a = col_args();
            a.cp = cprm;
            a.cp.do_update = l.do_update;
            a.cp.nog_pass = l.nog_pass ? 1 : 0;
            a.cp.weights_only = l.weights_only ? 1 : 0;
            if (l.use_nog) a.cp.nog = nog_dev;
            if (l.split64) { a.cp.split = 1; a.ffb = ffb; }
            if (l.n_dpartial) { a.dpartial = dpartial; a.n_dpartial = l.n_dpartial; }
            if (l.stats) {
                a.do_stats = l.stats;
                a.spartial = stat_partial;
                a.tsum = stat_tsum;
                a.inv_fsum = 1.0 / amp_norm2;
                // launches of different geometry share the partial buffer: reset the slots
                hipLaunchKernelGGL(stat_fill_neutral, dim3((unsigned)((stat_nslots + 255) / 256)), dim3(256), 0, stream,
                                   stat_partial, stat_nslots);
            }
            if (l.listed) { a.col_list = active.list; a.n_active = active.n_dev; }
            a.list_xmap = l.list_xmap ? 1 : 0;
            if (l.col_flags) a.col_flags = col_active;
            a.zero_inv = l.empty.skip_inverse ? 1 : 0;
            a.zero_fwd = l.empty.skip_forward ? 1 : 0;
            a.h_prezeroed = l.empty.prezeroed ? 1 : 0;
            if (l.empty.list_walk && tile_list && tile_list_n) { a.tile_list = tile_list; a.tile_list_n = tile_list_n; }
            // weight-norm partials per half tile instead of per workgroup; the row launch behind it folds them (run_row_impl)
            if (l.wslots) {
                if (then_scale) return fail(HGS_ERR_STATE, "weight-norm slots ahead of a per-workgroup reduction");
                if (!wslots) { if (int e = clear_wslots()) return e; }
                a.wslots = wslots;
            }
            a.few_active = l.few_active ? 1 : 0;
            if (l.family == ColFamily::tile_split || l.family == ColFamily::tile_split_stats) { a.gh2 = gh2; a.gh2_sparse = l.gh2_sparse ? 1 : 0; }
            LCHK(launch_family(l, a));
            if (l.nog_pass) {
                if (int e = reduce(wpartial, l.grid, sums + 1 * B)) return e;
                hipLaunchKernelGGL(nog_finalize<R>, dim3((B + 63) / 64), dim3(64), 0, stream, (const double*)(sums + 1 * B),
                                   l.listed ? (const int*)active.n_dev : (const int*)nullptr, g.Ph, g.Pw, nog_dev, B);
                HIPCHK(hipGetLastError());
            }
            if (then_scale) {
                hipLaunchKernelGGL(reduce_to_scale<R>, dim3(B), dim3(256), 0, stream, (const double*)wpartial, l.grid,
                                   sums + 2 * B, wscale);
                HIPCHK(hipGetLastError());
            }
            return 0;
        });
    }
    // float64 split: the noise part, farfield values -> gh2, noise columns only (own profile slot)
    int launch_noise_inverse(const ColumnPlan& cp) {
        if (!cp.noise_inverse_grid) return 0;
        return timed(HGS_K_COL_INV, [&]() -> int {
            ColArgs<R> nb = col_args();
            nb.ff = ffb;
            nb.gh = gh2;
            nb.col_list = noise.list;
            nb.n_active = noise.n_dev;
            LCHK(launch_col<R>(g.Ph, C_LOAD | C_INV, dim3(cp.noise_inverse_grid, B), stream, nb));
            return 0;
        });
    }

    int iterate_spot_sparse(hgs_step* st, int n, uint8_t* hist) {
        if (int e = normalize_weights_now()) return e;      // the N-vector rule keeps the weights normalised
        if (int e = need_ff()) return e;
        const int groups = stat_ctx ? stat_ctx->groups : 0;
        auto window = [](int w, int* lo, int* hi) { *lo = (int)std::floor(-(w - 1) / 2.0); *hi = *lo + w - 1; };
        int lo = 0, hi = 0, l2, h2;
        if (st->feedback == HGS_FB_SPOT_WINDOW) window(st->spot_window, &lo, &hi);
        // the statistics windows sit at floor(spot_knm) (analysis.take, quirk A18), the weights at rint(spot_knm):
        // one more column to the left
        if (groups & 2) { window(stat_ctx->width, &l2, &h2); lo = std::min(lo, l2 - 1); hi = std::max(hi, h2); }
        if (int e = refresh_dilated(lo, hi)) return e;
        auto windows_needed = [&](const Plan& q) {
            return (st->feedback == HGS_FB_SPOT_WINDOW && q.do_update) || (groups & 2);
        };
        state.spot_sparse_call_begins();
        Plan p = plan_iteration(st, hist ? hist : nullptr);
        if (int e = keep_prev_phase(p, n)) return e;
        if (!gh_holds(windows_needed(p) ? 2 : 1)) { if (int e = run_row(plain_row(0, windows_needed(p) ? 2 : 1))) return e; }
        for (int i = 0; i < n; ++i) {
            state.column_pass_begins();
            if (p.use_fixed || p.store_phase) { if (int e = need_pff()) return e; }
            const CParams<R> cprm = cparams(st, p);
            if (windows_needed(p)) { if (int e = launch_dilated_forward()) return e; }
            if (p.do_update) {
                int r = timed(HGS_K_ELEMENTWISE, [&]() -> int {
                    SpotArgs<R> sa{};
                    sa.g = g; sa.n_spots = cfg.n_spots; sa.width = st->spot_window; sa.feedback = st->feedback;
                    sa.spot_xy = spot_xy; sa.amp_ff = aff; sa.ext_amp = ext_amp; sa.spot_amp = spot_amp; sa.w = w;
                    sa.fb = spot_fb; sa.cp = cprm;
                    sa.inline_window = 1;
                    hipLaunchKernelGGL(spot_update<R>, dim3(B), dim3(256), 0, stream, sa);
                    HIPCHK(hipGetLastError());
                    return 0;
                });
                if (r) return r;
            }
            const ColumnPlan cp = plan_spot_sparse_pass(pass_facts(st, p, true));      // (the weights were updated above)
            if (int e = launch_column(cp.main, cprm)) return e;
            if (stat_ctx) { if (int e = fused_stats_finish(i, cp)) return e; }
            if (p.store_phase) state.phase_ff_stored();
            if (stat_ctx) { if (int e = eff_gate_after(st, nullptr, stat_ctx->dev_out + ((size_t)i * 2 + st->efficiency_group) * B * 4)) return e; }
            st->iter++;
            Plan pn{0, 0, 0};
            int store_next = 1;
            if (i + 1 < n) {
                pn = plan_iteration(st, hist ? hist + i + 1 : nullptr);
                store_next = windows_needed(pn) ? 2 : 1;
            }
            const bool last = i + 1 == n;
            RowClose rc = plain_row(last ? cp.last_mode : 2, (last && cp.last_mode == 3) ? 0 : store_next);
            rc.load_sparse = 1;
            if (int e = run_row(rc, &cp)) return e;
            p = pn;
        }
        return 0;
    }

    int iterate(hgs_step* st, int n, uint8_t* hist) override {
        RoctxRange range(opt_roctx, "hgs_iterate");
        if (n < 0) return fail(HGS_ERR_ARG, "n_iter must be >= 0");
        if (n == 0) return 0;
        if (int e = check_step(st)) return e;
        // the reference raises as soon as an iteration with iter > 0 consults statistics that were never tracked
        if (!stat_ctx && eff_gate_set(st) && (st->iter > 0 || n > 1))
            return fail(HGS_ERR_ARG, "Must track statistics to fix phase based on efficiency!");
        const bool fused = fused_ok(st) && !opt_stepwise;
        if (!fused && spot_sparse_ok(st)) return iterate_spot_sparse(st, n, hist);
        if (!fused) {
            state.prev_phase_dropped();           // the general operators keep HGS_PHASE_FF itself up to date
            for (int i = 0; i < n; ++i) {
                if (int e = n2f(0)) return e;
                Plan p = plan_iteration(st, hist ? hist + i : nullptr);
                if (int e = constraint_planned(st, p)) return e;
                if (int e = f2n()) return e;
                st->iter++;
            }
            return 0;
        }
        state.fused_call_begins();
        // Sparse targets: when few columns hold a non-zero weight/target, only those columns are
        // transformed (col_fused_kernel with a column list) and only they cross HBM between the two
        // kernels.  phase_ff (WGS-Kim) is then stored on the active columns only: nothing else can be
        // read back by the loop.
        bool sp = false;
        if (tun.sparse) {
            if (int e = refresh_sparse()) return e;
            sp = active.n_min > 0 && active.n_max * 2 <= g.Pw;
        } else if (st->mraf_enabled && st->method != HGS_GS && tun.mraf_split && tun.gh2_mask && tile_geometry_ok() && g.Pw >= 4096) {
            // single-pass MRAF: which columns hold a NaN target (the noise part exists only there) -- a fact about the
            // target, scanned once per upload; the dense launches themselves still walk every column
            if (int e = refresh_sparse()) return e;
        } else if (const DenseScan ds = dense_scan_needed(pass_facts(st, Plan{0, 0, 0}, false)); ds.scan) {
            // one scan launch and a device-to-host synchronisation per upload of weights or target, dense images included
            if (ds.rescan_outside) state.rescan_if_written_outside();
            if (int e = refresh_sparse()) return e;
        }
        // "computational_spot" statistics on the sparse path: amp_ff is produced on the spot columns dilated
        // by the integration window (col_kernel FWD|STORE over that list) before the fused kernel runs
        const bool spot_stats = stat_ctx && (stat_ctx->groups & 2);
        if (sp && spot_stats) {
            // windows sit at floor(spot_knm) (analysis.take, quirk A18), the weights at rint(spot_knm): one more
            // column to the left
            const int lo = (int)std::floor(-(stat_ctx->width - 1) / 2.0);
            if (int e = refresh_dilated(lo - 1, lo + stat_ctx->width - 1)) return e;
            if (int e = need_ff()) return e;
        }
        const int store_sparse = spot_stats ? 2 : 1;
        Plan p = plan_iteration(st, hist ? hist : nullptr);
        if (int e = keep_prev_phase(p, n)) return e;
        // (the previous call may have left G of these columns behind: gh_state, row_kernel MODE 3)
        if (!gh_holds(sp ? store_sparse : 0)) { if (int e = run_row(plain_row(0, sp ? store_sparse : 0))) return e; }
        // the row launch that closed the body before, in THIS call, stored zeros in the empty columns of gh (never kept across
        // calls: the last launch of a call leaves G of every column)
        bool gh_prezeroed = false;
        for (int i = 0; i < n; ++i) {
            state.column_pass_begins();
            if (p.use_fixed || p.store_phase) { if (int e = need_pff()) return e; }
            // facts -> plan: the column scans the form consults first (their counts feed the choice), then the plan itself
            PassFacts f = pass_facts(st, p, sp);
            const Scans scans = scans_needed(f);
            if (scans.noise) { if (int e = refresh_noise()) return e; }
            if (scans.signal) { if (int e = refresh_signal()) return e; }
            if (scans.flags) { if (int e = refresh_sparse()) return e; }         // (clean unless the weights / target moved)
            if (scans.noise || scans.signal || scans.flags) f = pass_facts(st, p, sp);
            // (flags cannot change inside a call; a body that scans them again takes the plain form, which writes the same zeros)
            f.gh_prezeroed = gh_prezeroed && !scans.flags;
            ColumnPlan cp = plan_column_pass(f);
            if (int e = acquire(cp, f)) return e;
            // the row launch before decided on the plan of THIS body (same pure function, same facts): where it stored zeros,
            // this launch must be the one that counts on them -- any other would read them as G
            if (f.gh_prezeroed && !cp.accepts_prezeroed) return fail(HGS_ERR_STATE, "zero-masked G ahead of a column pass that reads every column");
            // execute
            const CParams<R> cprm = cparams(st, p);
            if (cp.dilated_forward) { if (int e = launch_dilated_forward()) return e; }
            if (int e = launch_prepass(cp, cprm)) return e;
            if (cp.nog) { if (int e = launch_column(cp.nog_pass, cprm)) return e; }
            if (int e = launch_column(cp.main, cprm, cp.scale_after_main)) return e;
            if (cp.second_pass) { if (int e = launch_column(cp.second, cprm)) return e; }
            if (int e = launch_noise_inverse(cp)) return e;
            if (stat_ctx) { if (int e = fused_stats_finish(i, cp)) return e; }
            if (p.store_phase) state.phase_ff_stored();
            if (p.do_update) state.fused_update_done();
            if (stat_ctx) { if (int e = eff_gate_after(st, nullptr, stat_ctx->dev_out + ((size_t)i * 2 + st->efficiency_group) * B * 4)) return e; }
            st->iter++;
            Plan pn{0, 0, 0};
            if (i + 1 < n) pn = plan_iteration(st, hist ? hist + i + 1 : nullptr);
            // the row launch that closes the iteration (plan_row_close): on the sparse path it reads the active columns and writes
            // those the next column launches read; the last one of the call extracts the phase.  The next body's facts are those it
            // will form itself: nothing between here and there changes them.
            const bool last = i + 1 == n;
            const PassFacts fn = pass_facts(st, pn, sp);
            const RowClose rc = plan_row_close(cp, f, last ? nullptr : &fn);
            if (int e = run_row(rc, &cp)) return e;
            gh_prezeroed = rc.zero_par >= 0;
            p = pn;
        }
        return 0;
    }

    // ---- hgs_iterate_stats: the loop of optimize_gs with stat_groups (_hologram.py:1465-1490) -------------
    // Fused path: the column kernel accumulates the "computational" statistics of the field it
    // constrains (StatAcc) and, for the spot group, stores amp_ff for the window sums; one tiny
    // finalize launch per iteration; the host reads all n_iter results once at the end.
    int fused_stats_finish(int i, const ColumnPlan& cp) {
        StatCtx& c = *stat_ctx;
        const int nparts = cp.wpartial_n * STAT_WAVES;
        if (c.groups & 1) {
            hipLaunchKernelGGL(stat_finalize, dim3(B), dim3(256), 0, stream, (const double*)stat_partial, nparts,
                               (const double*)stat_tsum, 1.0 / amp_norm2, c.dev_out + ((size_t)i * 2 + 0) * B * 4);
            HIPCHK(hipGetLastError());
        }
        if (c.groups & 2) {
            SpotArgs<R> sa{};
            sa.g = g; sa.n_spots = cfg.n_spots; sa.width = c.width; sa.feedback = 1; sa.spot_xy = c.dxy; sa.amp_ff = aff;
            sa.fb = spot_fb;
            hipLaunchKernelGGL(spot_window<R>, dim3((cfg.n_spots + 127) / 128, B), dim3(128), 0, stream, sa);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(spot_stat_finalize<R>, dim3(B), dim3(256), 0, stream, (const R*)spot_fb,
                               (const double*)spot_amp, cfg.n_spots, amp_norm2, c.dev_out + ((size_t)i * 2 + 1) * B * 4);
            HIPCHK(hipGetLastError());
        }
        return 0;
    }

    int iterate_stats(hgs_step* st, int n, uint8_t* hist, int groups, int width, const double* xy,
                      double* out) override {
        if (n < 0) return fail(HGS_ERR_ARG, "n_iter must be >= 0");
        if (groups & ~3) return fail(HGS_ERR_ARG, "unknown statistics group mask %d", groups);
        if (groups == 0) return iterate(st, n, hist);
        if (!out) return fail(HGS_ERR_ARG, "statistics requested without an output buffer");
        if (n == 0) return 0;
        if (cfg.kind != 0) return fail(HGS_ERR_UNSUPPORTED, "hgs_iterate_stats is for the padded-grid holograms");
        if (int e = check_step(st)) return e;
        if (int e = eff_gate_check(st, groups)) return e;
        std::vector<int32_t> ixy;
        if (groups & 2) {
            if (cfg.n_spots <= 0 || !xy || !has_spots) return fail(HGS_ERR_STATE, "spot statistics need spots");
            const int N = cfg.n_spots;
            ixy.resize(2 * N);
            if (int e = check_windows(xy, xy + N, N, width, ixy.data(), "integration window of spot %d leaves the grid")) return e;
        }
        for (size_t k = 0; k < (size_t)n * 2 * B * 4; ++k) out[k] = NAN;
        const bool fused = (fused_ok(st) || spot_sparse_ok(st)) && !opt_stepwise;
        if (!fused) {
            state.prev_phase_dropped();
            // general path: materialise, reduce, constrain -- one host read of a few doubles per iteration
            for (int i = 0; i < n; ++i) {
                if (int e = n2f(0)) return e;
                if (groups & 1) { if (int e = stats(0, 1, nullptr, out + ((size_t)i * 2 + 0) * B * 4)) return e; }
                if (groups & 2) { if (int e = stats(1, width, xy, out + ((size_t)i * 2 + 1) * B * 4)) return e; }
                Plan p = plan_iteration(st, hist ? hist + i : nullptr);
                if (int e = constraint_planned(st, p)) return e;
                if (int e = f2n()) return e;
                if (int e = eff_gate_after(st, out + ((size_t)i * 2 + st->efficiency_group) * B * 4, nullptr)) return e;
                st->iter++;
            }
            return 0;
        }
        StatCtx c;
        c.groups = groups;
        c.width = width;
        const int max_blocks = std::max(std::max(tile_blocks, col_blocks), n_cu * 3);
        const size_t nslots = (size_t)B * max_blocks * STAT_WAVES;
        stat_nslots = nslots;
        if (need_zeroed(stat_partial, nslots * STAT_N)) return HGS_ERR_DEVICE;
        if (need_zeroed(stat_tsum, (size_t)B)) return HGS_ERR_DEVICE;
        if (groups & 2) { if (int e = need_aff()) return e; }
        HIPCHK(c.dev_out.alloc((size_t)n * 2 * B * 4));
        // (c's buffers are freed on every way out; launches that may still use them have drained by then)
        struct Drain { hipStream_t s; ~Drain() { hipStreamSynchronize(s); } } drain{stream};
        if (groups & 2) {
            if (c.dxy.alloc(ixy.size()) != hipSuccess) return fail(HGS_ERR_DEVICE, "hipMalloc");
            if (hipMemcpyAsync(c.dxy, ixy.data(), ixy.size() * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess) return fail(HGS_ERR_DEVICE, "hipMemcpy");
        }
        hipLaunchKernelGGL(stat_fill_neutral, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, stream, stat_partial.get(), nslots);
        // sum T^2 (the fused path has no NaN targets)
        hipLaunchKernelGGL(ew_sumsq<R>, dim3(ew_blocks, B), dim3(256), 0, stream, (const R*)t, P, epartial.get());
        if (hipGetLastError() != hipSuccess) return fail(HGS_ERR_DEVICE, "statistics setup launch failed");
        if (int r = reduce(epartial, ew_blocks, stat_tsum)) return r;
        stat_ctx = &c;
        const int r = iterate(st, n, hist);
        stat_ctx = nullptr;
        if (r) return r;
        std::vector<double> h((size_t)n * 2 * B * 4);
        if (d2h(h.data(), c.dev_out, h.size() * sizeof(double))) return fail(HGS_ERR_DEVICE, "statistics read-back failed");
        for (int i = 0; i < n; ++i)
            for (int gidx = 0; gidx < 2; ++gidx)
                if (groups & (1 << gidx))
                    std::memcpy(out + ((size_t)i * 2 + gidx) * B * 4, h.data() + ((size_t)i * 2 + gidx) * B * 4, (size_t)B * 4 * sizeof(double));
        return 0;
    }

    hipEvent_t timed_ev[2] = {nullptr, nullptr};      // hgs_iterate_timed: created once (a pair per call costs ~10 us)
    int iterate_timed(hgs_step* st, int n, double* ms) override {
        if (!timed_ev[0]) {
            HIPCHK(hipEventCreate(&timed_ev[0]));
            HIPCHK(hipEventCreate(&timed_ev[1]));
        }
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipEventRecord(timed_ev[0], stream));
        int r = iterate(st, n, nullptr);
        HIPCHK(hipEventRecord(timed_ev[1], stream));
        HIPCHK(hipEventSynchronize(timed_ev[1]));
        float f = 0;
        HIPCHK(hipEventElapsedTime(&f, timed_ev[0], timed_ev[1]));
        *ms = f;
        return r;
    }

    // ---- statistics (_stats.py:7-116): device reductions, host finishing on a handful of doubles ----
    static void finish_stats(const std::vector<double>& fvals, const std::vector<double>& tvals, double total,
                             bool has_total, double* out) {
        // host finishing for short vectors (spot groups): direct restatement on doubles
        double sf = 0, st = 0, stf = 0;
        const size_t n = fvals.size();
        for (size_t i = 0; i < n; ++i) {
            sf += fvals[i] * fvals[i];
            if (tvals[i] == tvals[i]) st += tvals[i] * tvals[i];
        }
        double eff;
        if (has_total) eff = sf / total;
        for (size_t i = 0; i < n; ++i)
            if (tvals[i] == tvals[i]) stf += (tvals[i] / std::sqrt(st)) * (fvals[i] / std::sqrt(sf));
        if (!has_total) eff = stf * stf;
        double rmin = INFINITY, rmax = -INFINITY, emin = INFINITY, emax = -INFINITY, es = 0, es2 = 0, cnt = 0;
        for (size_t i = 0; i < n; ++i) {
            const double tp = tvals[i] * tvals[i] / st, fp = fvals[i] * fvals[i] / sf;
            if (tp != 0 && tp == tp) {
                const double ratio = fp / tp, err = tp - fp;
                rmin = std::fmin(rmin, ratio); rmax = std::fmax(rmax, ratio);
                emin = std::fmin(emin, err); emax = std::fmax(emax, err);
                es += err; es2 += err * err; cnt += 1;
            }
        }
        const double mean = es / cnt, var = std::fmax(0.0, es2 / cnt - mean * mean);
        out[0] = eff;
        out[1] = 1 - (rmax - rmin) / (rmax + rmin);
        out[2] = cnt * (emax - emin);
        out[3] = cnt * std::sqrt(var);
    }

    int stats(int group, int width, const double* xy, double* out) override {
        if (!aff || !state.farfield_valid()) return fail(HGS_ERR_STATE, "statistics need a materialised farfield");
        const int nb = std::min(ew_blocks, 1024);
        if (group == 0) {
            // persistent scratch: hipMalloc / hipFree per call would synchronise the device every iteration
            if (need_zeroed(stats_scratch, (size_t)B * 1024 * 7 + (size_t)B * 2)) return HGS_ERR_DEVICE;
            double* d1 = stats_scratch;
            double* d_sfst = d1 + (size_t)B * nb * 7;
            hipLaunchKernelGGL(stats_pass1<R>, dim3(nb, B), dim3(256), 0, stream, (const R*)aff, (const R*)t, P, d1);
            HIPCHK(hipGetLastError());
            std::vector<double> h((size_t)B * nb * 7);
            if (int e = d2h(h.data(), d1, (size_t)B * nb * 3 * sizeof(double))) return e;
            std::vector<double> sfst(2 * B), stf(B);
            for (int b = 0; b < B; ++b) {
                double s0 = 0, s1 = 0, s2 = 0;
                for (int i = 0; i < nb; ++i) {
                    const double* o = &h[((size_t)b * nb + i) * 3];
                    s0 += o[0]; s1 += o[1]; s2 += o[2];
                }
                sfst[2 * b] = s0; sfst[2 * b + 1] = s1; stf[b] = s2;
            }
            HIPCHK(hipMemcpyAsync(d_sfst, sfst.data(), 2 * B * sizeof(double), hipMemcpyHostToDevice, stream));
            hipLaunchKernelGGL(stats_pass2<R>, dim3(nb, B), dim3(256), 0, stream, (const R*)aff, (const R*)t, P,
                               (const double*)d_sfst, d1);
            HIPCHK(hipGetLastError());
            if (int e = d2h(h.data(), d1, (size_t)B * nb * 7 * sizeof(double))) return e;
            for (int b = 0; b < B; ++b) {
                double rmin = INFINITY, rmax = -INFINITY, emin = INFINITY, emax = -INFINITY, es = 0, es2 = 0, cnt = 0;
                for (int i = 0; i < nb; ++i) {
                    const double* o = &h[((size_t)b * nb + i) * 7];
                    rmin = std::fmin(rmin, o[0]); rmax = std::fmax(rmax, o[1]);
                    emin = std::fmin(emin, o[2]); emax = std::fmax(emax, o[3]);
                    es += o[4]; es2 += o[5]; cnt += o[6];
                }
                const double eff = stf[b] / std::sqrt(sfst[2 * b] * sfst[2 * b + 1]);
                const double mean = es / cnt, var = std::fmax(0.0, es2 / cnt - mean * mean);
                out[4 * b + 0] = eff * eff;
                out[4 * b + 1] = 1 - (rmax - rmin) / (rmax + rmin);
                out[4 * b + 2] = cnt * (emax - emin);
                out[4 * b + 3] = cnt * std::sqrt(var);
            }
            return 0;
        }
        if (group == 1) {
            if (cfg.n_spots <= 0 || !xy) return fail(HGS_ERR_STATE, "spot statistics need spots");
            const int N = cfg.n_spots;
            // window sums at floor(spot_knm) (take() floors, quirk A18); width 1 = the pixel itself
            std::vector<int32_t> ixy(2 * N);
            if (int e = check_windows(xy, xy + N, N, width, ixy.data(), "integration window of spot %d leaves the grid")) return e;
            if (need_zeroed(stats_dxy, (size_t)2 * N)) return HGS_ERR_DEVICE;
            int* dxy = stats_dxy;
            HIPCHK(hipMemcpyAsync(dxy, ixy.data(), 2 * N * sizeof(int), hipMemcpyHostToDevice, stream));
            SpotArgs<R> s{};
            s.g = g; s.n_spots = N; s.width = width; s.feedback = 1; s.spot_xy = dxy; s.amp_ff = aff; s.fb = spot_fb;
            hipLaunchKernelGGL(spot_window<R>, dim3((N + 127) / 128, B), dim3(128), 0, stream, s);
            HIPCHK(hipGetLastError());
            std::vector<R> fb((size_t)B * N);
            std::vector<double> tv(N), fs(B);
            HIPCHK(hipMemcpyAsync(fb.data(), spot_fb, (size_t)B * N * sizeof(R), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipMemcpyAsync(tv.data(), spot_amp, N * sizeof(double), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipMemcpyAsync(fs.data(), sums, B * sizeof(double), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            for (int b = 0; b < B; ++b) {
                std::vector<double> fv(N);
                for (int n = 0; n < N; ++n) fv[n] = (double)fb[(size_t)b * N + n];
                finish_stats(fv, tv, fs[b], true, out + 4 * b);
            }
            return 0;
        }
        return fail(HGS_ERR_ARG, "unknown statistics group %d", group);
    }

    int set_option(int option, int value) override {
        // (a change of the column policy may change which columns the next launch expects in gh)
        if (option == HGS_OPT_SPARSE_COLUMNS || option == HGS_OPT_FORCE_STEPWISE || option == HGS_OPT_TILE_KERNEL) state.column_policy_changed();
        switch (option) {
            case HGS_OPT_SPARSE_COLUMNS: tun.sparse = value ? 1 : 0; return 0;
            case HGS_OPT_FORCE_STEPWISE: opt_stepwise = value ? 1 : 0; return 0;
            case HGS_OPT_TILE_KERNEL: tun.tile = value ? 1 : 0; state.scan_policy_changed(); return 0;
            case HGS_OPT_SEPARABLE: comp.opt_separable = value ? 1 : 0; return 0;
            case HGS_OPT_SEPARABLE_MIN_SPOTS: comp.opt_sep_min = value > 0 ? value : 1; return 0;
            case HGS_OPT_SEP_WORKGROUPS:
                if (value < 0) return fail(HGS_ERR_ARG, "HGS_OPT_SEP_WORKGROUPS must be 0 (2 x #CU) or a positive workgroup count, got %d", value);
                return comp.set_sep_workgroups(cview(), value);
            case HGS_OPT_RUN_KERNELS: comp.opt_run = value ? 1 : 0; return 0;
            case HGS_OPT_EMPTY_COL_LOADS: tun.empty_col_loads = value ? 1 : 0; return 0;
            case HGS_OPT_EMPTY_COL_INVERSE: tun.empty_col_inverse = value ? 1 : 0; return 0;
            case HGS_OPT_EMPTY_COL_FORWARD: tun.empty_col_forward = value ? 1 : 0; return 0;
            case HGS_OPT_EMPTY_COL_PREZERO: tun.empty_col_prezero = value ? 1 : 0; return 0;
            case HGS_OPT_EMPTY_COL_LIST: tun.empty_col_list = value ? 1 : 0; return 0;
            case HGS_OPT_KEEP_PREV_PHASE: opt_prev_phase = value ? 1 : 0; if (!value) state.prev_phase_dropped(); return 0;
            case HGS_OPT_ROCTX:
                if (value && !g_roctx.load()) return fail(HGS_ERR_UNSUPPORTED, "no roctx library (librocprofiler-sdk-roctx / libroctx64) found");
                opt_roctx = value ? 1 : 0;
                return 0;
        }
        return fail(HGS_ERR_ARG, "unknown option %d", option);
    }
    int sync() override {
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
};

// makes `dev` current for the calling thread, restores the previous device when it goes out of scope
struct DeviceGuard {
    int prev = -1, dev;
    bool ok = true;
    DispatchLog* prev_log;
    explicit DeviceGuard(int d, DispatchLog* log = nullptr) : dev(d), prev_log(g_dispatch) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
        g_dispatch = log;
    }
    ~DeviceGuard() {
        g_dispatch = prev_log;
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};

}  // namespace hgs

// =================================================================================================
// C ABI
// =================================================================================================
struct hgs_engine {
    hgs::EngineBase* impl;
};

extern "C" {

int hgs_create(const hgs_config* cfg, hgs_engine** out) {
    if (!cfg || !out) return hgs::fail(HGS_ERR_ARG, "null argument");
    *out = nullptr;
    hgs::EngineBase* impl = nullptr;
    if (cfg->real_bytes == 4) impl = new hgs::Engine<float>();
    else if (cfg->real_bytes == 8) impl = new hgs::Engine<double>();
    else return hgs::fail(HGS_ERR_ARG, "real_bytes must be 4 or 8 (got %d)", cfg->real_bytes);
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    int e = impl->init(*cfg);
    if (prev >= 0 && prev != cfg->device) (void)hipSetDevice(prev);
    if (e) {
        delete impl;
        return e;
    }
    *out = new hgs_engine{impl};
    return 0;
}

int hgs_destroy(hgs_engine* e) {
    if (!e) return 0;
    delete e->impl;
    delete e;
    return 0;
}

// every entry point validates the handle and makes the engine's device current for the calling thread
// (lazy allocations, event creation and launches all follow the current device)
// and puts the caller's device back on return: a torch process whose current device differs from the engine's
// keeps allocating and launching where it was
#define ENG(e)                                                                         \
    if (!(e) || !(e)->impl) return hgs::fail(HGS_ERR_ARG, "null engine handle");       \
    hgs::DeviceGuard guard_((e)->impl->device, &(e)->impl->dispatch);                   \
    if (!guard_.ok) return hgs::fail(HGS_ERR_DEVICE, "hipSetDevice(%d) failed", (e)->impl->device);

int hgs_set_array(hgs_engine* e, int which, const void* host, size_t nbytes) { ENG(e) return e->impl->set_array(which, host, nbytes, false); }
int hgs_set_array_device(hgs_engine* e, int which, const void* dev, size_t nbytes) { ENG(e) return e->impl->set_array(which, dev, nbytes, true); }
int hgs_copy_phase(hgs_engine* dst, hgs_engine* src) {
    if (!src || !src->impl) return hgs::fail(HGS_ERR_ARG, "null source engine");
    ENG(dst)
    hgs::EngineBase::PhaseRef ref;
    if (int r = src->impl->phase_ref(&ref)) return r;
    return dst->impl->copy_phase_from(ref);
}
int hgs_get_array(hgs_engine* e, int which, void* host, size_t nbytes) { ENG(e) return e->impl->get_array(which, host, nbytes, false); }
int hgs_get_array_device(hgs_engine* e, int which, void* dev, size_t nbytes) { ENG(e) return e->impl->get_array(which, dev, nbytes, true); }
int hgs_reset_weights(hgs_engine* e) { ENG(e) return e->impl->reset_weights(); }
int hgs_reset(hgs_engine* e) { ENG(e) return e->impl->reset_state(); }
int hgs_set_array_sparse(hgs_engine* e, int which, const int32_t* xy, const void* values, int32_t n) {
    ENG(e)
    return e->impl->set_array_sparse(which, xy, values, n);
}
int hgs_nearfield2farfield(hgs_engine* e, int store_phase_ff) { ENG(e) return e->impl->n2f(store_phase_ff); }
int hgs_farfield_constraint(hgs_engine* e, hgs_step* step) {
    ENG(e)
    if (!step) return hgs::fail(HGS_ERR_ARG, "null step");
    return e->impl->constraint(step);
}
int hgs_farfield2nearfield(hgs_engine* e) { ENG(e) return e->impl->f2n(); }
int hgs_multiplane_farfield2nearfield(hgs_engine* const* children, const double* weights, int n) {
    if (!children || !weights || n < 1) return hgs::fail(HGS_ERR_ARG, "multiplane: need at least one child and its weight");
    if (n > hgs::MP_MAX) return hgs::fail(HGS_ERR_UNSUPPORTED, "multiplane: at most %d children", hgs::MP_MAX);
    hgs::EngineBase::MpInfo info[hgs::MP_MAX];
    for (int k = 0; k < n; ++k) {       // validate the whole family before touching any state
        if (!children[k] || !children[k]->impl) return hgs::fail(HGS_ERR_ARG, "multiplane: null child %d", k);
        if (int r = children[k]->impl->mp_info(&info[k])) return r;
        if (info[k].S != info[0].S || info[k].B != info[0].B || info[k].real_bytes != info[0].real_bytes ||
            info[k].device != info[0].device)
            return hgs::fail(HGS_ERR_ARG, "multiplane: child %d differs in SLM shape, batch, precision or device", k);
    }
    hgs::DeviceGuard guard_(info[0].device);
    if (!guard_.ok) return hgs::fail(HGS_ERR_DEVICE, "hipSetDevice(%d) failed", info[0].device);
    for (int k = 0; k < n; ++k) {
        hgs::g_dispatch = &children[k]->impl->dispatch;
        if (int r = children[k]->impl->f2n_complex()) return r;
        if (int r = children[k]->impl->mp_info(&info[k])) return r;     // the nearfield buffer exists now
    }
    // every child's inverse transform must have landed before child 0's stream reads them
    for (int k = 1; k < n; ++k)
        if (hipStreamSynchronize(info[k].stream) != hipSuccess) return hgs::fail(HGS_ERR_DEVICE, "multiplane: stream sync failed");
    hgs::g_dispatch = nullptr;
    return children[0]->impl->mp_combine(info, weights, n);
}
int hgs_iterate(hgs_engine* e, hgs_step* step, int n_iter, uint8_t* hist) {
    ENG(e)
    if (!step) return hgs::fail(HGS_ERR_ARG, "null step");
    return e->impl->iterate(step, n_iter, hist);
}
int hgs_cg_iterate(hgs_engine* e, const hgs_cg_params* params, int n_iter, double* loss_out) {
    ENG(e)
    if (!params) return hgs::fail(HGS_ERR_ARG, "null parameters");
    return e->impl->cg_iterate(params, n_iter, loss_out);
}
int hgs_remove_vortices(hgs_engine* e, int32_t* n_removed) { ENG(e) return e->impl->remove_vortices(n_removed); }
int hgs_get_display(hgs_engine* e, const hgs_display_params* p, void* host, size_t nbytes) {
    ENG(e)
    if (!p) return hgs::fail(HGS_ERR_ARG, "null parameters");
    return e->impl->get_display(p, host, nbytes, false);
}
int hgs_get_display_device(hgs_engine* e, const hgs_display_params* p, void* dev, size_t nbytes) {
    ENG(e)
    if (!p) return hgs::fail(HGS_ERR_ARG, "null parameters");
    return e->impl->get_display(p, dev, nbytes, true);
}
int hgs_iterate_stats(hgs_engine* e, hgs_step* step, int n_iter, uint8_t* hist, int stat_groups, int width,
                      const double* spot_xy_float, double* stats_out) {
    ENG(e)
    if (!step) return hgs::fail(HGS_ERR_ARG, "null step");
    return e->impl->iterate_stats(step, n_iter, hist, stat_groups, width, spot_xy_float, stats_out);
}
int hgs_stats(hgs_engine* e, int group, int width, const double* xy, double* out) {
    ENG(e)
    if (!out) return hgs::fail(HGS_ERR_ARG, "null output");
    return e->impl->stats(group, width, xy, out);
}
int hgs_sync(hgs_engine* e) { ENG(e) return e->impl->sync(); }
int hgs_set_option(hgs_engine* e, int option, int value) { ENG(e) return e->impl->set_option(option, value); }
int hgs_profile_enable(hgs_engine* e, int on) { ENG(e) return e->impl->profile_enable(on); }
int hgs_profile_read(hgs_engine* e, double* out) {
    ENG(e)
    if (!out) return hgs::fail(HGS_ERR_ARG, "null output");
    return e->impl->profile_read(out);
}
int hgs_iterate_timed(hgs_engine* e, hgs_step* step, int n_iter, double* ms) {
    ENG(e)
    if (!step || !ms) return hgs::fail(HGS_ERR_ARG, "null argument");
    return e->impl->iterate_timed(step, n_iter, ms);
}

static int dispatch_text_out(hgs::DispatchLog& log, char* buf, size_t nbytes, size_t* needed) {
    const std::string t = log.text();
    if (needed) *needed = t.size() + 1;
    if (!buf || nbytes < t.size() + 1) {
        if (buf && nbytes) buf[0] = 0;
        if (!buf && nbytes == 0 && needed) return 0;      // size query: the record is kept
        return hgs::fail(HGS_ERR_ARG, "dispatch record needs %zu bytes", t.size() + 1);
    }
    std::memcpy(buf, t.c_str(), t.size() + 1);
    log.v.clear();
    return 0;
}

int hgs_dispatch_read(hgs_engine* e, char* buf, size_t nbytes, size_t* needed) {
    if (!e || !e->impl) return hgs::fail(HGS_ERR_ARG, "null engine handle");
    return dispatch_text_out(e->impl->dispatch, buf, nbytes, needed);
}

int hgs_poly_dispatch_read(char* buf, size_t nbytes, size_t* needed) { return dispatch_text_out(hgs::g_poly_log, buf, nbytes, needed); }

int hgs_set_array_poly(hgs_engine* e, int which, const hgs_poly_params* p) { ENG(e) return e->impl->set_array_poly(which, p); }

int hgs_poly_eval(const hgs_poly_params* p, void* out, size_t nbytes, int out_is_device) {
    if (int r = hgs::poly_check(p)) return r;
    if (!out) return hgs::fail(HGS_ERR_ARG, "null destination pointer");
    const int out_bytes = p->out_bytes ? p->out_bytes : p->grid_bytes;
    if (out_bytes != 4 && out_bytes != 8) return hgs::fail(HGS_ERR_ARG, "hgs_poly_eval: out_bytes must be 0, 4 or 8 (got %d)", p->out_bytes);
    const size_t all = (size_t)p->n * p->h * p->w * out_bytes;
    if (nbytes != all)
        return hgs::fail(HGS_ERR_ARG, "hgs_poly_eval: bad size %zu (%zu expected: %d masks of %d x %d %d-byte reals)", nbytes, all, p->n, p->h, p->w, out_bytes);
    if (out_is_device && ((uintptr_t)out % (uintptr_t)out_bytes))
        return hgs::fail(HGS_ERR_ARG, "hgs_poly_eval: the device buffer is not aligned to its %d-byte elements", out_bytes);
    hgs::DeviceGuard guard_(p->device, &hgs::g_poly_log);
    if (!guard_.ok) return hgs::fail(HGS_ERR_DEVICE, "hipSetDevice(%d) failed", p->device);
    auto plain = [](auto&& launch) -> int { return launch(); };
    if (out_is_device) return hgs::poly_run(p, out, out_bytes, nullptr, plain);
    hgs::DevBuf<char> tmp;
    if (tmp.alloc(all) != hipSuccess) return hgs::fail(HGS_ERR_DEVICE, "hgs_poly_eval: no device memory for %zu bytes", all);
    if (int r = hgs::poly_run(p, tmp.get(), out_bytes, nullptr, plain)) return r;
    if (hipMemcpy(out, tmp.get(), all, hipMemcpyDeviceToHost) != hipSuccess) return hgs::fail(HGS_ERR_DEVICE, "hgs_poly_eval: device to host copy failed");
    return 0;
}

int hgs_pattern_dispatch_read(char* buf, size_t nbytes, size_t* needed) { return dispatch_text_out(hgs::g_poly_log, buf, nbytes, needed); }

int hgs_set_array_pattern(hgs_engine* e, int which, const hgs_pattern_params* p) { ENG(e) return e->impl->set_array_pattern(which, p); }

int hgs_pattern_eval(const hgs_pattern_params* p, void* out, size_t nbytes, int out_is_device) {
    if (int r = hgs::pattern_check(p)) return r;
    if (!out) return hgs::fail(HGS_ERR_ARG, "null destination pointer");
    const int out_bytes = p->out_bytes ? p->out_bytes : p->grid_bytes;
    if (out_bytes != 4 && out_bytes != 8) return hgs::fail(HGS_ERR_ARG, "hgs_pattern_eval: out_bytes must be 0, 4 or 8 (got %d)", p->out_bytes);
    const size_t all = (size_t)p->h * p->w * out_bytes;
    if (nbytes != all)
        return hgs::fail(HGS_ERR_ARG, "hgs_pattern_eval: bad size %zu (%zu expected: %d x %d %d-byte reals)", nbytes, all, p->h, p->w, out_bytes);
    if (out_is_device && ((uintptr_t)out % (uintptr_t)out_bytes))
        return hgs::fail(HGS_ERR_ARG, "hgs_pattern_eval: the device buffer is not aligned to its %d-byte elements", out_bytes);
    hgs::DeviceGuard guard_(p->device, &hgs::g_poly_log);
    if (!guard_.ok) return hgs::fail(HGS_ERR_DEVICE, "hipSetDevice(%d) failed", p->device);
    auto plain = [](auto&& launch) -> int { return launch(); };
    if (out_is_device) return hgs::pattern_run(p, out, out_bytes, nullptr, plain);
    hgs::DevBuf<char> tmp;
    if (tmp.alloc(all) != hipSuccess) return hgs::fail(HGS_ERR_DEVICE, "hgs_pattern_eval: no device memory for %zu bytes", all);
    if (int r = hgs::pattern_run(p, tmp.get(), out_bytes, nullptr, plain)) return r;
    if (hipMemcpy(out, tmp.get(), all, hipMemcpyDeviceToHost) != hipSuccess) return hgs::fail(HGS_ERR_DEVICE, "hgs_pattern_eval: device to host copy failed");
    return 0;
}

const char* hgs_last_error(void) { return hgs::g_err.c_str(); }

const char* hgs_version(void) {
    static std::string v;
    if (v.empty()) {
        v = "hgs 0.2 gfx950";
        int n = 0;
        if (hipGetDeviceCount(&n) == hipSuccess && n > 0) {
            hipDeviceProp_t p;
            if (hipGetDeviceProperties(&p, 0) == hipSuccess) v += std::string(" ") + p.name + " " + p.gcnArchName;
        } else {
            v += " (no device)";
        }
    }
    return v.c_str();
}

}  // extern "C"
