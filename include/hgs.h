/*
 * hgs.h -- C ABI of the MI355X hologram (Gerchberg-Saxton / weighted-GS) engine.
 *
 * This is the drop-in boundary for slmsuite's optimize() hot path.  The reference has no FFI of
 * its own: the path sits behind the array-module alias `cp` (slmsuite/holography/algorithms/
 * _header.py:15-32) and the overridable per-iteration methods of `Hologram`
 * (slmsuite/holography/algorithms/_hologram.py).  Each entry point below replaces the reference
 * method(s) cited next to it; INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative hgs_status otherwise; the message of the
 *     last error of the calling thread is available from hgs_last_error();
 *   - an engine handle is single-threaded; different handles are independent; every entry point makes the
 *     engine's HIP device current for the duration of the call and restores the caller's current device;
 *   - the engine owns all device memory and one HIP stream; host buffers are caller-owned,
 *     C-contiguous, in the reference's natural layout (row-major, centred zero order), of the
 *     engine's real type (float when real_bytes == 4, double when 8; complex = 2 reals);
 *   - batched arrays are [batch][...]; passing exactly one hologram's bytes broadcasts it;
 *   - calls are asynchronous on the engine stream unless they move data to/from the host.
 *   - there is NO CPU fallback: without a usable gfx950 device hgs_create fails with
 *     HGS_ERR_DEVICE.
 */
#ifndef HGS_H
#define HGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hgs_engine hgs_engine;

typedef enum {
    HGS_OK = 0,
    HGS_ERR_ARG = -1,      /* invalid argument (ValueError on the Python side)            */
    HGS_ERR_DEVICE = -2,   /* no device / HIP runtime error (RuntimeError)                */
    HGS_ERR_STATE = -3,    /* operation not valid in the current state                    */
    HGS_ERR_UNSUPPORTED = -4
} hgs_status;

/* Geometry of one engine.  Hologram.__init__ (_hologram.py:196-439): `shape` -> pad_h/pad_w,
 * `slm_shape` -> slm_h/slm_w, dtype (:391-398) -> real_bytes.  Powers of two in [64, 8192] run the fused
 * kernels; any other shape (the reference only warns about those, :378-384) runs the same operators axis by
 * axis on the workgroup transforms (general operators only, no fused loop): a power-of-two axis up to 16384
 * (float64: 8192) directly, any other length in [2, 8192] (float64: [2, 4096]) through Bluestein's identity.
 * Longer axes return HGS_ERR_UNSUPPORTED.  The SLM block is
 * centred (toolbox.unpad, toolbox/__init__.py:1699-1712). */
typedef struct {
    int32_t device;      /* HIP device ordinal                                          */
    int32_t pad_h, pad_w;
    int32_t slm_h, slm_w;
    int32_t real_bytes;  /* 4 | 8                                                       */
    int32_t batch;       /* independent holograms advanced together        */
    int32_t n_spots;     /* > 0 enables spot-window / external-spot feedback            */
    int32_t kind;        /* 0: padded DFT grid (Hologram / SpotHologram);
                            1: CompressedSpotHologram (_spots.py:178-1018): n_spots free-floating
                               spots with polynomial phase kernels, no padded grid (pad_* ignored) */
    int32_t n_monomials; /* kind 1: monomials x^px y^py of the kernel phase polynomial  */
} hgs_config;

/* ALGORITHM_INDEX (_header.py:72) */
enum { HGS_GS = 0, HGS_WGS_LEONARDO = 1, HGS_WGS_KIM = 2, HGS_WGS_NOGRETTE = 3, HGS_WGS_WU = 4,
       HGS_WGS_TANH = 5 };
/* feedback sources of _update_weights (_hologram.py:1914, _spots.py:1573-1624) */
enum { HGS_FB_PIXEL = 0 /* "computational" */, HGS_FB_SPOT_WINDOW = 1 /* "computational_spot" */,
       HGS_FB_EXTERNAL = 2 /* "external_spot" */ };

/* Per-call flags: the POD image of Hologram.flags (_hologram.py:1370-1410).  Fields marked
 * in/out are advanced by the engine exactly as optimize_gs / _gs_farfield_routines do. */
typedef struct {
    int32_t method;              /* HGS_GS ...                                           */
    int32_t feedback;            /* HGS_FB_*                                             */
    int32_t iter;                /* in/out  self.iter (:1490)                            */
    int32_t fixed_phase;         /* in/out  flags["fixed_phase"] (:1556-1585).  Set while the engine holds
                                    no phase_ff (after hgs_reset), an iteration stores the phase first --
                                    the guard of :1601.  The reference's MRAF branch (:1643) lacks that
                                    guard and raises there; a host that wants the
                                    reference's behaviour refuses the call, as the Python class does    */
    int32_t fix_phase_iteration; /* flags["fix_phase_iteration"]                         */
    int32_t false_run;           /* in/out  trailing count of contiguous False entries in
                                    stats["flags"]["fixed_phase"] (:1574-1577); -1 = history
                                    contains a non-boolean entry (never fixes by iteration)   */
    int32_t mraf_enabled;        /* target contains NaN (_mraf_helper_routines :1498)    */
    int32_t has_mraf_factor;     /* flags["mraf_factor"] is not None                     */
    int32_t zero_mode;           /* flags["zero_factor"] given and != 0 (:1514)          */
    int32_t spot_window;         /* spot_integration_width_knm (_spots.py:1284-1297)     */
    int32_t efficiency_group;    /* statistics group whose efficiency gates WGS-Kim (0 "computational",
                                    1 "computational_spot"): the LAST group of stats["stats"] (:1562-1567) */
    int32_t reserved;            /* keeps the doubles 8-byte aligned; set to 0           */
    double feedback_exponent, feedback_factor, mraf_factor, zero_factor;
    double fix_phase_efficiency; /* flags["fix_phase_efficiency"] (:1560-1569), NaN = None.  WGS-Kim only: the
                                    phase is fixed from the iteration AFTER the first one (iter > 0) whose recorded
                                    efficiency exceeds it.  Needs hgs_iterate_stats with that group (batch = 1);
                                    hgs_iterate / hgs_farfield_constraint return HGS_ERR_ARG when it is set without
                                    statistics ("Must track statistics ..."), like the reference's ValueError. */
} hgs_step;

/* array selectors for hgs_set_array / hgs_get_array */
enum {
    HGS_PHASE = 0,        /* [batch][slm_h][slm_w] real      Hologram.phase              */
    HGS_AMP = 1,          /* [slm_h][slm_w] real, unit L2    Hologram.amp (array form)   */
    HGS_AMP_SCALAR = 2,   /* 1 real                          Hologram.amp (scalar form)  */
    HGS_PROP_KERNEL = 3,  /* [slm_h][slm_w] real             Hologram.propagation_kernel; nbytes = 0: none */
    HGS_TARGET = 4,       /* [batch][pad_h][pad_w] real      Hologram.target (may hold NaN) */
    HGS_WEIGHTS = 5,      /* [batch][pad_h][pad_w] real      Hologram.weights            */
    HGS_PHASE_FF = 6,     /* [batch][pad_h][pad_w] real      Hologram.phase_ff           */
    HGS_FARFIELD = 7,     /* [batch][pad_h][pad_w] complex   Hologram.farfield           */
    HGS_AMP_FF = 8,       /* [batch][pad_h][pad_w] real      Hologram.amp_ff             */
    HGS_SPOT_INDEX = 9,   /* int32 [2][n_spots] (kx row 0, ky row 1)  spot_knm_rounded   */
    HGS_SPOT_AMP = 10,    /* double [n_spots]                SpotHologram.spot_amp       */
    HGS_EXTERNAL_AMP = 11,/* double [n_spots]                external_spot_amp           */
    HGS_ZERO_WEIGHTS = 12,/* [batch][pad_h][pad_w] complex   dense image of zero_weights */
    /* kind 1 (CompressedSpotHologram); TARGET/WEIGHTS/PHASE_FF/FARFIELD/AMP_FF are [batch][n_spots] */
    HGS_XGRID = 13,       /* [slm_h][slm_w] real   slm.grid[0] * zernike scaling (_spots.py:614-618) */
    HGS_YGRID = 14,       /* [slm_h][slm_w] real   slm.grid[1] * zernike scaling                     */
    HGS_MONOMIALS = 15,   /* int32 [n_monomials][2] (px, py)   phase._zernike_get_cantor terms; the pseudo-term
                             (-1, 0) is the vortex plate w * atan2(y, x), w > 0 only (phase.py:1783-1790)     */
    HGS_SPOT_COEFF = 16,  /* real [n_monomials][n_spots]       ... and weights (phase.py:850-920)    */
    HGS_PHASE_PREV = 17,  /* get only: [batch][slm_h][slm_w] real -- the phase the last one-iteration hgs_iterate call
                             STARTED from (HGS_OPT_KEEP_PREV_PHASE); HGS_ERR_STATE when none is held */
    HGS_CG_GRAD = 18,     /* get only: [slm_h][slm_w] real -- dL/dphase of the last hgs_cg_iterate body that kept it
                             (hgs_cg_params.keep_grad); HGS_ERR_STATE before the first such body */
    HGS_VORTICES = 19,    /* get only: int32 [n][3] (x, y, winding) -- the vortices the last hgs_remove_vortices call found and
                             removed, n its n_removed; HGS_ERR_STATE before the first call */
    HGS_DISPLAY_CORRECTION = 20 /* hgs_set_array only: DOUBLE [slm_h][slm_w] in either precision -- the wavefront correction
                             hgs_get_display adds (slm.source["phase"], float64 in the reference); nbytes = 0: none */
};

int hgs_create(const hgs_config* cfg, hgs_engine** out);
int hgs_destroy(hgs_engine* e);

/* host -> device / device -> host (synchronous).  Replaces the cp.array(...)/.get() traffic of
 * Hologram.__init__, reset_phase (:536), set_weights (:829), get_phase (:786) ... */
int hgs_set_array(hgs_engine* e, int which, const void* host, size_t nbytes);
int hgs_get_array(hgs_engine* e, int which, void* host, size_t nbytes);
/* device -> caller-provided DEVICE buffer (e.g. a torch tensor handed to RCCL); synchronous */
int hgs_get_array_device(hgs_engine* e, int which, void* dev, size_t nbytes);
/* caller-provided DEVICE buffer -> engine (same layouts and sizes as hgs_set_array): what the reference does when it is
 * handed CuPy arrays (`cp.array(x, copy=False)`, _hologram.py:70-77) -- no host bounce.  Arrays the engine parses on the
 * host (HGS_SPOT_INDEX, HGS_XGRID/YGRID, HGS_MONOMIALS, HGS_SPOT_COEFF, HGS_AMP_SCALAR) return HGS_ERR_UNSUPPORTED. */
int hgs_set_array_device(hgs_engine* e, int which, const void* dev, size_t nbytes);
/* dst.phase <- src.phase on the device (same SLM shape and precision; one source hologram broadcasts over dst's batch;
 * engines on different GPUs use a peer copy).  Hologram.get_farfield (_hologram.py:853-931, the per-frame call of
 * SimulatedCamera) transforms the current phase on another grid without moving it through the host. */
int hgs_copy_phase(hgs_engine* dst, hgs_engine* src);
/* Hologram.reset_weights (:603-614): weights = target with NaN -> 0; zero_weights cleared */
int hgs_reset_weights(hgs_engine* e);
/* Hologram.reset (:442-478) as far as the device is concerned: hgs_reset_weights, and phase_ff / farfield /
 * amp_ff go back to "None" (a later WGS-Kim fix stores a fresh phase; reading them back fails with
 * HGS_ERR_STATE until hgs_nearfield2farfield ran).  Phase, amplitude, target, spots and options stay. */
int hgs_reset(hgs_engine* e);
/* Sparse upload of a farfield-sized real array (HGS_TARGET or HGS_WEIGHTS, kind 0): the array becomes ZERO everywhere
 * except values[k] at pixel (kx = xy[k], ky = xy[n + k]), k < n, later entries winning where pixels repeat (NumPy fancy
 * assignment, _spots.py:1541).  One hologram's list broadcasts over the batch.  This is what
 * SpotHologram._set_target_spots produces without null points: n_spots values instead of pad_h * pad_w.  A NaN
 * background (null points) cannot be expressed here: upload such a target densely with hgs_set_array. */
int hgs_set_array_sparse(hgs_engine* e, int which, const int32_t* xy, const void* values, int32_t n);

/* Hologram._nearfield2farfield (:1038-1056) + _midloop_cleaning (:951-953): fills farfield and
 * amp_ff; with store_phase_ff != 0 also phase_ff = atan2(farfield) (_populate_results :934-949). */
int hgs_nearfield2farfield(hgs_engine* e, int store_phase_ff);
/* Hologram._gs_farfield_routines (:1550-1661) incl. _update_weights (:1914 / _spots.py:1573) and
 * _update_weights_generic (:1786-1879); operates on the materialised farfield. */
int hgs_farfield_constraint(hgs_engine* e, hgs_step* step);
/* Hologram._farfield2nearfield (:1058-1073) + _nearfield_extract (:1026-1036). */
int hgs_farfield2nearfield(hgs_engine* e);
/* n_iter bodies of the optimize_gs loop (:1465-1490) with no callback and no statistics:
 * the fused fast path (the farfield is never materialised when the method allows it).
 * fixed_phase_history[n_iter] (optional) receives flags["fixed_phase"] as _update_stats would
 * have recorded it in each iteration. */
int hgs_iterate(hgs_engine* e, hgs_step* step, int n_iter, uint8_t* fixed_phase_history);
/* _HologramStats._calculate_stats (_stats.py:7-116), efficiency_compensation = False.
 * group 0: "computational" (amp_ff vs target); group 1: "computational_spot"
 * (window sums at spot_knm with total power, _spots.py:1626-1679).
 * out[batch][4] = efficiency, uniformity, pkpk_err, std_err.  Needs a materialised farfield. */
int hgs_stats(hgs_engine* e, int group, int width, const double* spot_xy_float, double* out);

/* hgs_iterate for optimize(..., stat_groups=[...]) (_hologram.py:1479): additionally returns
 * the statistics _update_stats records in every iteration, i.e. those of the farfield the iteration
 * starts from.  stat_groups: bit 0 "computational", bit 1 "computational_spot" (needs width and
 * spot_xy_float as hgs_stats).  stats_out[n_iter][2][batch][4] (group slot 0 / 1; slots of groups
 * not requested are NaN).  On the fused path the column kernel accumulates the reductions in the
 * pass that applies the constraint (no farfield is materialised, one host read at the end);
 * otherwise the call runs the general path with a hgs_stats per iteration. */
int hgs_iterate_stats(hgs_engine* e, hgs_step* step, int n_iter, uint8_t* fixed_phase_history,
                      int stat_groups, int width, const double* spot_xy_float, double* stats_out);

/* Hologram.optimize_cg (_hologram.py:1664-1759) with the reference's defaults: loss ComplexMSELoss (:6-14, mean reduction),
 * optimizer torch.optim.Adam without weight decay or amsgrad, feedback "computational".  No autograd: the loss
 *     L = (1 / M) sum_k (|F_k| / ||F|| - t_k)^2,   F = the farfield of amp * exp(i (phase + propagation_kernel)),  M = pad_h * pad_w
 * has the closed-form gradient dL/dphase = Im(conj(n) g), n the nearfield and g the inverse transform of
 * (2 / (M ||F||)) (|F| / ||F|| - t) F / |F| over the SLM window (the term through ||F|| vanishes: the transform is unitary and
 * ||n|| does not depend on the phase).  One body is hgs_nearfield2farfield, an element-wise pass over the farfield, the
 * inverse transform without phase extraction and an element-wise Adam update over the SLM window
 *     m <- beta1 m + (1 - beta1) g,   v <- beta2 v + (1 - beta2) g^2,
 *     phase <- phase - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps),     t = 1, 2, ...
 * The phase is not wrapped.  The engine keeps m, v and t between calls; `restart` zeroes them first (the reference builds a
 * new optimizer in every optimize() call), and so does hgs_reset, after which HGS_CG_GRAD is not held either.  Weights, phase_ff and the statistics are untouched; the farfield buffer is
 * consumed (hgs_nearfield2farfield rebuilds it from the new phase).  The target must not hold NaN (the loss would be NaN). */
typedef struct {
    double lr, beta1, beta2, eps;
    int32_t restart;     /* != 0: zero m, v and t before the first body                                   */
    int32_t keep_grad;   /* != 0: every body also stores its gradient for hgs_get_array(HGS_CG_GRAD)       */
} hgs_cg_params;
/* n_iter bodies without a host synchronisation in between; loss_out[n_iter] (optional) receives the loss each body
 * evaluated, i.e. that of the phase it STARTED from (flags["loss_result"], :1714).  kind 0 and batch 1 only
 * (HGS_ERR_UNSUPPORTED otherwise); power-of-two and general padded shapes alike. */
int hgs_cg_iterate(hgs_engine* e, const hgs_cg_params* params, int n_iter, double* loss_out);

/* Hologram._remove_vortices (_hologram.py:961-998) as its code intends -- the reference acts only under plot=True --:
 * analysis.image_remove_vortices(phase_ff, target > 0) (analysis/__init__.py:1207-1309) on the stored HGS_PHASE_FF.
 *   winding(y, x) = rint(-(dd0[y, x] - dd1[y, x] - dd0[y, x - 1] + dd1[y - 1, x]) / 2 pi),  dd_a = mod(diff_a(phase) - pi, 2 pi):
 *       the winding of the plaquette (y-1..y, x-1..x); row 0 and column 0 hold none;
 *   a vortex counts where the whole 5 x 5 neighbourhood of (y, x) lies inside the grid with target > 0 (binary_erosion with a
 *       zero border; NaN pixels of an MRAF target are outside);
 *   phase_ff -= sum over those vortices of  w * atan2(X - x, Y - y),  X, Y the pixel indices (the reference's argument
 *       order, x first), over the WHOLE image and without wrapping.
 * The list is built in a fixed order (count, scan, scatter), so two calls on the same state agree to the bit in either
 * precision.  n_removed (optional) receives the number of vortices; hgs_get_array(HGS_VORTICES) returns them.  The
 * farfield, amp_ff, the weights, the phase and the statistics are untouched.  kind 0 and batch 1 only (HGS_ERR_UNSUPPORTED
 * otherwise); HGS_ERR_STATE when no phase_ff is held or no target is set; power-of-two and general padded shapes alike. */
int hgs_remove_vortices(hgs_engine* e, int32_t* n_removed);

/* The gray levels an SLM takes, from the device phase: Hologram.get_phase (_hologram.py:786-811), the float branch of
 * SLM.set_phase (hardware/slms/slm.py:664-681) and SLM._phase2gray (:695-783), equal to the reference bit for bit.
 * With R = 2^bitdepth and s = phase_scaling, per pixel
 *     p = phase + pi in the engine's precision (pi rounded to it) -- with include_propagation and a kernel held:
 *         phase + kernel, no pi; without a kernel the flag changes nothing, as in the reference;
 *     x = p widened to double, plus HGS_DISPLAY_CORRECTION where one is held and phase_correct != 0;
 *     y = x * f,  f = -(R * s / 2 / pi);
 *     s == 1:  m = max y over the hologram;  m >= 0: y -= R * 2 * ceil(m / R);  out = (rint(y) - 1) & (R - 1);
 *     s != 1:  min y <= -R or max y > 0:  y -= 1,  y = mod(y, R s) with the divisor's sign,  y += R (1 - s),  and for s > 1
 *              y < 0 -> R - 1;  otherwise y += R - 1;  out = y truncated toward zero.
 * Every product and sum rounds on its own (no fused multiply-add): the shift of the s == 1 branch depends on the data and
 * moves values onto rounding ties.  The extremes are those of ONE hologram -- the reference converts one mask per call --
 * and never leave the device: a range pass and a convert pass, no host synchronisation in between.  NaN phases are
 * undefined, as in the reference.  Output: [batch][slm_h][slm_w] of uint8 (bitdepth <= 8) or uint16, nbytes exactly that;
 * both engine kinds, any batch.  The phase, the farfield and every other array are untouched. */
typedef struct {
    double  phase_scaling;       /* wav_um / wav_design_um, > 0 */
    int32_t bitdepth;            /* 1..16 */
    int32_t include_propagation;
    int32_t phase_correct;
    int32_t reserved;
} hgs_display_params;
int hgs_get_display(hgs_engine* e, const hgs_display_params* p, void* host, size_t nbytes);
/* ... into a caller-provided DEVICE buffer (e.g. a torch tensor); synchronous */
int hgs_get_display_device(hgs_engine* e, const hgs_display_params* p, void* dev, size_t nbytes);

/* Polynomial phase masks rastered on the device: toolbox.phase.polynomial (phase.py:1672-1795) and zernike_sum (:964-1166).
 * For n stacked masks over h * w pixels
 *     out[k][p] = sum over a + b <= degree of table[k][b][a] * xs(p)^a * ys(p)^b  (+ vortex[k] * atan2(ys, xs) where vortex[k] > 0),
 *     xs = x * x_scale,  ys = y * y_scale,
 * evaluated in double by Horner's scheme whatever the grid's type and rounded ONCE to the grid's type (grid_bytes).  table
 * is the dense triangle of monomial coefficients the caller folds its terms and weights into: row b holds the degree - b + 1
 * coefficients of y^b, a ascending; rows follow each other, (degree + 1)(degree + 2) / 2 doubles per mask.  degree above
 * HGS_POLY_MAX_DEGREE returns HGS_ERR_UNSUPPORTED.
 * mask_mode: HGS_POLY_MASK_ZERO / _NAN write 0 / NaN outside  square(x * x_scale) + square(y * y_scale) <= 1, a predicate
 * evaluated in the grid's own type with every product, square and the sum rounded on its own and the scales rounded to that
 * type first -- NumPy's arithmetic, so the masked SET is the reference's.
 * Coordinates: either the two axis vectors of a product grid (x_axis[w], y_axis[h]) or the two full arrays
 * (x_grid[h][w], y_grid[h][w]; rotated or calibrated grids), host pointers of the grid's type.  Full arrays that turn out to
 * be a product grid are read as axes.  hgs_dispatch_read shows which form ran: poly_kernel<R=..,OUT_BYTES=..,PROD=..>. */
enum { HGS_POLY_MASK_NONE = 0, HGS_POLY_MASK_ZERO = 1, HGS_POLY_MASK_NAN = 2 };
#define HGS_POLY_MAX_DEGREE 20
typedef struct {
    int32_t h, w;            /* pixels of one mask                                                     */
    int32_t n;               /* stacked masks                                                          */
    int32_t degree;          /* 0 .. HGS_POLY_MAX_DEGREE                                               */
    int32_t grid_bytes;      /* 4 | 8: type of the coordinates; the values are rounded to it           */
    int32_t out_bytes;       /* hgs_poly_eval: type the values are stored as, 4 | 8; 0 = grid_bytes     */
    int32_t mask_mode;       /* HGS_POLY_MASK_*                                                        */
    int32_t device;          /* hgs_poly_eval: HIP device ordinal                                      */
    double x_scale, y_scale;
    const double* table;     /* [n][(degree + 1)(degree + 2) / 2]                                      */
    const double* vortex;    /* [n], or NULL: no vortex plate                                          */
    const void* x_axis;      /* [w] and                                                                */
    const void* y_axis;      /* [h]: a product grid -- or NULL, then                                   */
    const void* x_grid;      /* [h][w] and                                                             */
    const void* y_grid;      /* [h][w]                                                                 */
} hgs_poly_params;
/* [n][h][w] of out_bytes-sized reals into a host array or, out_is_device != 0, a DEVICE buffer (e.g. a torch tensor) aligned
 * to its element size; nbytes exactly that.  Needs no engine; synchronous.  Its launches are recorded per thread and read
 * with hgs_poly_dispatch_read (buffer semantics of hgs_dispatch_read). */
int hgs_poly_eval(const hgs_poly_params* p, void* out, size_t nbytes, int out_is_device);
int hgs_poly_dispatch_read(char* buf, size_t nbytes, size_t* needed);
/* ... into one of the engine's own arrays, nothing passing through the host: HGS_PROP_KERNEL, HGS_PHASE (one mask broadcast
 * over the batch) in the engine's type, or HGS_DISPLAY_CORRECTION (double).  The values are those hgs_poly_eval gives for
 * grid_bytes, converted to the array's type -- what uploading that result with hgs_set_array stores.  n must be 1 and
 * (h, w) the SLM shape (HGS_ERR_ARG otherwise); out_bytes and device are ignored.  Synchronous. */
int hgs_set_array_poly(hgs_engine* e, int which, const hgs_poly_params* p);

/* The masks of toolbox.phase that are no polynomials, rastered on the device (csrc/pattern_kernels.hpp): sinusoid and binary
 * gratings (phase.py:78-258), the four-window masks built from gratings (quadrants, bahtinov; :261-389), axicon (:455-498),
 * Laguerre-Gauss and Hermite-Gauss mode masks (:1842-1935).
 *   HGS_PATTERN_BLAZE     2 pi (vx x + vy y)                                        (quad only: a plain blaze is a polynomial)
 *   HGS_PATTERN_SINUSOID  (a - b) / 2 * (1 + sin(2 pi (vx x + vy y) + shift)) + b
 *   HGS_PATTERN_BINARY    a where d > 0 or |d| <= 1e-8, else b, with d = mod(2 pi (vx x + vy y) + shift, 2 pi), set to 0 where
 *                         isclose(d, 2 pi), less 2 pi (1 - duty); duty is clipped to [0, 1].  A vector with a component
 *                         above 1 in magnitude counts PIXELS: the coordinates are the pixel indices (within the window, for
 *                         quad) and each component is replaced by its reciprocal (0 stays 0).  A zero vector gives b, or a
 *                         when shift != 0 and mod(shift, 2 pi) > 2 pi duty.  d is formed with NumPy's roundings in the
 *                         grid's type, or in double with decision_double != 0 (vectors that came as float64 scalars) and
 *                         wherever pixels are counted.
 *   HGS_PATTERN_AXICON    2 pi sqrt((x kx)^2 + (y ky)^2), (kx, ky) = vec[0..1]; 2 pi k |x| or 2 pi k |y| where the other is 0
 *   HGS_PATTERN_LG        l atan2(x, y) + pi [L_p^|l|(16 (x^2 + y^2) / w^2) < 0], each term only for l != 0 / p != 0
 *   HGS_PATTERN_HG        pi where H_n(4 x / w) H_m(4 y / w) > 0, else 0
 * quad != 0 (grating modes): four windows that start at row h / 2 and column w / 2, in the order top-right, bottom-right,
 * top-left, bottom-left, each with its own vector vec[2 i], vec[2 i + 1]; the last row and the last column are 0 (the
 * reference clips the end of a window to h - 1 and w - 1).  Otherwise vec[0..1] alone counts.
 * Values are formed in double; round_grid != 0 rounds them to the grid's type before they are stored as out_bytes-sized
 * reals.  Orders p, n, m above HGS_PATTERN_MAX_ORDER return HGS_ERR_UNSUPPORTED, other bad arguments HGS_ERR_ARG.
 * Coordinates as in hgs_poly_params.  The dispatch record shows pattern_kernel<R=..,OUT_BYTES=..,PROD=..,MODE=..> [quad]. */
enum { HGS_PATTERN_BLAZE = 0, HGS_PATTERN_SINUSOID = 1, HGS_PATTERN_BINARY = 2, HGS_PATTERN_AXICON = 3, HGS_PATTERN_LG = 4,
       HGS_PATTERN_HG = 5 };
#define HGS_PATTERN_MAX_ORDER 20
typedef struct {
    int32_t h, w;            /* pixels of the mask                                                      */
    int32_t grid_bytes;      /* 4 | 8: type of the coordinates                                          */
    int32_t out_bytes;       /* hgs_pattern_eval: type the values are stored as, 4 | 8; 0 = grid_bytes  */
    int32_t device;          /* hgs_pattern_eval: HIP device ordinal                                    */
    int32_t mode;            /* HGS_PATTERN_*                                                           */
    int32_t quad;            /* grating modes: four windows                                             */
    int32_t round_grid;      /* round the values to the grid's type                                     */
    int32_t decision_double; /* HGS_PATTERN_BINARY: form d in double                                    */
    int32_t l, p, n, m;      /* HGS_PATTERN_LG: l, p;  HGS_PATTERN_HG: n, m                             */
    int32_t reserved;
    double vec[8];           /* up to four 2-vectors                                                    */
    double shift, a, b, duty;
    double radius;           /* w of the mode masks: the source radius, finite and not 0                */
    const void* x_axis;      /* as in hgs_poly_params                                                   */
    const void* y_axis;
    const void* x_grid;
    const void* y_grid;
} hgs_pattern_params;
/* [h][w] of out_bytes-sized reals into a host array or, out_is_device != 0, a DEVICE buffer aligned to its element size;
 * nbytes exactly that.  Needs no engine; synchronous.  Its launch joins the per-thread record hgs_poly_dispatch_read reads;
 * hgs_pattern_dispatch_read reads that same record. */
int hgs_pattern_eval(const hgs_pattern_params* p, void* out, size_t nbytes, int out_is_device);
int hgs_pattern_dispatch_read(char* buf, size_t nbytes, size_t* needed);
/* ... into HGS_PROP_KERNEL, HGS_PHASE (broadcast over the batch) or HGS_DISPLAY_CORRECTION (double) on the engine's stream,
 * by the rules of hgs_set_array_poly: (h, w) must be the SLM shape, the values are those of hgs_pattern_eval (with
 * out_bytes = 8) converted to the array's type; out_bytes and device are ignored.  Synchronous. */
int hgs_set_array_pattern(hgs_engine* e, int which, const hgs_pattern_params* p);

/* MultiplaneHologram._farfield2nearfield (_multiplane.py:255-279): every child runs
 * _farfield2nearfield(extract=False) on its own (constrained) farfield; the children's complex
 * nearfields over the SLM are summed on the device,
 *     nf = sum_k weights[k] * nf_k * exp(-i propagation_kernel_k),   phase = atan2(nf),
 * and the common phase is written into every child's HGS_PHASE (the reference's children share
 * one phase array).  Children may differ in pad shape and kind but must agree in SLM shape,
 * batch, precision and device; n <= 16.  Synchronous. */
int hgs_multiplane_farfield2nearfield(hgs_engine* const* children, const double* weights, int n);

int hgs_sync(hgs_engine* e);

/* Engine options.  HGS_OPT_SPARSE_COLUMNS (default 1): in hgs_iterate / hgs_iterate_stats, when few of
 * the farfield columns hold a non-zero weight or target (spot arrays), transform only those columns
 * and move only them between the two kernels; the phase and the weights are those of the dense path
 * (every other column of the constrained farfield is exactly zero).  Covers pixel feedback and, with
 * the spot columns dilated by the integration window, the spot feedback modes.  While it is active,
 * HGS_PHASE_FF stored by WGS-Kim is refreshed on the active columns only (the rest cannot influence the
 * loop; hgs_nearfield2farfield(store_phase_ff = 1) refreshes every pixel).  0 forces the dense kernels.
 *   Where the tile-resident kernel applies (fp32, pad_h >= 4096) and the active columns fill their 4-column tiles at
 *   least half (images, MRAF noise boxes), the active set is rounded up to whole tiles and that kernel walks the tile
 *   list; results are those of the dense launch bit for bit.
 *   MRAF with a weight update runs ONE column pass with ONE inverse per column (round 6): the weights that enter an update are
 *   normalised, so ||w'||^2 = 1 + D, D = the sum over the signal pixels of w'^2 - w^2, which a forward-only pre-pass over the
 *   columns that hold signal pixels forms before the pass rebuilds the field (WGS-Leonardo / WGS-Kim without in-pass statistics;
 *   float32 and float64).  The first update after new weights or a new target -- and the other rules -- split the rebuilt field
 *   instead (its signal and noise part are transformed separately and joined by the row kernel once ||w'|| is known), or take
 *   two passes where neither form applies.
 * HGS_OPT_FORCE_STEPWISE (default 0): hgs_iterate / hgs_iterate_stats loop the three general operators
 *   (materialised farfield) even where a fused kernel exists -- the reference's own op sequence; used by tests.
 * HGS_OPT_TILE_KERNEL (default 1): use the tile-resident fused column kernels where they apply (fp32: col_tile_kernel at
 *   pad_h >= 4096, the half-width col_tile2_kernel at pad_h = 4096 and 2048); 0 forces the per-column kernel at every size.
 * HGS_OPT_SEPARABLE (default 1), HGS_OPT_SEPARABLE_MIN_SPOTS (default 96): kind 1, run the two transforms as
 *   complex GEMMs on the matrix cores when the basis and the grid factorise; 0 forces the direct kernels.
 * HGS_OPT_SEP_WORKGROUPS (default 0): kind 1, the workgroups of each of the two stream-K GEMMs (cgemm_streamk).  The line of
 *   tiles * KT k-steps of a GEMM is cut into G equal shares; 0 means G = min(2 * #CU, tiles * KT), a value v > 0 means
 *   G = min(v, 2 * #CU, tiles * KT) -- the schedule a device with fewer compute units (a partition) would run, which the
 *   tests use to reach every regime of the schedule at small shapes (a workgroup that walks whole tiles, ranges that cross
 *   or end on a tile boundary, several workgroups per tile).  Results under any two values differ only in how fp32 partial
 *   sums are grouped.  Negative values return HGS_ERR_ARG.  Set after the kernels were uploaded, the tables of the
 *   schedule and the two buffers of partial planes whose size follows it are rebuilt at once (the stream drains first).
 *   hgs_dispatch_read marks cgemm_streamk launches whose G the option holds below min(2 * #CU, tiles * KT) with `sk_cap`.
 *   Pinned by tests/test_streamk_gemm.py: under every value both transforms stay within 2e-5 (farfield) / 1e-4 (phase
 *   phasor) of float64 direct summation in every 128-wide output tile, a batch equals its single runs bit for bit, and
 *   0 after a cap gives the uncapped results back bit for bit; the schedule itself by tests/test_streamk_schedule.py.
 * HGS_OPT_RUN_KERNELS (default 1): kind 1, fp32, regular pixel grid and a phase polynomial of degree <= 2 (any basis of
 *   tilts, focus and astigmatisms, separable or not): the direct transforms advance exp(i phi) along runs of 16 pixels by
 *   a two-term recurrence instead of evaluating the polynomial, sin and cos per pixel; 0 forces the per-pixel kernels.
 * Options are per engine and take effect at the next call; nothing is read from the environment after
 * hgs_create (which reads the developer overrides once: the grid sizes HGS_ROW_BLOCKS / HGS_COL_BLOCKS / HGS_TILE_BLOCKS /
 * HGS_TILE2_BLOCKS / HGS_ROW_PREF_BLOCKS, and the A/B switches HGS_ROW_XCD, HGS_COL_XMAP, HGS_ROW_SHIFT, HGS_ROW_SHIFT64, HGS_ROW_PREF,
 * HGS_ROW_PREF_BATCH, HGS_TILE_RULE, HGS_MRAF_SPLIT, HGS_MRAF_SPLIT64, HGS_GH2_MASK, HGS_TILE_LIST, HGS_TILE_SHIFT16, HGS_TILE_NR4,
 * HGS_TILE2, HGS_TILE2_MIN_BATCH, HGS_TILE2_PHASE2, HGS_KEEP_G, HGS_FUSED_SHIFT, HGS_MONO_TAB, HGS_MRAF_PRESUM, HGS_PRESUM_ROWS,
 * HGS_PRESUM_BLOCKS, HGS_EMPTY_COL_LOADS, HGS_EMPTY_COL_INVERSE, HGS_EMPTY_COL_FORWARD,
 * HGS_EMPTY_COL_PREZERO, HGS_EMPTY_COL_LIST -- all default to the tuned path;
 * HGS_TRACE_INIT=1 prints where hgs_create spends its time).
 *   HGS_KEEP_G (default 1): the last row launch of a float32 hgs_iterate call leaves G of the next body behind, and the next
 *   call -- or hgs_nearfield2farfield -- on an unchanged phase starts from it.  That G is the loop's own un-rounded phasor
 *   amp * nf / |nf|, not exp(i * HGS_PHASE) of the rounded, stored phase: the trailing transform is consistent with the loop
 *   (a loop cut into calls walks bit for bit like one call) rather than bit-identical with a fresh engine given the
 *   downloaded phase; the two agree to float32 rounding (tests/test_gpu_round6.py, 2e-6 on the farfield).
 * HGS_OPT_EMPTY_COL_LOADS (default 1; HGS_EMPTY_COL_LOADS in the environment): dense launches of the half-width kernel on a target
 *   with few active columns (a spot array with HGS_OPT_SPARSE_COLUMNS = 0; 4096 rows, SLM rows within five register slots, one
 *   hologram or a batch) request weights and targets only in the columns
 *   where the column scan found any; every other column reads as the zeros it holds without a fetch.  Results are the same
 *   bit for bit; 0 fetches every column (the tests' A/B reference).
 * HGS_OPT_EMPTY_COL_INVERSE (default 1; HGS_EMPTY_COL_INVERSE in the environment): in those launches a column the scan found
 *   empty also skips the weight rule and its inverse transform -- the constrained column is exactly zero, so is its inverse --
 *   and writes zeros into H.  The forward transform of every column still runs.  HGS_PHASE and HGS_WEIGHTS are the same bit for
 *   bit; 0 runs every inverse while the flags still go with the launch (the tests' A/B reference).
 * HGS_OPT_EMPTY_COL_FORWARD (default 1; HGS_EMPTY_COL_FORWARD in the environment): where HGS_OPT_EMPTY_COL_INVERSE acts, an empty
 *   column is not transformed forward either -- in these launches only the column's own weight rule reads its farfield, and
 *   that rule is skipped.  A half tile whose two columns are both empty requests no G rows, touches no LDS and passes no
 *   barrier: it only stores its zeros into H.  Every column of H is still written.  It rests on the inverse skip: with
 *   HGS_OPT_EMPTY_COL_INVERSE = 0 it does nothing.  hgs_dispatch_read marks the launches that skip with `zero_fwd`.
 *   HGS_PHASE and HGS_WEIGHTS are the same bit for bit; 0 loads and transforms every column (the tests' A/B reference).
 * HGS_OPT_EMPTY_COL_PREZERO (default 1; HGS_EMPTY_COL_PREZERO in the environment): where HGS_OPT_EMPTY_COL_FORWARD acts and the
 *   body is nothing but that column launch and its row launch, the zeros of the empty columns are written by the ROW launch that
 *   closes the body before: it stores zero instead of G in the columns the scan found empty (`zero_mask` in hgs_dispatch_read
 *   -- the same stores, one select each), and the column launch walks from one non-empty half tile to the next without touching
 *   the empty ones (`prezero`).  Inside one hgs_iterate call only: the first body of a call runs the plain form, the last row
 *   launch of a call leaves G of every column as before, so calls of a single body gain nothing.  HGS_PHASE and HGS_WEIGHTS are
 *   the same bit for bit; 0 has every column launch store its zeros itself (the tests' A/B reference).
 * HGS_OPT_EMPTY_COL_LIST (default 1; HGS_EMPTY_COL_LIST in the environment): where HGS_OPT_EMPTY_COL_PREZERO acts, the column
 *   launch walks the POSITIONS of the ascending list of 4-column tiles that hold anything (built on the device with the column
 *   scan) instead of every tile: pair i of workgroups takes list entries i, i + pairs, ..., so that 32 spot tiles go to 32
 *   pairs wherever they sit in the farfield (`tile_list` in hgs_dispatch_read); a workgroup without an entry returns at once.
 *   The weight norm of these launches is summed per half tile (one slot per hologram, tile, half and wave, folded by the row
 *   launch in a fixed order), so HGS_PHASE and HGS_WEIGHTS are the same bit for bit with the option off, and for every grid
 *   HGS_TILE2_BLOCKS asks for; 0 keeps the static walk over all tiles (the tests' A/B reference).
 * HGS_OPT_ROCTX (default 0): roctx ranges (hgs_iterate, hgs_nearfield2farfield, hgs_farfield_constraint,
 *   hgs_farfield2nearfield) for rocprofv3 --marker-trace; the roctx library is dlopen'ed on first use.
 * HGS_OPT_KEEP_PREV_PHASE (default 0): a fused hgs_iterate / hgs_iterate_stats call of ONE iteration that rewrites the
 *   farfield phase (i.e. does not use a fixed one) first copies HGS_PHASE to HGS_PHASE_PREV on the device.  The fused
 *   kernels never materialise Hologram.phase_ff (= atan2 of the farfield the iteration STARTED from, _hologram.py:1583 /
 *   :1602); a caller that runs the loop one iteration per call -- Hologram.optimize(callback=...) -- can rebuild it on
 *   demand from that phase (hgs_nearfield2farfield(store_phase_ff = 1) on a second engine).  Calls that iterate the
 *   general operators keep HGS_PHASE_FF itself up to date and hold no previous phase. */
enum { HGS_OPT_SPARSE_COLUMNS = 1, HGS_OPT_FORCE_STEPWISE = 2, HGS_OPT_TILE_KERNEL = 3, HGS_OPT_SEPARABLE = 4,
       HGS_OPT_SEPARABLE_MIN_SPOTS = 5, HGS_OPT_ROCTX = 6, HGS_OPT_RUN_KERNELS = 7, HGS_OPT_KEEP_PREV_PHASE = 8,
       HGS_OPT_EMPTY_COL_LOADS = 9, HGS_OPT_SEP_WORKGROUPS = 10,
       HGS_OPT_EMPTY_COL_INVERSE = 11, HGS_OPT_EMPTY_COL_FORWARD = 12, HGS_OPT_EMPTY_COL_PREZERO = 13,
       HGS_OPT_EMPTY_COL_LIST = 14 };
int hgs_set_option(hgs_engine* e, int option, int value);

/* Timing support for bench.py: per-kernel HIP-event timing on the engine stream. */
enum { HGS_K_ROW = 0, HGS_K_COL_FUSED = 1, HGS_K_COL_FWD = 2, HGS_K_COL_INV = 3, HGS_K_ELEMENTWISE = 4,
       HGS_K_CG_SEED = 5 /* cg_seed_kernel + its loss reduction */, HGS_K_CG_ADAM = 6 /* cg_adam_kernel */,
       HGS_K_COUNT = 7 };
int hgs_profile_enable(hgs_engine* e, int on);
/* out[HGS_K_COUNT][2] = {total milliseconds, launches} since the last call; syncs the stream.  The table grew from 5 to
 * 7 rows with hgs_cg_iterate: a caller sizes its buffer by HGS_K_COUNT of the header it was BUILT against, so one built
 * against the five-row header must be rebuilt before it runs on this library (version "hgs 0.2") */
int hgs_profile_read(hgs_engine* e, double* out);
/* elapsed milliseconds of hgs_iterate(step, n_iter) measured with a HIP event pair on the engine
 * stream (SURVEY 8d timing protocol) */
int hgs_iterate_timed(hgs_engine* e, hgs_step* step, int n_iter, double* ms);

/* Dispatch record: which kernel template instance each launch of this engine went to since the previous call, one line
 * per (instance, run-time flags):
 *     "col_tile_kernel<R=float,N=4096,PHASE=0,NR=6,STATS=false,EXTRAS=false,RULE=1,LISTED=0> xmap\t50\n"
 * (family, its template arguments by name -- the ones rocprofv3 prints positionally --, flags list / load_mask /
 * store_mask / xmap / batch / stats / nf_out / ..., launch count).  Families: row_kernel, col_kernel, col_fused_kernel,
 * col_tile_kernel, bluestein_lines, c_n2f_run, c_f2n_run, c_n2f_partial, c_f2n, cgemm_streamk, cg_seed_kernel, cg_adam_kernel,
 * vortex_find_kernel, vortex_remove_kernel, phase_display_kernel, poly_kernel, pattern_kernel
 * (the small element-wise / reduction helpers are not recorded).  The tests assert it next to the numbers: neighbouring variants often agree to
 * the last bit, so only this shows that a policy reached the kernel it names.  `needed` (optional) receives the bytes
 * the text takes including the terminator; with buf = NULL and nbytes = 0 the call is a size query and keeps the record,
 * otherwise a buffer that is too small fails with HGS_ERR_ARG (record kept) and success clears the record. */
int hgs_dispatch_read(hgs_engine* e, char* buf, size_t nbytes, size_t* needed);

const char* hgs_last_error(void);
/* library / device identification: "hgs <version> gfx950 <device name>" */
const char* hgs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HGS_H */
