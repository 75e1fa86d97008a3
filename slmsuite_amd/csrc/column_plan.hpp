// What one iteration of the fused loop launches, decided in one place: plan_column_pass() maps plain facts (geometry,
// the iteration's flags, the A/B switches, the column counts of the last scan) to the launches of the column pass and
// what the row launch after it must do (plan_row_close()).  Pure host C++ -- no HIP, no engine state, no device -- so that the table can be
// read here and tested without a GPU (tests/test_column_plan.py); Engine::iterate() fills the facts, acquires what the
// plan lists and executes it.
#pragma once
#include <algorithm>

#include "../../include/hgs.h"

namespace hgs {

// Every switch hgs_create reads from the environment (in the order include/hgs.h lists them) plus the two column
// policies of hgs_set_option.  All default to the tuned path.
struct Tuning {
    int row_blocks = 0, col_blocks = 0, tile_blocks = 0;   // HGS_ROW_BLOCKS, HGS_COL_BLOCKS, HGS_TILE_BLOCKS: workgroup caps of the launches
    int tile2_blocks = 0;       // HGS_TILE2_BLOCKS: workgroups of the half-width tile kernel over the batch (0 = 3 x / 2 x #CU)
    int row_pref_blocks = 0;    // HGS_ROW_PREF_BLOCKS: workgroups of the prefetching row kernel
    int row_xcd = 1;            // HGS_ROW_XCD=0: XCD-aware row mapping off
    int col_xmap = 1;           // HGS_COL_XMAP=0: XCD-aware mapping of the per-column kernel's passes off (dense and column-list launches)
    int row_shift = 1;          // HGS_ROW_SHIFT=0: shifted row kernel off
    int row_shift64 = 1;        // ... in float64 (HGS_ROW_SHIFT64=0; round 5)
    int row_pref = 1;           // HGS_ROW_PREF=0: prefetching row kernel off
    int row_pref_batch = 0;     // HGS_ROW_PREF_BATCH=1: ... also for a batch
    int tile_rule = 1;          // HGS_TILE_RULE=0: rule-specialised tile kernels off
    int mraf_split = 1;         // HGS_MRAF_SPLIT=0: MRAF weight updates in two column passes
    int mraf_split64 = 1;       // HGS_MRAF_SPLIT64=0: float64 MRAF weight updates in two passes
    int gh2_mask = 1;           // HGS_GH2_MASK=0: noise part stored / read for every column
    int tile_list = 1;          // HGS_TILE_LIST=0: column lists always go to the per-column kernel
    int tile_shift16 = 1;       // HGS_TILE_SHIFT16=0: the tile kernel shifts by whole register slots
    int tile_nr4 = 1;           // HGS_TILE_NR4=0: slot-count instances of the rule kernels off (NR = 6 only)
    int tile2 = 1;              // HGS_TILE2=0: half-width tile kernel off
    int tile2_min_batch = 1;    // ... smallest batch that runs it at 4096 rows (HGS_TILE2_MIN_BATCH)
    int tile2_phase2 = 1;       // ... its phase-reading form at 4096 rows, one hologram (HGS_TILE2_PHASE2=0: col_tile_kernel)
    int keep_g = 1;             // HGS_KEEP_G=0
    int fused_shift = 1;        // HGS_FUSED_SHIFT=0: float64 per-column kernel unshifted (16 slots)
    int mono_tab = 1;           // HGS_MONO_TAB=0: per-pixel compressed kernels evaluate every monomial per spot
    int mraf_presum = 1;        // HGS_MRAF_PRESUM=0: the two-inverse split form on every update
    int presum_rows = 1;        // HGS_PRESUM_ROWS=0
    int presum_blocks = 0;      // HGS_PRESUM_BLOCKS: workgroups of the pre-pass (0 = tuned)
    int empty_col_loads = 1;    // HGS_EMPTY_COL_LOADS=0 / HGS_OPT_EMPTY_COL_LOADS: the half-width tile kernel fetches weights and targets of
                                // every column, also of those the scan found empty (the tests' A/B reference)
    int empty_col_inverse = 1;  // HGS_EMPTY_COL_INVERSE=0 / HGS_OPT_EMPTY_COL_INVERSE: ... and runs the rule block and the inverse transform
                                // of those columns as well (the flags still go with the launch)
    int empty_col_forward = 1;  // HGS_EMPTY_COL_FORWARD=0 / HGS_OPT_EMPTY_COL_FORWARD: ... and, where the inverse is skipped, loads and
                                // transforms them forward although nothing reads the result (acts only with empty_col_inverse)
    int empty_col_prezero = 1;  // HGS_EMPTY_COL_PREZERO=0 / HGS_OPT_EMPTY_COL_PREZERO: ... and, where the forward transform is skipped, every
                                // body of a call stores the zeros of the empty columns itself instead of finding them left by the row
                                // launch before it (acts only with empty_col_forward; ColumnPlan::accepts_prezeroed)
    int empty_col_list = 1;     // HGS_EMPTY_COL_LIST=0 / HGS_OPT_EMPTY_COL_LIST: ... and, where it finds them left, a workgroup
                                // keeps its static walk over ALL tiles instead of walking the positions of the list of tiles that
                                // hold anything (acts only with empty_col_prezero; EmptyCols::list_walk)
    int sparse = 1;             // HGS_OPT_SPARSE_COLUMNS
    int tile = 1;               // HGS_OPT_TILE_KERNEL (0 forces the per-column kernel at every size: the tests' A/B reference)
};

// flag evolution of _gs_farfield_routines (:1552-1585): what this iteration must do
struct Plan { int do_update, use_fixed, store_phase; };

struct PassFacts {
    int elem = 4;                   // sizeof(R)
    int Ph = 0, Pw = 0, B = 1, n_cu = 256, col_blocks = 1, tile_blocks = 1, r0 = 0, Sh = 1;
    Plan it{0, 0, 0};
    int method = HGS_GS, mraf_enabled = 0, zero_mode = 0;      // of the hgs_step
    int stat_groups = 0;            // hgs_iterate_stats drives the loop: its group mask (0: no statistics)
    bool w_unit = false;            // the stored weights are normalised by wscale (Engine::w_unit)
    bool sparse_enabled = false;    // the column pass walks the list of active columns
    bool sparse_tiles = false, sparse_dirty = true;
    bool gh_prezeroed = false;      // the row launch before this body, in this call, stored the zeros of the empty columns instead of
                                    // their G (RowClose::zero_par of the body before)
    bool w_outside_scan = false;    // a kernel that the scan does not see may have written a weight into a column it found empty
                                    // (the N-vector rule of the spot feedback modes writes at the spot pixels, whatever the target holds)
    int n_active_min = 0, n_active_max = 0, n_noise_max = 0, n_signal_max = 0;
    bool ffb_unavailable = false;   // the device could not give the farfield buffer of the float64 split form
    Tuning tun;
};

// one value per launcher entry point of launch.hpp
enum class ColFamily { fused, fused_rule1, fused_rule2, fused_stats, tile, tile_rule, tile_rule_listed, tile_stats,
                       tile_extras, tile_extras_stats, tile_split, tile_split_stats, tile_presum, tile2 };

// How a launch of col_tile2_kernel treats the columns the scan found empty: a ladder, each level on only where the one before
// it is, and none without the scan's flags (ColLaunch::col_flags).  One switch of Tuning::empty_col_* per level.
struct EmptyCols {
    bool skip_inverse = false;      // no rule block and no inverse transform (ColArgs::zero_inv)
    bool skip_forward = false;      // ... no load and no forward transform either; an empty half tile only stores zeros (zero_fwd)
    bool prezeroed = false;         // ... the zeros are in place already, empty half tiles are walked past (h_prezeroed)
    bool list_walk = false;         // ... along the scan's list of the tiles that hold anything (tile_list)
};

struct ColLaunch {
    ColFamily family = ColFamily::fused;
    int phase_mode = 0;   // 0 = phase taken from the field, 1 = ... and stored, 2 = stored phase used
    // RULE the launch asks for: 0 generic, 1 WGS-Leonardo / WGS-Kim update, 2 no update; tile_split: 3 (with rule_ok the launcher
    // takes RULE 4 for a listed Leonardo / Kim update); tile_presum: 5 (update with the pre-summed scale) or 6 (MRAF, no update)
    int rule = 0, rule_ok = 0;
    int nr = 0, shift = 0;          // tile families: register slots of the SLM rows, row shift
    int grid = 0;                   // workgroups per hologram
    bool listed = false, list_xmap = false, half_xmap = false, few_active = false, gh2_sparse = false, col_flags = false;
    EmptyCols empty;                // (tile2 only)
    // weight-norm partials one slot per (hologram, tile, half, wave) in a buffer of their own (ColArgs::wslots, tile_flags.hpp)
    // instead of one per workgroup in wpartial, so that the sum no longer depends on which workgroup took which half tile
    // (tile2 only); the row launch behind it folds them (RowClose::wslot_fold)
    bool wslots = false;
    bool nog_pass = false, use_nog = false, weights_only = false, split64 = false;
    int do_update = 0;
    int stats = 0;                  // ColArgs::do_stats: statistics groups this launch accumulates
    int n_dpartial = 0;             // partials of the pre-pass it folds (0: none)
};

enum class RowJoin { none, gh2, gh2_noise_only };

struct ColumnPlan {
    bool dilated_forward = false;   // "computational_spot" statistics on a column list: amp_ff of the dilated spot columns first
    bool nog = false;               // WGS-Nogrette: the forward-only pass that sums feedback / target
    ColLaunch nog_pass;
    bool presum = false, presum_col = false;   // pre-pass of the single-inverse MRAF update: tile kernel / per-column over the signal list
    int prepass_grid = 0, prepass_nr = 0, prepass_shift = 0;
    bool prepass_list_xmap = false;
    ColLaunch main;
    bool scale_after_main = false;  // reduce_to_scale between the main pass and what follows
    bool second_pass = false;       // the two-pass form
    ColLaunch second;
    int noise_inverse_grid = 0;     // float64 split: inverse-only launch over the noise columns (0: none)
    // the row launch that closes the iteration
    bool finalize = false;
    RowJoin join = RowJoin::none;
    bool gh2_mask = false;          // ... the joining launch reads gh2 in the noise columns only
    int last_mode = 1;              // MODE of the call's last row launch: 3 also leaves G of the next body behind
    int wpartial_n = 0;             // partials the last column launch left (weight norm; statistics)
    // The row launch BEFORE this body may store the zero H of the empty columns instead of their G (RowClose::zero_par) and the
    // main launch then walks past empty half tiles (main.empty.prezeroed): the half-width kernel with the scan's flags (a current
    // scan, no weight written behind it, no column list, at most five slots: column_launch), the instance that reads them (PHASE 0,
    // 4096 rows), every empty-column switch up to empty_col_prezero on, and nothing else in the body that reads or writes gh -- no
    // second pass, Nogrette sum, pre-pass or in-pass statistics
    bool accepts_prezeroed = false;
    // buffers the plan needs
    bool need_gh2 = false, need_ffb = false, need_dpartial = false, need_nog_dev = false;
};

// ---- geometry ------------------------------------------------------------------------------------------------------
// the tile-resident fused column kernel applies: fp32, 4096 / 8192 rows, the SLM rows within six register slots
// (the kernel shifts its transform input by tile_shift() rows -- any multiple of 16 keeps the shift-theorem factor a
//  per-lane constant -- so the SLM rows start in the first 16 rows of register slot 0)
inline int tile_shift(const PassFacts& f) { return f.tun.tile_shift16 ? (f.r0 / 16) * 16 : (f.r0 / (f.Ph / 16)) * (f.Ph / 16); }
inline int tile_slots(const PassFacts& f) { const int Tc = f.Ph / 16; return (f.r0 - tile_shift(f) + f.Sh + Tc - 1) / Tc; }
inline bool tile_geometry_ok(const PassFacts& f) {
    if (f.elem != 4 || f.Ph < 4096 || !f.tun.tile) return false;
    return tile_slots(f) <= 6;
}
// columns a workgroup pass of the column kernels handles side by side (ColCfg<N>::CPAR)
inline int col_cpar(int Ph) {
    const int T = Ph / 16;
    return T >= 256 ? 1 : std::min(4, 256 / T);
}
inline int list_blocks(const PassFacts& f, int n_list) { return std::max(1, std::min((n_list + col_cpar(f.Ph) - 1) / col_cpar(f.Ph), f.n_cu * 3)); }
// fewer than four columns per workgroup pass: the groups of a 4-column run of the list on one XCD (they share 32-byte tile
// rows where the active set is dense; ColArgs::list_xmap) -- the grid becomes a whole number of such groups
inline int list_xcd_round(const PassFacts& f, int blocks, bool* xmap) {
    const int gp = 8 * (4 / col_cpar(f.Ph));
    *xmap = f.tun.col_xmap && col_cpar(f.Ph) < 4 && blocks >= gp;
    return *xmap ? blocks - blocks % gp : blocks;
}
// slot counts the half-width tile kernel is compiled for (tile2_has() of launch_tile2_f32.hip)
inline int tile2_max_slots(int Ph) { return Ph == 4096 ? 6 : Ph == 2048 ? 10 : 0; }

// a plain pass: Leonardo / Kim update or none; no statistics, MRAF, Nogrette sum or forward-only pass
inline bool plain_pass(const ColLaunch& l, const PassFacts& f) {
    return !l.stats && !f.mraf_enabled && !l.nog_pass && !l.weights_only && !l.use_nog;
}
inline bool power_rule(int method) { return method == HGS_WGS_LEONARDO || method == HGS_WGS_KIM; }

// half-width tile-resident kernel (col_tile2_kernel): the grid it runs on, or 0 where it does not apply -- fp32, a dense
// launch of a plain pass, and
//   4096 rows: a batch (>= HGS_TILE2_MIN_BATCH holograms), farfield phase neither stored nor read (PHASE 0: the
//              phase-storing instances do not fit 168 registers; one hologram also reads a stored phase), SLM rows within
//              six slots -- 3 x #CU workgroups over the batch, a multiple of 16 per hologram so that the two halves of a
//              tile run on one XCD together;
//   2048 rows: SLM rows within ten slots -- 2 x #CU workgroups of two lane groups, one tile each at a time.
inline int tile2_grid(const PassFacts& f, bool tile_path, const ColLaunch& l) {
    const Tuning& t = f.tun;
    if (f.elem != 4 || !t.tile2 || !t.tile || f.sparse_enabled || !t.tile_rule || !plain_pass(l, f)) return 0;
    if (l.do_update && !power_rule(f.method)) return 0;
    if (tile_slots(f) > tile2_max_slots(f.Ph)) return 0;
    // the developer override HGS_TILE2_BLOCKS never exceeds what wpartial / the statistics partials are sized for
    // (B * max(col_blocks, tile_blocks, 3 * #CU) entries) nor the number of half tiles there are
    const int want = t.tile2_blocks > 0 ? std::min(t.tile2_blocks, 3 * f.n_cu) : 0;
    if (f.Ph == 4096) {
        if (f.B < t.tile2_min_batch || (l.phase_mode != 0 && !(l.phase_mode == 2 && t.tile2_phase2 && f.B == 1)) || !tile_path) return 0;
        const int per = (want > 0 ? want : 3 * f.n_cu) / f.B;
        return std::min(std::max(16, per / 16 * 16), std::max(16, f.Pw / 2 / 16 * 16));
    }
    if (f.Ph == 2048) return std::max(1, std::min(f.Pw / 4, (want > 0 ? want : 2 * f.n_cu) / f.B));
    return 0;
}

// per-column fused launch: rule-specialised kernel where the pass is plain (fp32)
inline void fused_family(const PassFacts& f, ColLaunch& l) {
    l.family = ColFamily::fused;
    l.rule = 0;
    if (l.stats) l.family = ColFamily::fused_stats;
    else if (f.elem == 4 && plain_pass(l, f) && f.tun.tile_rule) {
        if (!l.do_update) { l.family = ColFamily::fused_rule2; l.rule = 2; }
        else if (power_rule(f.method)) { l.family = ColFamily::fused_rule1; l.rule = 1; }
    }
}

// ---- the forms an MRAF weight update can take ----------------------------------------------------------------------
// MRAF with a weight update takes two passes over the columns: the rebuilt field mixes the NORMALISED weights (signal
// region) with the un-weighted farfield (noise region), so ||w'|| has to be known first.  Pass 0: forward transform +
// weight update (+ statistics), no inverse; then wscale = 1/||w'||; pass 1: forward transform again, rebuild, inverse.
struct MrafForms {
    bool two_pass, tile_path;
    // ... unless the tile-resident kernel runs the column pass: the inverse transform is linear, so it transforms the
    // signal part (un-normalised new weights) and the noise part separately in ONE pass and the row kernel joins
    // them once ||w'|| is known (col_tile_kernel RULE 3, row_kernel SPLIT)
    bool split;
    // ... and the float64 per-column kernel the same way, its noise part through a farfield buffer and an inverse-only
    // launch over the columns that hold noise (CParams::split): one forward transform and one read of weights and
    // target per column instead of two
    // (float32 too where the tile-resident kernel does not run: SLM rows over more than six register slots, short columns)
    // (not where the single-inverse form below takes the update: presum_ok)
    bool split64;
    // ... and with ONE inverse per column where ||w'|| can be had BEFORE the field is rebuilt (round 6): the weights that
    // enter this update are normalised (w_unit), so ||w'||^2 = 1 + D, D = sum over the signal pixels of w'^2 - w^2, which a
    // forward-only pre-pass over the columns that hold signal pixels forms (col_presum_kernel; a quarter of the columns
    // at cfg 5).  The main pass (col_tile_kernel RULE 5) rebuilds with the final scale: no second inverse in the noise
    // columns, no noise part parked in LDS, nothing for the row kernel to join.  WGS-Leonardo / WGS-Kim without in-pass
    // statistics; the first update after new weights or a new target (and every other rule) takes the split form.
    bool presum;
    // ... and everywhere else the fused path runs an MRAF update (float64; float32 geometries outside the tile-resident
    // kernel's or narrower than 4096 columns): the per-column kernel makes the pre-pass over the list of signal columns
    // (CParams::presum) and the main pass -- per-column or the generic tile kernel -- rebuilds with the pre-summed scale.
    // Replaces the float64 split form (pass + inverse-only launch over the noise columns + joining row launch) and the
    // two-pass form.
    bool presum_col;
};
// before the column counts are consulted: split64 / presum_col say which list the form reads
inline MrafForms mraf_forms(const PassFacts& f) {
    const Tuning& t = f.tun;
    MrafForms m{};
    m.two_pass = f.mraf_enabled && f.it.do_update;
    // (a column list rounded to whole tiles: the same kernels walk the list)
    m.tile_path = (!f.sparse_enabled || f.sparse_tiles) && tile_geometry_ok(f);
    m.split = m.two_pass && m.tile_path && f.Pw >= 4096 && t.mraf_split;
    const bool split64_ok = m.two_pass && !m.tile_path && f.Pw >= 4096 && t.mraf_split && t.mraf_split64;
    const bool presum_ok = m.two_pass && t.mraf_presum && f.w_unit && !f.stat_groups && power_rule(f.method);
    m.split64 = split64_ok && !presum_ok;
    m.presum = presum_ok && m.split && f.elem == 4;
    m.presum_col = presum_ok && !m.presum;
    return m;
}

// The column scans a form consults (each a device launch plus a host sync when the weights or the target moved since the
// last one): asked from the facts known without them, run by the caller BEFORE plan_column_pass(), whose choice their counts
// feed -- the noise columns for the float64 split form, the signal columns for the per-column pre-pass, the column flags for
// the tile pre-pass.
struct Scans { bool noise, signal, flags; };
inline Scans scans_needed(const PassFacts& f) {
    const MrafForms m = mraf_forms(f);
    return Scans{m.split64, m.presum_col, m.presum};
}

// ---- the planner's own predicates on a launch / a plan (column_launch() and plan_column_pass() store what they say in
// ColLaunch::wslots, ColumnPlan::accepts_prezeroed and EmptyCols::list_walk; the engine reads those fields, never these) ----
// the updating launches of the instances of col_tile2_kernel that can receive column flags (WTBUF: 4096 rows, at most five
// slots, PHASE 0; the register form of a batch or the parked few-active form of one hologram -- launch_tile2_n picks by
// exactly these facts)
inline bool wslots_ok(const ColLaunch& l, const PassFacts& f) {
    if (f.elem != 4 || f.Ph != 4096 || l.family != ColFamily::tile2) return false;
    if (l.phase_mode != 0 || l.nr > 5 || !l.do_update) return false;
    return f.B > 1 || l.few_active;
}
// ColumnPlan::accepts_prezeroed (see there), of a plan whose launches and row join are set
inline bool prezero_ok(const ColumnPlan& cp, const PassFacts& f) {
    const Tuning& t = f.tun;
    const ColLaunch& l = cp.main;
    if (f.elem != 4 || f.Ph != 4096) return false;
    if (l.family != ColFamily::tile2 || !l.col_flags || l.phase_mode != 0) return false;
    if (!t.empty_col_inverse || !t.empty_col_forward || !t.empty_col_prezero) return false;
    if (cp.second_pass || cp.nog || cp.presum || cp.presum_col || cp.dilated_forward || cp.noise_inverse_grid || l.stats || f.stat_groups) return false;
    return cp.join == RowJoin::none;
}
// ... and the launch that finds the zeros walks the positions of the scan's tile list instead of every tile
inline bool tile_list_ok(const ColumnPlan& cp, const PassFacts& f) { return prezero_ok(cp, f) && f.tun.empty_col_list != 0; }

// one launch of the main column pass: pass -1 = the Nogrette sum, 0 = the main launch, 1 = the second pass of the two-pass form
inline ColLaunch column_launch(const PassFacts& f, const MrafForms& m, const ColumnPlan& cp, int pass) {
    const Tuning& t = f.tun;
    const bool sp = f.sparse_enabled;
    const bool plain_two_pass = m.two_pass && !m.split && !m.split64 && !m.presum_col;
    ColLaunch l;
    l.phase_mode = f.it.use_fixed ? 2 : (f.it.store_phase ? 1 : 0);
    l.do_update = f.it.do_update;
    l.shift = tile_shift(f);
    l.nr = tile_slots(f);
    if (pass == -1) {                 // Nogrette: sum of fc only
        l.nog_pass = l.weights_only = true;
        l.phase_mode = 0;
    } else if (cp.nog) {
        l.use_nog = true;
    }
    if (plain_two_pass && pass == 0) {
        l.weights_only = true;
        l.phase_mode = 0;
    }
    if (m.presum_col) l.n_dpartial = cp.prepass_grid;
    if (m.split64 && pass == 0) l.split64 = true;
    if (m.two_pass && pass == 1) l.do_update = 0;
    if (f.stat_groups && pass == 0 && (!sp || (f.stat_groups & 1)))
        l.stats = sp ? (f.stat_groups & 1) : f.stat_groups;       // sparse: amp_ff already stored
    l.listed = sp;
    l.grid = f.col_blocks;
    const int tile_grid = sp ? std::max(1, std::min(f.tile_blocks, f.n_active_max / 4)) : f.tile_blocks;
    if (sp && !m.tile_path) {
        l.grid = list_xcd_round(f, list_blocks(f, f.n_active_max), &l.list_xmap);
        fused_family(f, l);
    } else if (m.presum && pass == 0) {
        l.family = ColFamily::tile_presum;
        l.rule = 5;
        l.grid = tile_grid;
        l.n_dpartial = cp.prepass_grid;
        l.col_flags = sp;
    } else if (m.split && pass == 0) {
        l.family = l.stats ? ColFamily::tile_split_stats : ColFamily::tile_split;
        l.rule = 3;
        l.rule_ok = t.tile_rule;
        l.grid = tile_grid;
        l.gh2_sparse = t.gh2_mask && !f.sparse_dirty && !sp;      // (set together with the row launch's gh2_mask)
        l.col_flags = sp;       // (scanned with the weights / target this loop started from)
    } else if (const int t2 = tile2_grid(f, m.tile_path, l)) {
        // half-width tile-resident kernel: batches at 4096 rows (three workgroups per CU), dense launches at
        // 2048 rows (col_tile2_kernel); plain passes only
        l.family = ColFamily::tile2;
        l.rule = l.do_update ? 1 : 2;
        l.grid = t2;
        l.few_active = !f.sparse_dirty && f.n_active_min > 0 && f.n_active_max * 4 <= f.Pw;
        // ... and the scan's column flags go with it: weights / targets are requested only in the columns that hold any
        // (current scan only -- every writer of either array outside the column kernels marks it dirty or is named above)
        // (4096 rows, at most five slots: the instances of col_tile2_kernel that read them, WTBUF)
        l.col_flags = l.few_active && f.Ph == 4096 && l.nr <= 5 && t.empty_col_loads && !f.w_outside_scan;
        l.half_xmap = f.Ph >= 4096 && t2 % 16 == 0;
        l.empty.skip_inverse = l.col_flags && t.empty_col_inverse;
        l.empty.skip_forward = l.empty.skip_inverse && t.empty_col_forward;
        l.wslots = wslots_ok(l, f);
    } else if (m.tile_path) {
        l.grid = tile_grid;
        const bool extras = f.mraf_enabled || l.nog_pass || l.weights_only;
        // MRAF without a weight update (GS, iteration 0, the no-update bodies of WGS): the rule-free MRAF form
        // compiled per slot count (col_tile_kernel RULE 6) instead of the generic six-slot instance
        const bool mraf_plain = f.mraf_enabled && !l.do_update && !l.nog_pass && !l.weights_only && !l.stats &&
                                t.tile_rule && t.mraf_presum && f.elem == 4 && !f.zero_mode;
        if (mraf_plain) {
            l.family = ColFamily::tile_presum;
            l.rule = 6;
            l.col_flags = sp;
        } else if (extras) {
            l.family = l.stats ? ColFamily::tile_extras_stats : ColFamily::tile_extras;
        } else {
            // the hot launches: weight rule compiled in (col_tile_kernel RULE) where it is the
            // Leonardo / Kim update or no update at all
            const int rule = !t.tile_rule ? 0 : !l.do_update ? 2 : power_rule(f.method) ? 1 : 0;
            if (l.stats) l.family = ColFamily::tile_stats;
            else if (rule != 0) {
                l.family = sp ? ColFamily::tile_rule_listed : ColFamily::tile_rule;
                l.rule = rule;
                if (!t.tile_nr4) l.nr = 6;
            } else l.family = ColFamily::tile;
        }
    } else {
        fused_family(f, l);
    }
    return l;
}

inline ColumnPlan plan_column_pass(const PassFacts& f) {
    const Tuning& t = f.tun;
    const bool sp = f.sparse_enabled;
    MrafForms m = mraf_forms(f);
    ColumnPlan cp;
    // (a column list: only where at most half of the listed columns hold noise -- where every one does, as around a noise
    //  box, the single pass saves no transform and pays the extra launch: measured 119 against 105 us at 4096^2)
    if (m.split64 && sp && f.n_noise_max * 2 > f.n_active_max) m.split64 = false;
    // (a farfield-sized buffer more: 268 MB per float64 hologram at 4096^2.  Where the device cannot give it the
    //  update runs in two passes as it did before round 4 -- slower, same results -- instead of failing the call)
    if (m.split64 && f.ffb_unavailable) m.split64 = false;
    // (a target without a single finite non-zero pixel: D = 0 trivially, but nothing to gain either -- two plain passes)
    if (m.presum_col && f.n_signal_max <= 0) m.presum_col = false;
    cp.presum = m.presum;
    cp.presum_col = m.presum_col;
    cp.prepass_shift = tile_shift(f);
    cp.prepass_nr = tile_slots(f);
    if (m.presum) {
        // (the pre-pass' grid: one workgroup per CU slot it can hold)
        cp.prepass_grid = std::max(1, std::min(f.Pw / 4, (t.presum_blocks > 0 ? std::min(t.presum_blocks, 3 * f.n_cu)
                                                                              : (f.Ph >= 8192 ? 1 : 2) * f.n_cu) / f.B));
    } else if (m.presum_col) {
        // (no more workgroups than the dense launch of this geometry keeps resident: at 8192 rows in float64 one per CU --
        //  the list over three rounds of workgroups cost the pre-pass a prologue per round)
        const int blocks = std::max(1, std::min(list_blocks(f, f.n_signal_max), t.presum_blocks > 0 ? t.presum_blocks : f.col_blocks));
        // (the signal columns of an image fill their tiles)
        cp.prepass_grid = list_xcd_round(f, blocks, &cp.prepass_list_xmap);
    }
    cp.dilated_forward = sp && (f.stat_groups & 2);
    // WGS-Nogrette needs nanmean(feedback / target) over the whole farfield before the update (:1851):
    // one more forward-only pass that just accumulates it
    cp.nog = f.method == HGS_WGS_NOGRETTE && f.it.do_update;
    cp.second_pass = m.two_pass && !m.split && !m.split64 && !m.presum_col;
    if (cp.nog) cp.nog_pass = column_launch(f, m, cp, -1);
    cp.main = column_launch(f, m, cp, 0);
    if (cp.second_pass) cp.second = column_launch(f, m, cp, 1);
    // (the single-inverse pass needs wscale only from the NEXT column launch on: the row launch folds the
    //  partials, as after a plain update -- one 4.7 us launch less per iteration)
    cp.scale_after_main = m.two_pass && !m.presum && !m.presum_col;
    cp.noise_inverse_grid = (m.split64 && f.n_noise_max > 0) ? list_blocks(f, f.n_noise_max) : 0;
    cp.wpartial_n = cp.second_pass ? cp.second.grid : cp.main.grid;
    // the row kernel that follows folds the weight-norm partials into wscale (unless already done)
    cp.finalize = f.it.do_update != 0 && (!m.two_pass || m.presum || m.presum_col);
    cp.join = cp.main.split64 ? RowJoin::gh2_noise_only
              : (cp.main.family == ColFamily::tile_split || cp.main.family == ColFamily::tile_split_stats) ? RowJoin::gh2 : RowJoin::none;
    // (a column-list launch already reads the listed columns only, and a noise box fills its list: there the
    //  second mask costs its fetch -- 42.4 -> 46.1 us at cfg 5 -- and saves nothing)
    cp.gh2_mask = cp.join == RowJoin::gh2_noise_only || (cp.join == RowJoin::gh2 && t.gh2_mask && !f.sparse_dirty && !sp);
    // the last launch of the call extracts the phase; in float32 (and unless a single-pass MRAF body has to join its
    // two parts) it also leaves G of the next body behind (MODE 3) -- of EVERY column, also on the column-list path,
    // so that whatever comes next (another call, the transform that ends optimize()) can start from it on every path
    cp.last_mode = (t.keep_g && f.elem == 4 && cp.join == RowJoin::none) ? 3 : 1;
    cp.need_gh2 = (m.split || m.split64) && !m.presum;
    cp.need_ffb = m.split64;
    cp.need_dpartial = m.presum || m.presum_col;
    cp.need_nog_dev = cp.nog;
    cp.accepts_prezeroed = prezero_ok(cp, f);
    cp.main.empty.prezeroed = cp.accepts_prezeroed && f.gh_prezeroed;
    cp.main.empty.list_walk = cp.main.empty.prezeroed && tile_list_ok(cp, f);
    return cp;
}

// ---- the row launch that closes a body ------------------------------------------------------------------------------
// load / store: 0 = every column, 1 = active columns, 2 = active columns dilated by the spot windows
struct RowClose {
    int mode = 0;                   // row_kernel MODE (3 = MODE 2 that also writes the phase; float32 only)
    bool finalize = false;          // one extra block folds the weight-norm partials into wscale
    bool wslot_fold = false;        // ... those the column launch left per half tile (ColLaunch::wslots)
    int load_sparse = 0, store_sparse = 0;
    int zero_par = -1;              // >= 0: RowArgs::zero_par -- the zero H of the empty columns is stored instead of their G
};
// cp / f: the body it closes; next: the facts of the body after it as that body will form them itself (nothing between this
// launch and that plan changes them), or null after the last body of a call.  Zeros are stored only where the next body
// accepts them and consults no column scan that could change the flags they were stored by; never by the last launch of a
// call, which leaves G of every column.
inline RowClose plan_row_close(const ColumnPlan& cp, const PassFacts& f, const PassFacts* next) {
    const bool sp = f.sparse_enabled;
    const int store_sparse = (f.stat_groups & 2) ? 2 : 1;
    RowClose rc;
    rc.mode = next ? 2 : cp.last_mode;
    rc.finalize = cp.finalize;
    rc.wslot_fold = cp.finalize && !cp.second_pass && cp.main.wslots;
    rc.load_sparse = sp ? 1 : 0;
    rc.store_sparse = (rc.mode == 3 || !sp) ? 0 : store_sparse;
    if (next && f.elem == 4 && !sp && cp.join == RowJoin::none) {
        const ColumnPlan cpn = plan_column_pass(*next);
        const Scans sn = scans_needed(*next);
        if (cpn.accepts_prezeroed && !sn.noise && !sn.signal && !sn.flags) rc.zero_par = (f.r0 - cpn.main.shift) & 1;
    }
    return rc;
}

// ---- the column scan ahead of dense launches ---------------------------------------------------------------------------
// Dense launches at 4096 rows in float32: how many columns hold anything picks the instance of the half-width tile kernel for
// one hologram (ColLaunch::few_active), and says in which columns that kernel requests weights and targets at all (col_flags;
// batches pay the scan for this alone, unless MRAF keeps them off that kernel) -- a fact about the target, scanned once per upload.
// rescan_outside: weights written behind the scan's back since are scanned again, once (PassFacts::w_outside_scan).
struct DenseScan { bool scan, rescan_outside; };
inline DenseScan dense_scan_needed(const PassFacts& f) {
    const bool scan = f.elem == 4 && f.tun.tile2 && f.Ph == 4096 && (f.B == 1 || (f.tun.empty_col_loads && !f.mraf_enabled));
    return DenseScan{scan, scan && f.tun.empty_col_loads != 0};
}

// spot feedback on a sparse target (Engine::iterate_spot_sparse): the fused launch over the spot columns, weight update off
// (the N-vector rule ran before it)
inline ColumnPlan plan_spot_sparse_pass(const PassFacts& f) {
    ColumnPlan cp;
    ColLaunch& l = cp.main;
    l.phase_mode = f.it.use_fixed ? 2 : (f.it.store_phase ? 1 : 0);
    l.listed = true;
    l.grid = list_blocks(f, f.n_active_max);
    l.stats = f.stat_groups & 1;
    fused_family(f, l);
    cp.wpartial_n = l.grid;
    cp.last_mode = (f.tun.keep_g && f.elem == 4) ? 3 : 1;          // (MODE 3 stores every column, see plan_column_pass())
    return cp;
}

}  // namespace hgs
