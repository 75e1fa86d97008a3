// Host program of tests/test_column_plan.py, test_column_plan_prezero.py and test_tile_list.py: slmsuite_amd/csrc/column_plan.hpp
// without a GPU.
//   plan   one line of key=value facts per line of stdin -> one JSON object per line: the plan of the body, the row launch that
//          closes it as the last body of a call ("close_last") and ahead of a next body ("close_next"), and the per-upload scan
//          decision.  The next body has the same facts (gh_prezeroed aside) unless "next:" follows, with the facts that differ.
//          "preset=cfg2" starts from a cfg-2-like body instead of from nothing (preset_cfg2); r0 not given: a centred SLM block.
//   sweep  a grid of facts, the invariants of the plan checked on every point -> "violation ..." lines, then "checked N"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>

#include "column_plan.hpp"

using namespace hgs;

// col_blocks / tile_blocks as hgs_create derives them (Engine::init)
static void derive_blocks(PassFacts& f) {
    const int tiles = f.Pw / 4;
    int cap = f.n_cu * 3;
    cap = cap / f.B > 0 ? cap / f.B : 1;
    const int per = (tiles + cap - 1) / cap;
    f.col_blocks = (tiles + per - 1) / per;
    const int passes = 4 / col_cpar(f.Ph), q = 8 * passes;
    if (passes > 1 && f.tun.col_xmap) {
        double best = 0;
        int best_g = 0;
        for (int G = q; G <= cap && G / passes <= tiles; G += q) {
            const int gp = G / passes, sweeps = (tiles + gp - 1) / gp;
            const double eff = (double)tiles / ((double)sweeps * gp);
            if (eff >= best - 1e-9) { best = eff; best_g = G; }
        }
        if (best_g > 0 && best >= 0.9) f.col_blocks = best_g;
    }
    f.tile_blocks = std::max(1, std::min(tiles, (f.Ph >= 8192 ? f.n_cu : f.n_cu * 2) / f.B));
}

// a cfg-2-like body: fp32, 4096 x 4096, 1152 SLM rows (five register slots), one hologram, 256 CUs, WGS-Leonardo with a weight
// update, a current scan that found 32 active columns, column lists off
static void preset_cfg2(PassFacts& f) {
    f = PassFacts{};
    f.elem = 4; f.Ph = 4096; f.Pw = 4096; f.B = 1; f.n_cu = 256; f.Sh = 1152;
    f.it = Plan{1, 0, 0};
    f.method = HGS_WGS_LEONARDO;
    f.sparse_dirty = false;
    f.n_active_min = f.n_active_max = 32;
    f.tun.sparse = 0;
}

static const char* family_name(ColFamily c) {
    static const char* names[] = {"fused", "fused_rule1", "fused_rule2", "fused_stats", "tile", "tile_rule", "tile_rule_listed", "tile_stats",
                                  "tile_extras", "tile_extras_stats", "tile_split", "tile_split_stats", "tile_presum", "tile2"};
    return names[(int)c];
}
static bool is_tile(ColFamily c) { return c != ColFamily::fused && c != ColFamily::fused_rule1 && c != ColFamily::fused_rule2 && c != ColFamily::fused_stats; }
static bool is_split(const ColLaunch& l) { return l.family == ColFamily::tile_split || l.family == ColFamily::tile_split_stats; }

static int* tuning_field(Tuning& t, const std::string& k) {
    static const std::map<std::string, int Tuning::*> m = {
        {"HGS_TILE2_BLOCKS", &Tuning::tile2_blocks}, {"HGS_COL_XMAP", &Tuning::col_xmap}, {"HGS_TILE_RULE", &Tuning::tile_rule},
        {"HGS_MRAF_SPLIT", &Tuning::mraf_split}, {"HGS_MRAF_SPLIT64", &Tuning::mraf_split64}, {"HGS_GH2_MASK", &Tuning::gh2_mask},
        {"HGS_TILE_LIST", &Tuning::tile_list}, {"HGS_TILE_SHIFT16", &Tuning::tile_shift16}, {"HGS_TILE_NR4", &Tuning::tile_nr4},
        {"HGS_TILE2", &Tuning::tile2}, {"HGS_TILE2_MIN_BATCH", &Tuning::tile2_min_batch}, {"HGS_TILE2_PHASE2", &Tuning::tile2_phase2},
        {"HGS_KEEP_G", &Tuning::keep_g}, {"HGS_MRAF_PRESUM", &Tuning::mraf_presum}, {"HGS_PRESUM_BLOCKS", &Tuning::presum_blocks},
        {"HGS_OPT_EMPTY_COL_LOADS", &Tuning::empty_col_loads}, {"HGS_OPT_EMPTY_COL_INVERSE", &Tuning::empty_col_inverse},
        {"HGS_OPT_EMPTY_COL_FORWARD", &Tuning::empty_col_forward}, {"HGS_OPT_EMPTY_COL_PREZERO", &Tuning::empty_col_prezero},
        {"HGS_OPT_EMPTY_COL_LIST", &Tuning::empty_col_list},
        {"HGS_OPT_SPARSE_COLUMNS", &Tuning::sparse}, {"HGS_OPT_TILE_KERNEL", &Tuning::tile}};
    auto it = m.find(k);
    return it == m.end() ? nullptr : &(t.*(it->second));
}

// the facts one body forms; what was not given is derived once all tokens are read (finish)
struct Parsed {
    PassFacts f;
    bool blocks_given = false, r0_given = false;
    bool token(const std::string& tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) { fprintf(stderr, "bad token %s\n", tok.c_str()); return false; }
        const std::string k = tok.substr(0, eq);
        if (k == "preset") {
            if (tok.substr(eq + 1) != "cfg2") { fprintf(stderr, "unknown preset %s\n", tok.c_str()); return false; }
            preset_cfg2(f);
            return true;
        }
        const int v = atoi(tok.c_str() + eq + 1);
        if (k == "elem") f.elem = v; else if (k == "Ph") f.Ph = v; else if (k == "Pw") f.Pw = v; else if (k == "B") f.B = v;
        else if (k == "n_cu") f.n_cu = v; else if (k == "col_blocks") { f.col_blocks = v; blocks_given = true; }
        else if (k == "tile_blocks") { f.tile_blocks = v; blocks_given = true; }
        else if (k == "r0") { f.r0 = v; r0_given = true; } else if (k == "Sh") f.Sh = v; else if (k == "do_update") f.it.do_update = v;
        else if (k == "use_fixed") f.it.use_fixed = v; else if (k == "store_phase") f.it.store_phase = v;
        else if (k == "method") f.method = v; else if (k == "mraf") f.mraf_enabled = v; else if (k == "zero_mode") f.zero_mode = v;
        else if (k == "stat_groups") f.stat_groups = v; else if (k == "w_unit") f.w_unit = v != 0;
        else if (k == "sparse_enabled") f.sparse_enabled = v != 0; else if (k == "sparse_tiles") f.sparse_tiles = v != 0;
        else if (k == "sparse_dirty") f.sparse_dirty = v != 0; else if (k == "n_active_min") f.n_active_min = v;
        else if (k == "n_active_max") f.n_active_max = v; else if (k == "n_active") f.n_active_min = f.n_active_max = v;
        else if (k == "n_noise_max") f.n_noise_max = v;
        else if (k == "n_signal_max") f.n_signal_max = v; else if (k == "ffb_unavailable") f.ffb_unavailable = v != 0;
        else if (k == "gh_prezeroed") f.gh_prezeroed = v != 0; else if (k == "w_outside_scan") f.w_outside_scan = v != 0;
        else if (int* p = tuning_field(f.tun, k)) *p = v;
        else { fprintf(stderr, "unknown fact %s\n", k.c_str()); return false; }
        return true;
    }
    void finish() {
        if (!r0_given) f.r0 = (f.Ph - f.Sh) / 2;
        if (!blocks_given) derive_blocks(f);
    }
};

static void print_launch(const char* name, const ColLaunch& l) {
    printf("\"%s\": {\"family\": \"%s\", \"phase_mode\": %d, \"rule\": %d, \"rule_ok\": %d, \"nr\": %d, \"shift\": %d, \"grid\": %d, "
           "\"listed\": %d, \"list_xmap\": %d, \"half_xmap\": %d, \"few_active\": %d, \"gh2_sparse\": %d, \"col_flags\": %d, "
           "\"empty\": {\"skip_inverse\": %d, \"skip_forward\": %d, \"prezeroed\": %d, \"list_walk\": %d}, \"wslots\": %d, \"nog_pass\": %d, "
           "\"use_nog\": %d, \"weights_only\": %d, \"split64\": %d, \"do_update\": %d, \"stats\": %d, \"n_dpartial\": %d}, ",
           name, family_name(l.family), l.phase_mode, l.rule, l.rule_ok, l.nr, l.shift, l.grid, l.listed, l.list_xmap, l.half_xmap,
           l.few_active, l.gh2_sparse, l.col_flags, l.empty.skip_inverse, l.empty.skip_forward, l.empty.prezeroed, l.empty.list_walk, l.wslots,
           l.nog_pass, l.use_nog, l.weights_only, l.split64, l.do_update, l.stats, l.n_dpartial);
}
static void print_close(const char* name, const RowClose& rc) {
    printf("\"%s\": {\"mode\": %d, \"finalize\": %d, \"wslot_fold\": %d, \"load_sparse\": %d, \"store_sparse\": %d, \"zero_par\": %d}, ", name,
           rc.mode, rc.finalize, rc.wslot_fold, rc.load_sparse, rc.store_sparse, rc.zero_par);
}

static int plan_lines() {
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        Parsed body, next;
        body.f.sparse_dirty = false;
        bool in_next = false;
        std::istringstream in(line);
        std::string tok;
        while (in >> tok) {
            if (tok == "next:" && !in_next) { in_next = true; next = body; continue; }
            if (!(in_next ? next : body).token(tok)) return 2;
        }
        if (!in_next) next = body;
        next.f.gh_prezeroed = false;          // (whether the next body finds zeros is what close_next says)
        body.finish();
        next.finish();
        const PassFacts& f = body.f;
        const Scans s = scans_needed(f);
        const DenseScan ds = dense_scan_needed(f);
        const ColumnPlan cp = plan_column_pass(f);
        printf("{\"col_blocks\": %d, \"tile_blocks\": %d, \"scan_noise\": %d, \"scan_signal\": %d, \"scan_flags\": %d, ", f.col_blocks,
               f.tile_blocks, s.noise, s.signal, s.flags);
        printf("\"dense_scan\": {\"scan\": %d, \"rescan_outside\": %d}, ", ds.scan, ds.rescan_outside);
        printf("\"dilated_forward\": %d, \"nog\": %d, \"presum\": %d, \"presum_col\": %d, \"prepass_grid\": %d, \"prepass_list_xmap\": %d, ",
               cp.dilated_forward, cp.nog, cp.presum, cp.presum_col, cp.prepass_grid, cp.prepass_list_xmap);
        print_launch("nog_pass", cp.nog_pass);
        print_launch("main", cp.main);
        print_launch("second", cp.second);
        print_close("close_last", plan_row_close(cp, f, nullptr));
        print_close("close_next", plan_row_close(cp, f, &next.f));
        printf("\"accepts_prezeroed\": %d, ", cp.accepts_prezeroed);
        printf("\"scale_after_main\": %d, \"second_pass\": %d, \"noise_inverse_grid\": %d, \"finalize\": %d, \"join\": \"%s\", \"gh2_mask\": %d, "
               "\"last_mode\": %d, \"wpartial_n\": %d, \"need_gh2\": %d, \"need_ffb\": %d, \"need_dpartial\": %d, \"need_nog_dev\": %d}\n",
               cp.scale_after_main, cp.second_pass, cp.noise_inverse_grid, cp.finalize,
               cp.join == RowJoin::none ? "none" : cp.join == RowJoin::gh2 ? "gh2" : "gh2_noise_only", cp.gh2_mask, cp.last_mode, cp.wpartial_n,
               cp.need_gh2, cp.need_ffb, cp.need_dpartial, cp.need_nog_dev);
    }
    return 0;
}

static long n_checked = 0, n_bad = 0;
static void violation(const char* what, const PassFacts& f, int sw) {
    if (++n_bad > 40) return;
    printf("violation: %s | elem=%d Ph=%d Pw=%d B=%d Sh=%d r0=%d do_update=%d use_fixed=%d store_phase=%d method=%d mraf=%d zero_mode=%d "
           "stat_groups=%d w_unit=%d sparse_enabled=%d sparse_tiles=%d sparse_dirty=%d n_active_max=%d n_noise_max=%d n_signal_max=%d "
           "ffb_unavailable=%d gh_prezeroed=%d w_outside_scan=%d switch_off=%d\n", what, f.elem, f.Ph, f.Pw, f.B, f.Sh, f.r0, f.it.do_update,
           f.it.use_fixed, f.it.store_phase, f.method, f.mraf_enabled, f.zero_mode, f.stat_groups, f.w_unit, f.sparse_enabled, f.sparse_tiles,
           f.sparse_dirty, f.n_active_max, f.n_noise_max, f.n_signal_max, f.ffb_unavailable, f.gh_prezeroed, f.w_outside_scan, sw);
}

// the empty-column ladder of one launch: each level only on the one below it, none outside the half-width kernel
static void check_ladder(const ColLaunch& l, const PassFacts& f, int sw) {
    const EmptyCols& e = l.empty;
    if ((e.skip_inverse && !l.col_flags) || (e.skip_forward && !e.skip_inverse) || (e.prezeroed && !e.skip_forward) || (e.list_walk && !e.prezeroed))
        violation("empty-column level without the one below it", f, sw);
    if (l.family != ColFamily::tile2 && (e.skip_inverse || e.skip_forward || e.prezeroed || e.list_walk || l.wslots))
        violation("empty-column level or weight-norm slots outside tile2", f, sw);
}

// the row launch that closes the body, ahead of `next` (null: the last body of a call)
static void check_close(const ColumnPlan& cp, const PassFacts& f, const PassFacts* next, int sw) {
    const RowClose rc = plan_row_close(cp, f, next);
    if (rc.mode != (next ? 2 : cp.last_mode) || rc.finalize != cp.finalize) violation("closing row launch: mode or fold", f, sw);
    if (rc.wslot_fold && !(cp.main.wslots && rc.finalize)) violation("slot fold without slots", f, sw);
    if (rc.mode == 3 && rc.store_sparse) violation("MODE 3 behind a store mask", f, sw);
    if (rc.zero_par >= 0 && !(next && rc.mode == 2 && !rc.load_sparse && !rc.store_sparse && cp.join == RowJoin::none &&
                              plan_column_pass(*next).accepts_prezeroed))
        violation("zeros stored for a body that does not accept them", f, sw);
}

// each invariant is a comment or a guard of the engine (see tests/test_column_plan.py)
static void check(const PassFacts& f, int sw) {
    const ColumnPlan cp = plan_column_pass(f);
    ++n_checked;
    const ColLaunch* ls[3] = {cp.nog ? &cp.nog_pass : nullptr, &cp.main, cp.second_pass ? &cp.second : nullptr};
    const int cap = std::max(std::max(f.col_blocks, f.tile_blocks), 3 * f.n_cu);
    for (const ColLaunch* l : ls) {
        if (!l) continue;
        if (f.elem == 8 && is_tile(l->family)) violation("tile family for 8-byte elements", f, sw);
        if (l->family == ColFamily::tile2 && (l->stats || f.mraf_enabled || l->nog_pass || l->use_nog || l->weights_only || f.sparse_enabled))
            violation("tile2 outside a plain dense pass", f, sw);
        if (l->grid < 1 || l->grid > cap) violation("grid beyond what the partial buffers are sized for", f, sw);
        if (l != &cp.main && (is_split(*l) || l->split64 || l->rule == 5)) violation("split / pre-sum form outside the main launch", f, sw);
        check_ladder(*l, f, sw);
        if (l != &cp.main && (l->empty.prezeroed || l->wslots)) violation("pre-zeroed H or weight-norm slots outside the main launch", f, sw);
    }
    if (cp.scale_after_main && cp.main.wslots) violation("weight-norm slots ahead of a per-workgroup reduction", f, sw);
    if (cp.main.empty.prezeroed != (cp.accepts_prezeroed && f.gh_prezeroed)) violation("pre-zeroed H not where it was left and is accepted", f, sw);
    if (cp.prepass_grid > cap || cp.noise_inverse_grid > cap || cp.wpartial_n > cap || cp.wpartial_n < 1) violation("grid beyond the partial buffers", f, sw);
    const bool presum_form = cp.presum || cp.presum_col || cp.main.rule == 5;
    if (presum_form && !(f.w_unit && f.it.do_update && f.mraf_enabled && (f.method == HGS_WGS_LEONARDO || f.method == HGS_WGS_KIM) && !f.stat_groups))
        violation("pre-sum form without its preconditions", f, sw);
    if (cp.presum != (cp.main.rule == 5) || (presum_form && (cp.prepass_grid < 1 || !cp.need_dpartial || cp.main.n_dpartial != cp.prepass_grid)))
        violation("pre-pass and main pass disagree", f, sw);
    const bool split_ran = is_split(cp.main) || cp.main.split64;
    if ((cp.join != RowJoin::none) != split_ran) violation("joining row launch without a split form (or the reverse)", f, sw);
    if (split_ran && !cp.need_gh2) violation("split form without gh2", f, sw);
    if (cp.main.split64 != cp.need_ffb || (cp.noise_inverse_grid > 0 && !cp.main.split64)) violation("column split and its buffer disagree", f, sw);
    if (cp.last_mode != 1 && !(cp.last_mode == 3 && f.elem == 4 && cp.join == RowJoin::none)) violation("last_mode 3 for 8-byte elements or with a join", f, sw);
    const int forms = (int)cp.second_pass + (int)is_split(cp.main) + (int)cp.main.split64 + (int)cp.presum + (int)cp.presum_col;
    if (forms > 1) violation("more than one MRAF update form", f, sw);
    if (f.mraf_enabled && f.it.do_update && forms != 1) violation("MRAF update without a form", f, sw);
    if (!(f.mraf_enabled && f.it.do_update) && forms != 0) violation("MRAF update form without an MRAF update", f, sw);
    if (cp.finalize && (!f.it.do_update || cp.scale_after_main)) violation("weight norm folded twice or without an update", f, sw);
    if (f.it.do_update && !cp.finalize && !cp.scale_after_main) violation("weight norm never folded", f, sw);
    if (cp.nog != (f.method == HGS_WGS_NOGRETTE && f.it.do_update) || cp.nog != cp.need_nog_dev) violation("Nogrette pass", f, sw);
    const Scans s = scans_needed(f);
    if ((cp.main.split64 && !s.noise) || (cp.presum_col && !s.signal) || (cp.presum && !s.flags)) violation("form without its column scan", f, sw);
    // the closing row launch: as the last of a call, ahead of the same body again, ahead of a body that stores the farfield phase
    PassFacts next = f;
    next.gh_prezeroed = false;
    check_close(cp, f, nullptr, sw);
    check_close(cp, f, &next, sw);
    next.it = Plan{f.it.do_update, 0, 1};
    check_close(cp, f, &next, sw);
}

static int sweep() {
    int Tuning::*switches[] = {nullptr, &Tuning::col_xmap, &Tuning::tile_rule, &Tuning::mraf_split, &Tuning::mraf_split64, &Tuning::gh2_mask,
                               &Tuning::tile_list, &Tuning::tile_shift16, &Tuning::tile_nr4, &Tuning::tile2, &Tuning::tile2_phase2, &Tuning::keep_g,
                               &Tuning::mraf_presum, &Tuning::sparse, &Tuning::tile, &Tuning::tile2_min_batch, &Tuning::tile2_blocks, &Tuning::presum_blocks,
                               &Tuning::empty_col_loads, &Tuning::empty_col_inverse, &Tuning::empty_col_forward, &Tuning::empty_col_prezero,
                               &Tuning::empty_col_list};
    const int n_sw = sizeof switches / sizeof switches[0];
    for (int sw = 0; sw < n_sw; ++sw)
    for (int elem : {4, 8})
    for (int Ph : {256, 512, 1024, 2048, 4096, 8192})
    for (int Pw : {Ph, 4096})
    for (int sixteenths : {1, 4, 6, 7, 16})           // SLM rows as a share of the padded rows: within / beyond six register slots
    for (int B : {1, 2, 3, 8})
    for (int method = HGS_GS; method <= HGS_WGS_TANH; ++method)
    for (int mraf : {0, 1})
    for (int upd : {0, 1})
    for (int phase_mode : {0, 1, 2})
    for (int groups : {0, 1, 2, 3})
    for (int sparse : {0, 1, 2, 3, 4})                // dense (scanned), dense (never scanned), column list, list of whole tiles,
                                                      // dense with few active columns (the scan's flags go with the launch)
    for (int w_unit : {0, 1}) {
        if (upd && method == HGS_GS) continue;
        if (Pw != Ph && Ph == 4096) continue;
        // (few active columns and the empty-column switches move a plan only where the half-width kernel runs)
        if ((sparse == 4 || sw >= n_sw - 5) && !(elem == 4 && Ph >= 2048 && Ph <= 4096)) continue;
        PassFacts f;
        if (sw) {
            f.tun.*switches[sw] = 0;
            if (switches[sw] == &Tuning::tile2_min_batch) f.tun.tile2_min_batch = 2;
            if (switches[sw] == &Tuning::tile2_blocks) f.tun.tile2_blocks = 1 << 20;
            if (switches[sw] == &Tuning::presum_blocks) f.tun.presum_blocks = 64;
        }
        f.elem = elem; f.Ph = Ph; f.Pw = Pw; f.B = B; f.n_cu = 256;
        f.Sh = std::max(1, Ph * sixteenths / 16 - (sixteenths == 16 ? 0 : 8));
        f.r0 = (Ph - f.Sh) / 2;
        derive_blocks(f);
        f.it = Plan{upd, phase_mode == 2, phase_mode == 1};
        f.method = method; f.mraf_enabled = mraf; f.zero_mode = 0; f.stat_groups = groups; f.w_unit = w_unit != 0;
        f.sparse_enabled = (sparse == 2 || sparse == 3) && f.tun.sparse;
        f.sparse_dirty = sparse == 1;
        f.sparse_tiles = sparse == 3 && tile_geometry_ok(f) && f.tun.tile_list;
        f.n_active_min = f.n_active_max = sparse == 1 ? 0 : sparse >= 2 ? Pw / 8 : Pw;
        for (int noise : {0, 1, 2}) {                 // noise / signal columns: none, a third of the active ones, all of them
            if (noise && !mraf) continue;
            f.n_noise_max = sparse == 1 ? 0 : f.n_active_max * noise / (noise == 1 ? 3 : 2);
            f.n_signal_max = sparse == 1 ? 0 : f.n_active_max - f.n_noise_max / 2;
            if (noise == 2 && sparse == 0) f.n_signal_max = 0;
            f.ffb_unavailable = false;
            f.gh_prezeroed = f.w_outside_scan = false;
            check(f, sw);
            const ColumnPlan cp = plan_column_pass(f);
            if (cp.need_ffb) { f.ffb_unavailable = true; check(f, sw); }
            // the two buffer-state facts of the flag-reading launches: zeros left by the row launch before (only ever ahead of a
            // body that accepts them), a weight written behind the scan
            if (cp.accepts_prezeroed) { f.gh_prezeroed = true; check(f, sw); f.gh_prezeroed = false; }
            if (cp.main.col_flags) { f.w_outside_scan = true; check(f, sw); }
        }
    }
    printf("checked %ld violations %ld\n", n_checked, n_bad);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "plan")) return plan_lines();
    if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
    fprintf(stderr, "usage: %s plan|sweep\n", argv[0]);
    return 2;
}
