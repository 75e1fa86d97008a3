// Host program of tests/test_tile_list.py: wslots_ok() and tile_list_ok() of slmsuite_amd/csrc/column_plan.hpp without a GPU, next
// to prezero_ok().  One line of key=value facts per line of stdin ->
// "<wslots_ok> <tile_list_ok> <prezero_ok> <family of the main launch> <col_flags> <few_active> <grid>" per line.
// Facts not named keep the defaults of a cfg-2-like body: fp32, 4096 x 4096, 1152 SLM rows (five register slots), one hologram,
// 256 CUs, WGS-Leonardo with a weight update, a current scan that found 32 active columns, column lists off.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <sstream>
#include <string>

#include "column_plan.hpp"

using namespace hgs;

int main() {
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        PassFacts f;
        f.elem = 4; f.Ph = 4096; f.Pw = 4096; f.B = 1; f.n_cu = 256; f.Sh = 1152;
        f.it = Plan{1, 0, 0};
        f.method = HGS_WGS_LEONARDO;
        f.sparse_dirty = false;
        f.n_active_min = f.n_active_max = 32;
        f.tun.sparse = 0;
        std::istringstream in(line);
        std::string tok;
        static const std::map<std::string, int Tuning::*> switches = {
            {"HGS_OPT_EMPTY_COL_LOADS", &Tuning::empty_col_loads}, {"HGS_OPT_EMPTY_COL_INVERSE", &Tuning::empty_col_inverse},
            {"HGS_OPT_EMPTY_COL_FORWARD", &Tuning::empty_col_forward}, {"HGS_OPT_EMPTY_COL_PREZERO", &Tuning::empty_col_prezero},
            {"HGS_OPT_EMPTY_COL_LIST", &Tuning::empty_col_list}, {"HGS_OPT_SPARSE_COLUMNS", &Tuning::sparse}, {"HGS_TILE2", &Tuning::tile2},
            {"HGS_TILE2_BLOCKS", &Tuning::tile2_blocks}};
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "bad token %s\n", tok.c_str()); return 2; }
            const std::string k = tok.substr(0, eq);
            const int v = atoi(tok.c_str() + eq + 1);
            if (k == "elem") f.elem = v; else if (k == "Ph") f.Ph = v; else if (k == "Pw") f.Pw = v; else if (k == "B") f.B = v;
            else if (k == "Sh") f.Sh = v;
            else if (k == "do_update") f.it.do_update = v; else if (k == "use_fixed") f.it.use_fixed = v;
            else if (k == "store_phase") f.it.store_phase = v; else if (k == "method") f.method = v;
            else if (k == "mraf") f.mraf_enabled = v; else if (k == "stat_groups") f.stat_groups = v;
            else if (k == "w_outside_scan") f.w_outside_scan = v != 0;
            else if (k == "sparse_dirty") f.sparse_dirty = v != 0;
            else if (k == "n_active") f.n_active_min = f.n_active_max = v;
            else if (switches.count(k)) f.tun.*switches.at(k) = v;
            else { fprintf(stderr, "unknown fact %s\n", k.c_str()); return 2; }
        }
        f.r0 = (f.Ph - f.Sh) / 2;
        // block counts as hgs_create derives them for one-column workgroup passes (4096 rows and up)
        f.col_blocks = std::min(f.Pw / 4, std::max(1, f.n_cu * 3 / f.B));
        f.tile_blocks = std::max(1, std::min(f.Pw / 4, (f.Ph >= 8192 ? f.n_cu : f.n_cu * 2) / f.B));
        const ColumnPlan cp = plan_column_pass(f);
        printf("%d %d %d %s %d %d %d\n", wslots_ok(cp.main, f) ? 1 : 0, tile_list_ok(cp, f) ? 1 : 0, prezero_ok(cp, f) ? 1 : 0,
               cp.main.family == ColFamily::tile2 ? "tile2" : "other", cp.main.col_flags ? 1 : 0, cp.main.few_active ? 1 : 0, cp.main.grid);
    }
    return 0;
}
