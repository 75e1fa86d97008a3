// Host program of tests/test_engine_state.py: slmsuite_amd/csrc/engine_state.hpp without a GPU.
//   events  the event names, one per line
//   run     one sequence of event names per line of stdin (applied to a fresh state) -> one JSON object per line: the flags
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>

#include "engine_state.hpp"

using hgs::EngineState;

struct Event { const char* name; void (*apply)(EngineState&); };

// every transition of the header; the ones with arguments at each value the engine passes
static const Event events[] = {
    {"nearfield_upload_begins", [](EngineState& s) { s.nearfield_upload_begins(); }},
    {"nearfield_input_changed", [](EngineState& s) { s.nearfield_input_changed(); }},
    {"geometry_changed", [](EngineState& s) { s.geometry_changed(); }},
    {"target_written", [](EngineState& s) { s.target_written(); }},
    {"weights_write_begins", [](EngineState& s) { s.weights_write_begins(); }},
    {"weights_written", [](EngineState& s) { s.weights_written(); }},
    {"scale_folded", [](EngineState& s) { s.scale_folded(); }},
    {"phase_ff_stored", [](EngineState& s) { s.phase_ff_stored(); }},
    {"farfield_materialised", [](EngineState& s) { s.farfield_materialised(false); }},
    {"farfield_materialised_pff", [](EngineState& s) { s.farfield_materialised(true); }},
    {"farfield_consumed", [](EngineState& s) { s.farfield_consumed(); }},
    {"general_rule_updated_weights", [](EngineState& s) { s.general_rule_updated_weights(); }},
    {"cg_gradient_stored", [](EngineState& s) { s.cg_gradient_stored(); }},
    {"fused_call_begins", [](EngineState& s) { s.fused_call_begins(); }},
    {"spot_sparse_call_begins", [](EngineState& s) { s.spot_sparse_call_begins(); }},
    {"rescan_if_written_outside", [](EngineState& s) { s.rescan_if_written_outside(); }},
    {"column_pass_begins", [](EngineState& s) { s.column_pass_begins(); }},
    {"fused_update_done", [](EngineState& s) { s.fused_update_done(); }},
    {"row_launch_begins", [](EngineState& s) { s.row_launch_begins(); }},
    {"row_stored_g_mode1_s0", [](EngineState& s) { s.row_stored_g(1, 0); }},
    {"row_stored_g_mode0_s0", [](EngineState& s) { s.row_stored_g(0, 0); }},
    {"row_stored_g_mode0_s1", [](EngineState& s) { s.row_stored_g(0, 1); }},
    {"row_stored_g_mode0_s2", [](EngineState& s) { s.row_stored_g(0, 2); }},
    {"row_stored_g_mode2_s1", [](EngineState& s) { s.row_stored_g(2, 1); }},
    {"row_stored_g_mode2_s2", [](EngineState& s) { s.row_stored_g(2, 2); }},
    {"row_stored_g_mode3_s0", [](EngineState& s) { s.row_stored_g(3, 0); }},
    {"prev_phase_kept", [](EngineState& s) { s.prev_phase_kept(); }},
    {"prev_phase_dropped", [](EngineState& s) { s.prev_phase_dropped(); }},
    {"scan_started", [](EngineState& s) { s.scan_started(); }},
    {"scan_finished", [](EngineState& s) { s.scan_finished(); }},
    {"dilation_rebuild_begins", [](EngineState& s) { s.dilation_rebuild_begins(); }},
    {"dilation_rebuilt", [](EngineState& s) { s.dilation_rebuilt(-2, 1); }},
    {"signal_list_rebuilt", [](EngineState& s) { s.signal_list_rebuilt(); }},
    {"noise_list_rebuild_begins", [](EngineState& s) { s.noise_list_rebuild_begins(); }},
    {"noise_list_rebuilt", [](EngineState& s) { s.noise_list_rebuilt(); }},
    {"ffb_was_zeroed", [](EngineState& s) { s.ffb_was_zeroed(); }},
    {"reset_state", [](EngineState& s) { s.reset_state(); }},
    {"column_policy_changed", [](EngineState& s) { s.column_policy_changed(); }},
    {"scan_policy_changed", [](EngineState& s) { s.scan_policy_changed(); }},
};

static void print_state(const EngineState& s) {
    printf("{\"gh_state\": %d, \"gh_holds\": [%d, %d, %d], \"gh_holds_keep_g_off\": [%d, %d, %d], \"farfield_valid\": %d, \"have_pff\": %d, "
           "\"have_prev\": %d, \"w_pending\": %d, \"w_unit\": %d, \"w_outside_scan\": %d, \"sparse_dirty\": %d, \"dil_valid\": %d, "
           "\"dil_lo\": %d, \"dil_hi\": %d, \"dilation_is_m2_1\": %d, \"noise_valid\": %d, \"signal_valid\": %d, \"ffb_zeroed\": %d, "
           "\"cg_have_grad\": %d}\n",
           s.gh_state(), s.gh_holds(0, true), s.gh_holds(1, true), s.gh_holds(2, true), s.gh_holds(0, false), s.gh_holds(1, false),
           s.gh_holds(2, false), s.farfield_valid(), s.have_pff(), s.have_prev(), s.w_pending(), s.w_unit(), s.w_outside_scan(),
           s.sparse_dirty(), s.dil_valid(), s.dil_lo(), s.dil_hi(), s.dilation_is(-2, 1), s.noise_valid(), s.signal_valid(),
           s.ffb_zeroed(), s.cg_have_grad());
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "events")) {
        for (const Event& e : events) puts(e.name);
        return 0;
    }
    if (argc != 2 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: %s events|run\n", argv[0]); return 2; }
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        EngineState s;
        std::istringstream in(line);
        std::string tok;
        while (in >> tok) {
            const Event* hit = nullptr;
            for (const Event& e : events) if (tok == e.name) hit = &e;
            if (!hit) { fprintf(stderr, "unknown event %s\n", tok.c_str()); return 2; }
            hit->apply(s);
        }
        print_state(s);
    }
    return 0;
}
