"""
The engine's validity flags, without a GPU: ``slmsuite_amd/csrc/engine_state.hpp`` is plain C++ (no HIP), so the table
"which event invalidates what" is checked here on the transitions themselves.  tests/engine_state_host.cpp applies a
sequence of named events to a fresh state and prints the flags; the GPU tests keep asserting what was LAUNCHED because of
them (tests/test_gpu_round6.py::test_weight_writers_send_one_mraf_update_through_the_old_form_a_target_none).
"""
import itertools
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "slmsuite_amd", "csrc", "engine_state.hpp")

NEARFIELD_INPUT = ("nearfield_upload_begins", "nearfield_input_changed")
ROW_STORES = {s: f"row_stored_g_mode2_s{s}" for s in (1, 2)}
ROW_STORES[0] = "row_stored_g_mode3_s0"


def _compiler():
    for cxx in ("c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/bin/amdclang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ / clang++) on this machine")
    exe = str(tmp_path_factory.mktemp("engine_state") / "engine_state_host")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "slmsuite_amd", "csrc"),
                        os.path.join(ROOT, "tests", "engine_state_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, sequences):
    """Flags after each sequence (a list of event names) from the initial state; one process for all of them."""
    text = "".join(" ".join(seq) + "\n" for seq in sequences)
    r = subprocess.run([exe, "run"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(sequences)
    return out


def _after(exe, *events):
    return _run(exe, [events])[0]


@pytest.fixture(scope="module")
def events(host):
    r = subprocess.run([host, "events"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.split()


def test_header_includes_no_hip():
    src = open(HEADER).read()
    assert "hip/" not in src and "__global__" not in src and "hipLaunch" not in src and "#include" not in src


def test_the_host_program_knows_every_transition(events):
    """The sweep below is over the host program's table: it has to list every non-const member of the header."""
    declared = set(re.findall(r"^\s+void (\w+)\(", open(HEADER).read(), flags=re.M))
    assert declared, "no transitions found in the header"
    for name in declared:
        assert any(e == name or e.startswith(name + "_") for e in events), f"{name} is missing from tests/engine_state_host.cpp"
    for e in events:
        assert any(e == name or e.startswith(name + "_") for name in declared), f"{e} names no transition of the header"


def test_initial_state(host):
    s = _after(host)
    assert s["gh_state"] == -1 and s["gh_holds"] == [0, 0, 0] and s["sparse_dirty"] == 1
    assert not any(s[k] for k in ("farfield_valid", "have_pff", "have_prev", "w_pending", "w_unit", "w_outside_scan", "dil_valid",
                                  "noise_valid", "signal_valid", "ffb_zeroed", "cg_have_grad"))


def test_fused_update_sets_w_unit_and_w_pending(host):
    s = _after(host, "fused_update_done")
    assert s["w_unit"] == 1 and s["w_pending"] == 1


@pytest.mark.parametrize("writer", [("weights_write_begins", "weights_written"),     # host / device upload of the raster
                                    ("weights_written",),                            # sparse upload; hgs_reset_weights
                                    ("reset_state", "weights_written"),              # hgs_reset
                                    ("scale_folded",),
                                    ("spot_sparse_call_begins",)])
def test_every_other_writer_of_the_weights_clears_w_unit(host, writer):
    s = _after(host, "scan_finished", "fused_update_done", *writer)
    assert s["w_unit"] == 0
    if "weights_written" in writer:
        assert s["w_pending"] == 0 and s["sparse_dirty"] == 1
    if writer == ("scale_folded",):
        assert s["w_pending"] == 0 and s["w_outside_scan"] == 1
    if writer == ("spot_sparse_call_begins",):
        assert s["w_outside_scan"] == 1 and s["farfield_valid"] == 0 and s["w_pending"] == 1


def test_a_target_upload_keeps_w_unit_and_dirties_the_scan(host):
    before = _after(host, "scan_finished", "fused_update_done")
    assert before["sparse_dirty"] == 0
    s = _after(host, "scan_finished", "fused_update_done", "target_written")
    assert s["w_unit"] == 1 and s["w_pending"] == 1 and s["sparse_dirty"] == 1


def test_only_the_fused_update_sets_w_unit(host, events):
    """Every sequence of up to three of the other events, from the initial state."""
    others = [e for e in events if e != "fused_update_done"]
    seqs = [seq for n in (1, 2, 3) for seq in itertools.product(others, repeat=n)]
    assert len(seqs) > 50_000
    bad = [seq for seq, s in zip(seqs, _run(host, seqs)) if s["w_unit"]]
    assert not bad, bad[:10]


def test_what_a_row_store_leaves_behind(host):
    """gh_holds(need) = HGS_KEEP_G and (state == need, or state 0, or state 2 serving need 1 while the dilation is valid)."""
    for s_store, ev in ROW_STORES.items():
        for dil in (False, True):
            pre = ("scan_finished", "dilation_rebuilt") if dil else ("scan_finished",)
            s = _after(host, *pre, "row_launch_begins", ev)
            assert s["gh_state"] == s_store
            want = [int(need == s_store or s_store == 0 or (s_store == 2 and need == 1 and dil)) for need in (0, 1, 2)]
            assert s["gh_holds"] == want, (s_store, dil, s)
            assert s["gh_holds_keep_g_off"] == [0, 0, 0]
    # MODE 1 extracts the phase: no G
    assert _after(host, "row_launch_begins", "row_stored_g_mode1_s0")["gh_state"] == -1
    # a row launch that fails stores nothing
    assert _after(host, ROW_STORES[0], "row_launch_begins")["gh_state"] == -1


def test_what_drops_g(host):
    for s_store, ev in ROW_STORES.items():
        for drop in NEARFIELD_INPUT + ("column_pass_begins", "reset_state", "column_policy_changed", "row_launch_begins"):
            assert _after(host, ev, drop)["gh_state"] == -1, (ev, drop)
        # a scan drops what was stored on the old lists, a dilation rebuild only what was stored on the dilated list
        assert _after(host, ev, "scan_started")["gh_state"] == (0 if s_store == 0 else -1)
        assert _after(host, ev, "dilation_rebuild_begins")["gh_state"] == (-1 if s_store == 2 else s_store)
        for keep in ("target_written", "weights_written", "scale_folded", "geometry_changed", "farfield_consumed", "fused_update_done",
                     "scan_finished", "dilation_rebuilt", "phase_ff_stored", "fused_call_begins", "spot_sparse_call_begins"):
            assert _after(host, ev, keep)["gh_state"] == s_store, (ev, keep)
    assert _after(host, ROW_STORES[0], "nearfield_input_changed")["farfield_valid"] == 0


def test_a_finished_scan_invalidates_the_derived_lists(host):
    pre = ("scan_finished", "dilation_rebuilt", "signal_list_rebuilt", "noise_list_rebuilt", "ffb_was_zeroed", "scale_folded", "target_written")
    s = _after(host, *pre)
    assert s["dil_valid"] and s["signal_valid"] and s["noise_valid"] and s["w_outside_scan"] and s["sparse_dirty"] and s["dilation_is_m2_1"]
    s = _after(host, *pre, "scan_started", "scan_finished")
    assert not (s["dil_valid"] or s["signal_valid"] or s["noise_valid"] or s["w_outside_scan"] or s["sparse_dirty"] or s["dilation_is_m2_1"])
    assert s["ffb_zeroed"] == 1          # ... until the noise list is actually rebuilt
    assert _after(host, *pre, "scan_started", "scan_finished", "noise_list_rebuild_begins")["ffb_zeroed"] == 0


def test_farfield_phase_and_previous_phase(host):
    assert _after(host, "farfield_materialised")["farfield_valid"] == 1 and _after(host, "farfield_materialised")["have_pff"] == 0
    assert _after(host, "farfield_materialised_pff")["have_pff"] == 1
    for ev in ("farfield_consumed", "fused_call_begins", "spot_sparse_call_begins", "geometry_changed", "nearfield_input_changed", "reset_state"):
        assert _after(host, "farfield_materialised_pff", ev)["farfield_valid"] == 0, ev
    assert _after(host, "farfield_materialised_pff", "farfield_consumed")["have_pff"] == 1
    assert _after(host, "phase_ff_stored", "reset_state")["have_pff"] == 0
    assert _after(host, "prev_phase_kept")["have_prev"] == 1
    for ev in ("prev_phase_dropped", "reset_state"):
        assert _after(host, "prev_phase_kept", ev)["have_prev"] == 0
    assert _after(host, "cg_gradient_stored")["cg_have_grad"] == 1 and _after(host, "cg_gradient_stored", "reset_state")["cg_have_grad"] == 0
    # weights written behind the scan's back are scanned again by the next dense call that asks; a clean state is left alone
    assert _after(host, "scan_finished", "rescan_if_written_outside")["sparse_dirty"] == 0
    assert _after(host, "scan_finished", "scale_folded", "rescan_if_written_outside")["sparse_dirty"] == 1
    assert _after(host, "scan_finished", "general_rule_updated_weights")["sparse_dirty"] == 1
    assert _after(host, "scan_finished", "scan_policy_changed")["sparse_dirty"] == 1
