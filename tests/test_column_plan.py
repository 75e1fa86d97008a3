"""
The fused loop's decision, without a GPU: ``slmsuite_amd/csrc/column_plan.hpp`` is plain C++ (no HIP), so the table the
dispatch tests observe on the device (tests/test_dispatch.py and the ``dispatch_of`` assertions of the round tests) is
checked here on the plan itself, and the plan's invariants over a swept grid of facts.  This file asserts what the plan
SAYS; the GPU dispatch tests keep asserting what was LAUNCHED.

Device facts are inputs: 256 CUs and the block counts hgs_create derives from them (tests/column_plan_host.cpp,
derive_blocks).  Geometry as the Python classes make it: a centred SLM block, r0 = (Ph - Sh) // 2.
"""
import os
import subprocess

from plan_host import GS, KIM, LEONARDO, NOGRETTE, ROOT, TANH, WU, host, plan  # noqa: F401  (host: the fixture)


def _plan(exe, **facts):
    facts.setdefault("Pw", facts["Ph"])
    return plan(exe, **facts)


# a dense image whose columns were scanned (HGS_OPT_SPARSE_COLUMNS = 1 finds every column active): what Hologram(...) gives
def _image(n, sh, **kw):
    return dict(dict(elem=4, Ph=n, Sh=sh, B=1, n_active_min=n, n_active_max=n, method=LEONARDO), **kw)


def _sub(d, **want):
    got = {k: d[k] for k in want}
    assert got == want, d


def test_header_includes_no_hip():
    src = open(os.path.join(ROOT, "slmsuite_amd", "csrc", "column_plan.hpp")).read()
    assert "hip/" not in src and "__global__" not in src and "hipLaunch" not in src


def test_dense_image_by_size_and_precision(host):
    """tests/test_dispatch.py::test_dense_image_reaches_the_kernel_of_its_size_and_precision"""
    # 4096^2 fp32, 1032 SLM rows from row 1532, one hologram, WGS-Leonardo: tile2, NR 5, RULE 2 then RULE 1
    for upd, rule in ((0, 2), (1, 1)):
        p = _plan(host, **_image(4096, 1032, do_update=upd))
        _sub(p["main"], family="tile2", nr=5, shift=1520, rule=rule, phase_mode=0, grid=768, half_xmap=1, listed=0, few_active=0)
        _sub(p, nog=0, presum=0, presum_col=0, second_pass=0, join="none", last_mode=3, finalize=upd, wpartial_n=768, scale_after_main=0)
    p = _plan(host, **_image(2048, 520, do_update=1))
    _sub(p["main"], family="tile2", rule=1, grid=512, half_xmap=0)
    assert p["main"]["nr"] <= 8         # (the launcher rounds up to the eight-slot instance)
    for upd, fam in ((0, "fused_rule2"), (1, "fused_rule1")):
        p = _plan(host, **_image(512, 136, do_update=upd))
        _sub(p["main"], family=fam, grid=p["col_blocks"])
    for n in (1024, 4096):             # float64: the generic per-column kernel, the tile-resident kernel is fp32 only
        for upd in (0, 1):
            p = _plan(host, **_image(n, n // 4 + 8, elem=8, do_update=upd))
            _sub(p["main"], family="fused", rule=0, grid=p["col_blocks"])
            _sub(p, last_mode=1)


def test_tall_slm_leaves_the_tile_kernel(host):
    """tests/test_dispatch.py::test_tall_slm_leaves_the_tile_kernel: more than six register slots -> per-column kernel"""
    _sub(_plan(host, **_image(4096, 1800, do_update=1))["main"], family="fused_rule1", listed=0)
    _sub(_plan(host, **_image(4096, 1500, do_update=1))["main"], family="tile2", nr=6)


def test_rule_follows_the_method(host):
    """tests/test_dispatch.py::test_rule_specialisation_follows_the_method (4096^2, 1152 SLM rows)"""
    for m in (GS, KIM, WU, TANH, NOGRETTE):
        _sub(_plan(host, **_image(4096, 1152, method=m, do_update=0))["main"], family="tile2", rule=2, nr=5)
    # WGS-Kim's updating bodies store the farfield phase: col_tile_kernel RULE 1, PHASE 1
    _sub(_plan(host, **_image(4096, 1152, method=KIM, do_update=1, store_phase=1))["main"], family="tile_rule", rule=1, phase_mode=1, nr=5, grid=512)
    # ... and with a fixed phase one hologram reads it in the half-width kernel (HGS_TILE2_PHASE2), a batch does not
    _sub(_plan(host, **_image(4096, 1152, method=KIM, do_update=1, use_fixed=1))["main"], family="tile2", phase_mode=2)
    _sub(_plan(host, **_image(4096, 1152, method=KIM, do_update=1, use_fixed=1, HGS_TILE2_PHASE2=0))["main"], family="tile_rule", phase_mode=2)
    _sub(_plan(host, **_image(4096, 1152, method=KIM, do_update=1, use_fixed=1, B=3))["main"], family="tile_rule", phase_mode=2)
    for m in (WU, TANH):
        _sub(_plan(host, **_image(4096, 1152, method=m, do_update=1))["main"], family="tile", rule=0)
    p = _plan(host, **_image(4096, 1152, method=NOGRETTE, do_update=1))
    _sub(p, nog=1, need_nog_dev=1, finalize=1)
    _sub(p["nog_pass"], family="tile_extras", nog_pass=1, weights_only=1, phase_mode=0)
    _sub(p["main"], family="tile", rule=0, use_nog=1, nog_pass=0)


def test_batch_runs_the_half_width_kernel_with_its_xcd_map(host):
    """tests/test_dispatch.py::test_batches_carry_the_batch_flag_and_keep_one_row_workgroups"""
    for upd, rule in ((0, 2), (1, 1)):
        p = _plan(host, **_image(4096, 1152, B=3, do_update=upd, sparse_dirty=1, n_active_min=0, n_active_max=0, HGS_OPT_SPARSE_COLUMNS=0))
        _sub(p["main"], family="tile2", nr=5, rule=rule, half_xmap=1, grid=256, few_active=0)


def test_statistics_and_spot_columns(host):
    p = _plan(host, **_image(4096, 1152, do_update=1, stat_groups=1))
    _sub(p["main"], family="tile_stats", stats=1)
    p = _plan(host, **_image(512, 136, do_update=1, stat_groups=3))
    _sub(p["main"], family="fused_stats", stats=3)
    # a spot array: column list, per-column kernel with the XCD map of its list groups; spot statistics from the dilated columns
    p = _plan(host, **_image(1024, 288, do_update=1, stat_groups=2, sparse_enabled=1, n_active_min=8, n_active_max=8))
    _sub(p, dilated_forward=1)
    _sub(p["main"], family="fused_rule1", listed=1, stats=0, grid=2, list_xmap=0)
    p = _plan(host, **_image(4096, 1152, do_update=1, sparse_enabled=1, n_active_min=64, n_active_max=64))
    _sub(p["main"], family="fused_rule1", listed=1, grid=64, list_xmap=1)
    # few active columns, dense launch (HGS_OPT_SPARSE_COLUMNS = 0): the NXF instance of the half-width kernel
    _sub(_plan(host, **_image(4096, 1152, do_update=1, n_active_min=64, n_active_max=64, HGS_OPT_SPARSE_COLUMNS=0))["main"], family="tile2", few_active=1)


def _mraf(**kw):
    # cfg 5: 4096^2 fp32, 1152 SLM rows, a signal window inside a noise box: a quarter of the columns hold signal
    return _image(4096, 1152, **dict(dict(mraf=1, do_update=1, n_noise_max=3072, n_signal_max=1024, n_active_min=3072, n_active_max=3072,
                                          HGS_OPT_SPARSE_COLUMNS=0), **kw))


def test_mraf_update_forms(host):
    """tests/test_gpu_round3.py / round4 / round6: split + join, pre-sum, two passes, and the switches that select them"""
    # first update after new weights (w_unit false): one pass, signal and noise part apart, joined by the row launch
    p = _plan(host, **_mraf(w_unit=0))
    _sub(p["main"], family="tile_split", rule=3, rule_ok=1, gh2_sparse=1, nr=5, grid=512)
    _sub(p, presum=0, presum_col=0, second_pass=0, scale_after_main=1, finalize=0, join="gh2", gh2_mask=1, last_mode=1, need_gh2=1)
    # later updates (w_unit): pre-sum over the signal columns, ONE inverse per column (RULE 5), nothing to join
    p = _plan(host, **_mraf(w_unit=1))
    _sub(p["main"], family="tile_presum", rule=5, n_dpartial=512, nr=5)
    _sub(p, presum=1, presum_col=0, prepass_grid=512, scan_flags=1, scan_signal=0, second_pass=0, scale_after_main=0, finalize=1, join="none",
         last_mode=3, need_gh2=0, need_dpartial=1)
    # bodies without an update: the rule-free MRAF instance
    _sub(_plan(host, **_mraf(do_update=0))["main"], family="tile_presum", rule=6)
    # other rules, in-pass statistics, HGS_MRAF_PRESUM=0: the split form on every update
    for kw in (dict(method=WU), dict(stat_groups=1), dict(HGS_MRAF_PRESUM=0)):
        p = _plan(host, **_mraf(w_unit=1, **kw))
        assert p["main"]["family"] in ("tile_split", "tile_split_stats") and p["join"] == "gh2" and not p["presum"], p
    _sub(_plan(host, **_mraf(do_update=0, HGS_MRAF_PRESUM=0))["main"], family="tile_extras")
    # HGS_MRAF_SPLIT=0: two passes (weights only, then rebuild + inverse), wscale in between
    p = _plan(host, **_mraf(w_unit=0, HGS_MRAF_SPLIT=0))
    _sub(p, second_pass=1, scale_after_main=1, finalize=0, join="none", last_mode=3)
    _sub(p["main"], family="tile_extras", weights_only=1, phase_mode=0, do_update=1)
    _sub(p["second"], do_update=0, weights_only=0)
    # HGS_GH2_MASK=0: the noise part stored / read in every column
    p = _plan(host, **_mraf(w_unit=0, HGS_GH2_MASK=0))
    _sub(p["main"], family="tile_split", gh2_sparse=0)
    _sub(p, join="gh2", gh2_mask=0)
    # float64: per-column kernel, noise part through the farfield buffer, inverse-only launch over the noise columns
    p = _plan(host, **_mraf(elem=8, w_unit=0))
    _sub(p["main"], family="fused", split64=1)
    _sub(p, scan_noise=1, need_ffb=1, need_gh2=1, join="gh2_noise_only", gh2_mask=1, noise_inverse_grid=768, last_mode=1, scale_after_main=1)
    # ... the device cannot give that buffer: two passes
    _sub(_plan(host, **_mraf(elem=8, w_unit=0, ffb_unavailable=1)), second_pass=1, need_ffb=0, join="none", noise_inverse_grid=0)
    _sub(_plan(host, **_mraf(elem=8, w_unit=0, HGS_MRAF_SPLIT64=0)), second_pass=1, scan_noise=0, join="none")
    # ... a column list of which more than half holds noise (a noise box): two passes too
    _sub(_plan(host, **_mraf(elem=8, w_unit=0, sparse_enabled=1, n_active_min=1024, n_active_max=1024, n_noise_max=1024)), second_pass=1, join="none")
    _sub(_plan(host, **_mraf(elem=8, w_unit=0, sparse_enabled=1, n_active_min=1024, n_active_max=1024, n_noise_max=256)), second_pass=0, join="gh2_noise_only")
    # float64 with normalised weights: per-column pre-pass over the signal list, one pass, nothing to join
    p = _plan(host, **_mraf(elem=8, w_unit=1))
    _sub(p, presum=0, presum_col=1, scan_signal=1, scan_noise=0, second_pass=0, join="none", finalize=1, need_ffb=0, need_gh2=0, need_dpartial=1)
    _sub(p["main"], family="fused", split64=0, n_dpartial=p["prepass_grid"])
    # ... without a single signal column: two plain passes
    _sub(_plan(host, **_mraf(elem=8, w_unit=1, n_signal_max=0)), presum_col=0, second_pass=1)


def test_column_lists_and_tile_switches(host):
    # an MRAF noise box fills its 4-column tiles: the tile kernels walk the list of whole tiles (tests/test_gpu_round3.py)
    lst = dict(sparse_enabled=1, sparse_tiles=1, n_active_min=1024, n_active_max=1024, HGS_OPT_SPARSE_COLUMNS=1)
    p = _plan(host, **_mraf(w_unit=0, **lst))
    _sub(p["main"], family="tile_split", listed=1, col_flags=1, grid=256, gh2_sparse=0)
    _sub(p, join="gh2", gh2_mask=0)
    _sub(_plan(host, **_image(4096, 1152, do_update=1, **lst))["main"], family="tile_rule_listed", rule=1, listed=1, grid=256)
    # HGS_TILE_LIST=0 (the scan never rounds to tiles): the per-column kernel walks the list
    lst0 = dict(lst, sparse_tiles=0, HGS_TILE_LIST=0)
    _sub(_plan(host, **_image(4096, 1152, do_update=1, **lst0))["main"], family="fused_rule1", listed=1, list_xmap=1)
    # HGS_TILE2_MIN_BATCH=2: single holograms at 4096 rows on col_tile_kernel; HGS_TILE_SHIFT16=0 HGS_TILE_NR4=0: whole-slot
    # shift, six-slot instance (tests/test_gpu_round5.py)
    _sub(_plan(host, **_image(4096, 1032, do_update=1, HGS_TILE2_MIN_BATCH=2))["main"], family="tile_rule", rule=1, nr=5, shift=1520)
    _sub(_plan(host, **_image(4096, 1032, do_update=1, HGS_TILE2_MIN_BATCH=2, HGS_TILE_SHIFT16=0, HGS_TILE_NR4=0))["main"],
         family="tile_rule", rule=1, nr=6, shift=1280)
    _sub(_plan(host, **_image(4096, 1032, do_update=1, HGS_TILE2=0))["main"], family="tile_rule", rule=1)
    _sub(_plan(host, **_image(4096, 1032, do_update=1, HGS_TILE2_MIN_BATCH=2, HGS_TILE_RULE=0))["main"], family="tile", rule=0)
    # HGS_OPT_TILE_KERNEL=0: the per-column kernel at every size (the tests' A/B reference)
    for n, sh in ((4096, 1032), (2048, 520), (8192, 2304)):
        _sub(_plan(host, **_image(n, sh, do_update=1, HGS_OPT_TILE_KERNEL=0))["main"], family="fused_rule1")
    _sub(_plan(host, **_image(8192, 2304, do_update=1))["main"], family="tile_rule", rule=1, grid=256)
    _sub(_plan(host, **_image(4096, 1032, do_update=1, HGS_KEEP_G=0)), last_mode=1)


def test_row_close_between_bodies_of_the_headline(host):
    """plan_row_close on the cfg-2-like body: zeros for the empty columns between two such bodies, never from the last launch
    of a call (it leaves G of every column, MODE 3), never ahead of a WGS-Kim body that stores the farfield phase."""
    middle = plan(host, preset="cfg2")["close_next"]
    last = plan(host, preset="cfg2")["close_last"]
    before_kim = plan(host, preset="cfg2", method=KIM, next=dict(store_phase=1))["close_next"]
    assert middle["zero_par"] >= 0 and last["zero_par"] == -1 and before_kim["zero_par"] == -1
    _sub(middle, mode=2, finalize=1, wslot_fold=1, load_sparse=0, store_sparse=0, zero_par=0)     # (r0 = shift = 1472)
    _sub(last, mode=3, finalize=1, wslot_fold=1, load_sparse=0, store_sparse=0)
    _sub(before_kim, mode=2, finalize=1, wslot_fold=1, load_sparse=0, store_sparse=0)
    # the body that finds the zeros: walks past empty half tiles along the scan's list; one that finds none does neither
    _sub(plan(host, preset="cfg2", gh_prezeroed=1)["main"]["empty"], skip_inverse=1, skip_forward=1, prezeroed=1, list_walk=1)
    _sub(plan(host, preset="cfg2")["main"]["empty"], skip_inverse=1, skip_forward=1, prezeroed=0, list_walk=0)
    # a column list: masks on both sides, the spot statistics' dilated columns stored; MODE 3 stores every column
    lst = dict(elem=4, Ph=1024, Sh=288, B=1, method=LEONARDO, do_update=1, sparse_enabled=1, n_active_min=8, n_active_max=8)
    _sub(_plan(host, **lst)["close_next"], mode=2, load_sparse=1, store_sparse=1, zero_par=-1, wslot_fold=0)
    _sub(_plan(host, stat_groups=2, **lst)["close_next"], load_sparse=1, store_sparse=2)
    _sub(_plan(host, **lst)["close_last"], mode=3, load_sparse=1, store_sparse=0)
    _sub(_plan(host, HGS_KEEP_G=0, **lst)["close_last"], mode=1, load_sparse=1, store_sparse=1)


def test_dense_scan_per_upload(host):
    """The scan ahead of dense launches: fp32 at 4096 rows with the half-width kernel; one hologram always (it picks the
    few-active instance), a batch for the column flags alone -- not with the loads switch off or under MRAF."""
    for facts, scan, rescan in ((dict(), 1, 1), (dict(B=8), 1, 1), (dict(HGS_OPT_EMPTY_COL_LOADS=0), 1, 0), (dict(B=8, HGS_OPT_EMPTY_COL_LOADS=0), 0, 0),
                                (dict(B=8, mraf=1), 0, 0), (dict(mraf=1), 1, 1), (dict(HGS_TILE2=0), 0, 0), (dict(elem=8), 0, 0),
                                (dict(Ph=2048, Sh=520), 0, 0), (dict(Ph=8192, Pw=8192, Sh=2304), 0, 0)):
        assert plan(host, preset="cfg2", **facts)["dense_scan"] == dict(scan=scan, rescan_outside=rescan), facts


def test_invariants_over_a_swept_grid_of_facts(host):
    """Element size x padded rows x SLM rows x batch x method x MRAF x update x phase mode x statistics x column policy x
    w_unit x noise / signal columns, with every A/B switch off in turn.  Each invariant is a guard or a comment of the engine:
    no tile family for 8-byte elements (the tile-resident kernels are fp32 only); tile2 only on plain dense passes; the pre-sum
    forms only with normalised weights (w_unit), an update, Leonardo / Kim and no in-pass statistics; a joining row launch if
    and only if a split form ran; MODE 3 as the last row launch only for 4-byte elements without a join; every grid within
    max(col_blocks, tile_blocks, 3 x #CU) per hologram (what wpartial, dpartial and the statistics partials are sized for);
    exactly one of {two passes, tile split, column split, tile pre-sum, column pre-sum} per MRAF update and none otherwise;
    the weight norm folded exactly once per update; every form preceded by the column scan it consults; no weight-norm slots
    ahead of a per-workgroup reduction (scale_after_main); each empty-column level only on the one below it (list walk, zeros
    in place, forward skipped, inverse skipped, the scan's flags), none of them nor the slots outside tile2 or outside the main
    launch where they count on the row launch before; the closing row launch stores zeros only between two bodies, as a plain
    MODE 2 launch without masks or a join, and only for a next body whose plan accepts them.  The column policies include dense
    launches with few active columns (the flags go with the launch), with zeros left ahead of every body that accepts them
    and with a weight written behind the scan."""
    r = subprocess.run([host, "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tail = r.stdout.strip().splitlines()
    assert tail and tail[-1].startswith("checked "), r.stdout[-2000:]
    n_checked, n_bad = int(tail[-1].split()[1]), int(tail[-1].split()[3])
    assert n_bad == 0, "\n".join(tail[:40])
    assert n_checked > 1_000_000, tail[-1]
