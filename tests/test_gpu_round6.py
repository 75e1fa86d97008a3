"""
Round 6 (``-m gpu``): what the round-5 review found around the device-resident callback loop and the half-width tile kernel's
dispatch; the single-inverse MRAF pass (pre-summed ||w'||) against the two-inverse form it replaces.
"""
import numpy as np
import pytest

from conftest import dispatch_of, force_stepwise, phase_rel_l2, rel_l2, report
from slmsuite_amd import _lib as L
from slmsuite_amd import synth
from slmsuite_amd.holography.algorithms import Hologram, SpotHologram

pytestmark = pytest.mark.gpu


def test_callback_reads_phase_ff_of_a_body_the_general_operators_ran():
    """
    A callback against the device-resident loop whose bodies do NOT run the fused kernels (spot-window feedback on a dense
    launch: the general operators inside the engine call; a shape that is no power of two: Bluestein lines): the engine keeps no previous phase then --
    HGS_PHASE_FF itself is what the body stored, and that is what ``hologram.phase_ff`` has to show at every invocation, as
    the host-driven loop shows it (before round 6 the callback got the host copy of an earlier read, or None).
    """
    def views_of(h, method, name):
        seen = []

        def cb(hh):
            pf = hh.phase_ff
            seen.append(None if pf is None else pf.copy())
            return False

        h.optimize(method, maxiter=4, verbose=False, callback=cb, **({"feedback": "computational_spot"} if "window" in name else {}))
        return seen

    cases = {
        "spot window feedback, dense launches": (lambda: SpotHologram.make_rectangular_array(
            (256, 256), (6, 6), (24, 24), basis="knm", slm_shape=(72, 120), phase=synth.seed_phase(5, (72, 120)),
            engine_options={L.OPT_SPARSE_COLUMNS: 0}), "WGS-Leonardo"),
        "GS 100x150 (Bluestein)": (lambda: Hologram(synth.random_target(4, (100, 150), 0.2, 1.0), phase=synth.seed_phase(4, (40, 60)), slm_shape=(40, 60)), "GS"),
    }
    for name, (make, method) in cases.items():
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fast, slow = make(), force_stepwise(make())
        vf, vs = views_of(fast, method, name), views_of(slow, method, name)
        d = dispatch_of(fast)
        assert d.count("col_fused_kernel") + d.count("col_tile_kernel") + d.count("col_tile2_kernel") == 0, d   # general operators
        assert [v is None for v in vf] == [v is None for v in vs], name
        worst = 0.0
        for k, (a, b) in enumerate(zip(vf, vs)):
            if a is None:
                continue
            assert k == 0 or not np.array_equal(a, vf[k - 1]), (name, k)          # a fresh array per body, not a stale copy
            worst = max(worst, phase_rel_l2(a, b))
        report(f"callback phase_ff on the general operators: {name}", phase_ff=worst)
        assert worst < 5e-4, (name, worst)


def test_callback_phase_assignment_does_not_depend_on_what_it_reads():
    """
    A phase assigned inside a callback is overwritten by the body that follows (_hologram.py:1483-1487) -- whether or not
    the callback looked at ``farfield`` / ``amp_ff`` after assigning it, and what it sees there is the field of the phase the
    body starts from, formed before the callback (:1465-1477).  (Until round 6 a read after the assignment uploaded the
    assigned phase and the body iterated from it.)
    """
    shape, slm = (256, 256), (72, 120)
    other = synth.seed_phase(11, slm)
    seen = {}

    def run(look):
        h = SpotHologram.make_rectangular_array(shape, (6, 6), (24, 24), basis="knm", slm_shape=slm, phase=synth.seed_phase(5, slm))

        def cb(hh):
            if hh.iter == 2:
                before = hh.amp_ff.copy() if look == "before" else None
                hh.phase = other.copy()
                if look == "after":
                    seen["after"] = hh.amp_ff.copy()
                if before is not None:
                    seen["before"] = before
            return False

        h.optimize("WGS-Leonardo", maxiter=5, verbose=False, callback=cb)
        return h.phase.copy(), np.array(h.weights, copy=True)

    p_none, w_none = run(None)
    p_before, w_before = run("before")
    p_after, w_after = run("after")
    np.testing.assert_array_equal(p_none, p_before)
    np.testing.assert_array_equal(p_none, p_after)
    np.testing.assert_array_equal(w_none, w_after)
    np.testing.assert_array_equal(w_none, w_before)
    np.testing.assert_array_equal(seen["before"], seen["after"])


def test_tile_option_off_reaches_the_per_column_kernel_at_2048_rows():
    """HGS_OPT_TILE_KERNEL = 0 is the tests' A/B reference: it has to leave col_tile2_kernel at 2048 rows too (round 5: only
    at 4096), and the two kernels agree to rounding."""
    shape, slm = (2048, 2048), (1080, 1920)
    out = {}
    for tile in (1, 0):
        h = SpotHologram.make_rectangular_array(shape, (8, 8), (64, 64), basis="knm", slm_shape=slm, phase=synth.seed_phase(2, slm),
                                                engine_options={L.OPT_SPARSE_COLUMNS: 0, L.OPT_TILE_KERNEL: tile})
        h.optimize("WGS-Leonardo", maxiter=4, verbose=False)
        d = dispatch_of(h)
        if tile:
            assert d.count("col_tile2_kernel", N=2048) == 4 and d.count("col_fused_kernel") == 0, d
        else:
            assert d.count("col_tile2_kernel") == 0 and d.count("col_fused_kernel", N=2048) == 4, d
        out[tile] = (h.phase.copy(), np.array(h.weights, copy=True))
    assert phase_rel_l2(out[1][0], out[0][0]) < 5e-6 and rel_l2(out[1][1], out[0][1]) < 5e-6


def test_trailing_transform_from_the_kept_g_against_the_stored_phase():
    """
    After a fused float32 loop the last row launch leaves G of the next body behind (row_kernel MODE 3) and the trailing
    transform of optimize() starts from it: amp * v / |v| un-rounded, where a fresh engine (get_farfield's side engine, a new
    hologram) starts from exp(i * stored phase).  The two describe the same field to float32 rounding -- consistent with the
    loop rather than bit-identical with the stored phase (include/hgs.h, HGS_KEEP_G).
    """
    shape, slm = (1024, 1024), (288, 480)
    for sparse in (0, 1):
        h = SpotHologram.make_rectangular_array(shape, (8, 8), (64, 64), basis="knm", slm_shape=slm, phase=synth.seed_phase(9, slm),
                                                engine_options={L.OPT_SPARSE_COLUMNS: sparse})
        h.optimize("WGS-Leonardo", maxiter=6, verbose=False)
        kept = h.farfield.copy()                               # _populate_results, from the G left behind
        d = dispatch_of(h)
        assert d.count("row_kernel", MODE=0) == 1, d           # only the first body built G from a phase
        g = Hologram(np.array(h.target, copy=True), phase=h.phase.copy(), slm_shape=slm)
        fresh = g.get_farfield()                               # exp(i * the stored phase) on an engine of its own
        err = rel_l2(kept, fresh)
        report(f"trailing transform, kept G vs stored phase (sparse={sparse})", farfield=err)
        assert err < 2e-6, err


# ---- MRAF with a weight update and ONE inverse per column (col_presum_kernel + col_tile_kernel RULE 5) ------------------------
def _mraf_target(n, dtype=np.float32):
    t = np.zeros((n, n), dtype=dtype)
    a, b = n // 2 - 3 * n // 16, n // 2 + 3 * n // 16
    t[a:b, a:b] = np.nan
    a, b = n // 2 - n // 8, n // 2 + n // 8
    t[a:b, a:b] = synth.random_target(5, (n // 4, n // 4), 0.2, 1.0, dtype=dtype)
    return t


@pytest.mark.parametrize("n, slm, method, extra, sparse", [
    (4096, (800, 1280), "WGS-Leonardo", {}, 0),                              # SLM rows in 4 register slots
    (4096, (1152, 1920), "WGS-Leonardo", {}, 0),                             # 6-slot instance
    (4096, (800, 1280), "WGS-Kim", dict(fix_phase_iteration=2), 0),          # phase_ff stored (body 2), read back (bodies 3, 4)
    (4096, (1152, 1920), "WGS-Leonardo", {}, 1),                             # engine default: the tile list around the noise box
    (8192, (1152, 1920), "WGS-Leonardo", {}, 0),                             # cfg 5's own geometry (4-slot instance, staged tiles)
])
def test_mraf_single_inverse_matches_the_split_form(n, slm, method, extra, sparse, monkeypatch):
    """
    MRAF with a WGS-Leonardo / WGS-Kim update (_hologram.py:1606-1653 after :1786-1879).  The weights that enter an update
    are normalised, so ||w'||^2 = 1 + D, D = sum over the signal pixels of w'^2 - w^2: a forward-only pre-pass over the
    columns that hold signal pixels forms D (col_presum_kernel) and the column pass rebuilds the field with the FINAL scale
    (col_tile_kernel RULE 5) -- one inverse per column and a plain row launch, where the split form (RULE 3 / 4 + row_kernel
    SPLIT) runs a second inverse in every noise column and joins the parts in the row kernel.  Same algebra, the scale
    applied before instead of after the inverse: bodies 3 .. 5 of a run against the split form on every update
    (HGS_MRAF_PRESUM=0, read by hgs_create).  The first update after new weights (body 2) takes the split form in both.
    """
    target = _mraf_target(n)
    phase0 = synth.seed_phase(7, slm)
    out = {}
    for presum in ("1", "0"):
        monkeypatch.setenv("HGS_MRAF_PRESUM", presum)
        h = Hologram(target, phase=phase0.copy(), slm_shape=slm, dtype=np.float32, engine_options={L.OPT_SPARSE_COLUMNS: sparse})
        h.optimize(method, maxiter=3, verbose=False, mraf_factor=0.5, **extra)
        d = dispatch_of(h)
        lst = ["list"] if sparse else []
        nolst = [] if sparse else ["list"]
        if presum == "1":
            assert d.count("col_presum_kernel", N=n) == 1, d
            assert d.count("col_tile_kernel", N=n, RULE=5, EXTRAS=True, flags=lst, without=nolst) == 1, d
            assert d.count("col_tile_kernel", RULE=3) + d.count("col_tile_kernel", RULE=4) == 1, d        # body 2: weights not yet behind an update
            assert d.count("row_kernel", SPLIT=True) == 1, d
        else:
            assert d.count("col_presum_kernel") == 0 and d.count("col_tile_kernel", RULE=5) == 0, d
            assert d.count("col_tile_kernel", RULE=3) + d.count("col_tile_kernel", RULE=4) == 2 and d.count("row_kernel", SPLIT=True) == 2, d
        three = (h.phase.copy(), np.nan_to_num(np.array(h.weights, copy=True)))
        h.optimize(method, maxiter=2, verbose=False, mraf_factor=0.5, **extra)
        d = dispatch_of(h)
        if presum == "1":      # the state survives the call boundary: both bodies on the single-inverse pass
            assert d.count("col_presum_kernel", N=n) == 2 and d.count("col_tile_kernel", RULE=5) == 2 and d.count("row_kernel", SPLIT=True) == 0, d
        out[presum] = three + (h.phase.copy(), np.nan_to_num(np.array(h.weights, copy=True)))
        if presum == "1":
            # new weights from the host: the next update cannot assume them normalised -- the split form once, then again RULE 5
            h.weights = np.array(h.weights, copy=True) * 3.0
            h.optimize(method, maxiter=2, verbose=False, mraf_factor=0.5, **extra)
            d = dispatch_of(h)
            assert d.count("col_tile_kernel", RULE=3) + d.count("col_tile_kernel", RULE=4) == 1 and d.count("col_tile_kernel", RULE=5) == 1, d
            assert np.all(np.isfinite(h.phase))
        h._release_engine()
    ep3, ew3 = phase_rel_l2(out["1"][0], out["0"][0]), rel_l2(out["1"][1], out["0"][1])
    ep5, ew5 = phase_rel_l2(out["1"][2], out["0"][2]), rel_l2(out["1"][3], out["0"][3])
    nrm = float(np.sqrt(np.sum(out["1"][1].astype(np.float64) ** 2)))
    report(f"single-inverse MRAF vs split {n} {slm} {method} sparse={sparse}", phase_3_bodies=ep3, weights_3_bodies=ew3,
           phase_5_bodies=ep5, weights_5_bodies=ew5, weight_norm=nrm)
    assert np.all(np.isfinite(out["1"][0])) and np.all(np.isfinite(out["1"][2]))
    assert abs(nrm - 1.0) < 2e-6, nrm          # the weights a caller reads are normalised as ever (wscale from the pass' own sums)
    assert ew3 < 1e-6, ew3                     # body 3's update sees the same farfield in both forms
    assert ep3 < 3e-6, ep3                     # ... its rebuilt field differs by where the scale is applied, i.e. by rounding
    assert ep3 > 0                             # (the two forms really are different launches)
    # two more bodies: the pixel-wise rule on a dense image amplifies rounding 50 - 500 x per body (test_single_pass_mraf_...)
    assert ep5 < 5e-2 and ew5 < 5e-2, (ep5, ew5)


def test_mraf_single_inverse_against_the_oracle():
    """Three bodies at 4096 x 4096 (SLM 800 x 600) -- the second and third on the single-inverse pass -- against the
    float64 oracle next to the float32 oracle's own distance from it."""
    from oracle import hgs_oracle as orc
    shape, slm = (4096, 4096), (800, 600)
    t = np.zeros(shape, dtype=np.float32)
    t[1400:2700, 600:1500] = np.nan
    t[1600:2500, 700:1400] = synth.random_target(6, (900, 700), 0.2, 1.0)
    phase0 = synth.seed_phase(8, slm)
    h = Hologram(t, phase=phase0.copy(), slm_shape=slm, dtype=np.float32, engine_options={L.OPT_SPARSE_COLUMNS: 0})
    h.optimize("WGS-Leonardo", maxiter=3, verbose=False, mraf_factor=0.7)
    d = dispatch_of(h)
    assert d.count("col_tile_kernel", N=4096, RULE=5) == 1 and d.count("col_presum_kernel", N=4096) == 1, d
    runs = {}
    for dt in (np.float32, np.float64):
        o = orc.OracleHologram(t.astype(dt), phase=phase0.astype(dt), slm_shape=slm, dtype=dt)
        o.optimize("WGS-Leonardo", maxiter=3, mraf_factor=0.7, populate=False)
        runs[dt] = (o.phase, np.nan_to_num(o.weights))
    yp, yw = phase_rel_l2(runs[np.float32][0], runs[np.float64][0]), rel_l2(runs[np.float32][1], runs[np.float64][1])
    ep, ew = phase_rel_l2(h.phase, runs[np.float64][0]), rel_l2(np.nan_to_num(h.weights), runs[np.float64][1])
    report("single-inverse MRAF vs float64 oracle, 3 bodies", phase=ep, weights=ew, oracle_fp32_vs_fp64_phase=yp, oracle_fp32_vs_fp64_weights=yw)
    assert ep < 3 * yp and ew < 3 * yw, (ep, yp, ew, yw)


def _mraf_frame(shape, dtype, box):
    """A noise frame around an image: NaN rows across the whole width (box False) or a NaN box (few noise columns)."""
    H, W = shape
    t = np.zeros(shape, dtype=dtype)
    r0, r1, c0, c1 = H // 4, 3 * H // 4, W // 2 - W // 6, W // 2 + W // 6
    if box:
        t[r0 - H // 16:r1 + H // 16, c0 - W // 32:c1 + W // 32] = np.nan
    else:
        t[r0 - H // 16:r1 + H // 16, :] = np.nan
    t[r0:r1, c0:c1] = synth.random_target(21, (r1 - r0, c1 - c0), 0.2, 1.0, dtype=dtype)
    return t


@pytest.mark.parametrize("dt, shape, slm", [(np.float64, (64, 4096), (40, 1500)), (np.float64, (256, 8192), (100, 3000)),
                                            (np.float64, (4096, 4096), (600, 900)),
                                            (np.float32, (256, 4096), (100, 1500)),          # short columns: the per-column kernel in float32
                                            (np.float32, (4096, 2048), (800, 600)),          # tile-resident rows, fewer than 4096 columns: the generic tile kernel
                                            (np.float32, (1024, 1024), (300, 400))])
@pytest.mark.parametrize("method, extra", [("WGS-Leonardo", {}), ("WGS-Kim", dict(fix_phase_iteration=2))])
@pytest.mark.parametrize("sparse", [0, 1])
def test_mraf_single_inverse_on_the_per_column_kernel(dt, shape, slm, method, extra, sparse, monkeypatch):
    """
    The same update wherever the fused path runs MRAF outside col_tile_kernel RULE 5: float64 (no tile-resident kernel) and
    the float32 geometries it does not cover.  The per-column kernel makes the pre-pass over the list of signal columns
    (CParams::presum: forward transform + rule, nothing written but D) and the main pass -- col_fused_kernel, or the generic
    tile kernel -- rebuilds with 1 / sqrt(1 + D): two launches and a plain row launch where the split form takes a pass, an
    inverse-only launch over the noise columns and a joining row launch, and the two-pass form two full passes.  Four bodies
    (the third and fourth on the new form) against the old forms (HGS_MRAF_PRESUM=0) and, in float64, against the oracle.
    """
    if shape == (4096, 4096) and (method != "WGS-Leonardo" or sparse):
        pytest.skip("one case at the large float64 size")
    target = _mraf_frame(shape, dt, box=bool(sparse))
    phase0 = synth.seed_phase(17, slm, dtype=dt)
    out = {}
    for presum in ("1", "0"):
        monkeypatch.setenv("HGS_MRAF_PRESUM", presum)
        h = Hologram(target.copy(), phase=phase0.copy(), slm_shape=slm, dtype=dt, engine_options={L.OPT_SPARSE_COLUMNS: sparse})
        h.optimize(method, maxiter=4, verbose=False, mraf_factor=0.5, **extra)
        d = dispatch_of(h)
        if presum == "1":
            assert d.count("col_presum_kernel") == 0 and d.count("col_tile_kernel", RULE=5) == 0, d
            # bodies 2, 3: pre-pass over the signal list (per-column kernel, RULE 0) + ONE main pass + a plain row launch
            assert d.count("col_fused_kernel", N=shape[0], RULE=0, flags=["list"]) >= 2, d
            assert d.count("row_kernel", SPLIT=True) + d.count("col_kernel", MODE=24) <= 2, d          # at most body 1's split form
        out[presum] = (h.phase.copy(), np.nan_to_num(np.array(h.weights, copy=True)), h.amp_ff.copy())
        h._release_engine()
    ep, ew = phase_rel_l2(out["1"][0], out["0"][0]), rel_l2(out["1"][1], out["0"][1])
    errs = dict(phase_vs_old_form=ep, weights_vs_old_form=ew)
    if dt == np.float64:
        from oracle import hgs_oracle as orc
        o = orc.OracleHologram(target.copy(), phase=phase0.copy(), slm_shape=slm, dtype=dt)
        o.optimize(method, maxiter=4, mraf_factor=0.5, **extra)
        errs.update(phase=phase_rel_l2(out["1"][0], o.phase), weights=rel_l2(out["1"][1], np.nan_to_num(o.weights)),
                    amp_ff=rel_l2(out["1"][2], o.amp_ff))
    report(f"single-inverse MRAF, per-column pre-pass {np.dtype(dt).name} {shape} {slm} {method} sparse={sparse}", **errs)
    # (ep may be exactly 0 on a small float32 grid: 1 / sqrt(1 + D) and 1 / sqrt(sum w'^2) round to the same float there and
    #  the two-pass form then multiplies the same numbers in the same order; the dispatch record above is what shows the path)
    assert np.all(np.isfinite(out["1"][0]))
    if dt == np.float64:
        assert max(errs.values()) < 1e-9, errs
    else:
        # float32: two update bodies apart on a dense image (rounding amplified 50 - 500 x per body, see the split-form tests)
        assert ep < 5e-3 and ew < 5e-3, errs


def test_weight_writers_send_one_mraf_update_through_the_old_form_a_target_none():
    """
    Who clears "the stored weights are normalised" (what the single-inverse MRAF update builds on), end to end, at the
    smallest geometry where that form runs: float32, pad (1024, 1024), SLM (300, 400) -- the per-column kernel, pre-pass
    ``col_fused_kernel ... list`` over the signal columns.  Three bodies, then in turn a weight reset, a host upload of
    weights and a new target of the same NaN layout, each followed by two more bodies.

    Launches per two-body call, as the code has it and as measured before the engine's host state was gathered into
    EngineState (the same engine, one commit earlier):
      after reset_weights:  1 pre-pass, 3 unlisted col_fused_kernel launches (body 1 in two passes, body 2 in one), 0 joins
      after h.weights = :   1 pre-pass, 3 unlisted launches, 0 joins
      after a new target:   2 pre-passes, 2 unlisted launches, 0 joins
    (1024 columns are fewer than the split forms take, so the old form here is the two-pass one: ``row_kernel SPLIT`` and
    ``col_kernel MODE=24`` -- how the old form shows at 4096 columns and more -- stay at zero throughout.)
    """
    shape, slm, n = (1024, 1024), (300, 400), 1024
    target = _mraf_frame(shape, np.float32, box=False)
    h = Hologram(target.copy(), phase=synth.seed_phase(17, slm), slm_shape=slm, dtype=np.float32, engine_options={L.OPT_SPARSE_COLUMNS: 0})
    h.optimize("WGS-Leonardo", maxiter=3, verbose=False, mraf_factor=0.5)
    d = dispatch_of(h)
    assert d.count("col_fused_kernel", N=n, RULE=0, flags=["list"]) == 1, d          # body 3: the single-inverse form is running

    def two_bodies():
        h.optimize("WGS-Leonardo", maxiter=2, verbose=False, mraf_factor=0.5)
        d = dispatch_of(h)
        assert np.all(np.isfinite(h.phase))
        got = (d.count("col_fused_kernel", N=n, flags=["list"]), d.count("col_fused_kernel", N=n, without=["list"]),
               d.count("row_kernel", SPLIT=True) + d.count("col_kernel", MODE=24))
        print("dispatch after", got, "\n", d)
        return got

    h.reset_weights()
    assert two_bodies() == (1, 3, 0)
    h.weights = np.array(h.weights, copy=True) * 3.0
    assert two_bodies() == (1, 3, 0)
    other = target.copy()
    other[np.isfinite(target) & (target > 0)] = synth.random_target(22, shape, 0.2, 1.0)[np.isfinite(target) & (target > 0)]
    h.set_target(other)
    assert two_bodies() == (2, 2, 0)
    h._release_engine()


def test_fixed_phase_without_a_stored_phase_on_an_mraf_target_raises_like_the_reference():
    """
    Reference quirk A12: a WGS-Kim run fixes the phase, ``reset()`` keeps the flags and forgets ``phase_ff``;
    with NaN in the target the next run's first iteration evaluates ``exp(1j * None)`` (_hologram.py:1643 has no
    ``or self.phase_ff is None`` as :1601 has) -- TypeError in the reference and in the oracle, a RuntimeError that says why
    in the class, before anything is touched.  Without NaN in the target the same state is guarded in both (:1601) and runs.
    """
    from oracle import hgs_oracle as orc
    shape, slm = (64, 128), (40, 100)
    for mraf in (True, False):
        target = synth.random_target(3, shape, 0.2, 1.0, dtype=np.float64)
        if mraf:
            target[:12, :] = np.nan
        phase = synth.seed_phase(3, slm, dtype=np.float64)
        h = Hologram(target.copy(), phase=phase.copy(), slm_shape=slm, dtype=np.float64)
        o = orc.OracleHologram(target.copy(), phase=phase.copy(), slm_shape=slm, dtype=np.float64)
        for x in (h, o):
            kw = {} if x is o else {"verbose": False}
            x.optimize("WGS-Kim", maxiter=3, fix_phase_iteration=1, **kw)
        assert h.flags["fixed_phase"] and o.flags["fixed_phase"]
        h.reset(reset_phase=False, reset_flags=False)
        o.reset()
        assert h.phase_ff is None and o.phase_ff is None and h.flags["fixed_phase"] and o.flags["fixed_phase"]
        if mraf:
            with pytest.raises(TypeError):                         # (iteration 0 of a call: no weight update, so no rule clears the flag)
                o.optimize("WGS-Leonardo", maxiter=2)
            for method in ("GS", "WGS-Leonardo", "WGS-Kim"):
                with pytest.raises(RuntimeError, match="phase_ff"):
                    h.optimize(method, maxiter=2, verbose=False)
                assert h.iter == 0 and h.phase_ff is None
            h.flags["fixed_phase"] = False                         # what the message says: the run goes through
            h.optimize("GS", maxiter=2, verbose=False)
        else:
            h.optimize("GS", maxiter=2, verbose=False)
            o.optimize("GS", maxiter=2)
            assert phase_rel_l2(h.phase, o.phase) < 1e-9
        h._release_engine()
