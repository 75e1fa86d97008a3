"""
Column flags in the half-width tile kernel (``-m gpu``): on a target with few active columns whose scan is current,
``col_tile2_kernel`` requests weights and targets only in the columns where the scan found any (``HGS_OPT_EMPTY_COL_LOADS``,
default on); every other column reads as the zeros it holds through an empty buffer resource.  The registers are the same
either way, so everything here is compared BYTE FOR BYTE against the same engine with the option off, next to the dispatch
record (the ``col_flags`` flag of the launch says whether the flags went with it).

Small pads that the kernel accepts: 4096 rows x 256 columns (SLM 1152 x 120: five register slots, the parked
next-tile-ahead instance for one hologram, the register form for a batch) and 2048 rows x 256 columns (SLM 1080 x 120: two
lane groups per workgroup).  The 2048-row form keeps its plain loads -- it measured slower with the resource form -- so at
2048 rows both sides of every comparison run the same code: those cases only guard against the flags leaking into that form
(the dispatch record must not show them there).  Sparse columns are off unless a test says otherwise: the dense launches are
what the flags are for.
"""
import numpy as np
import pytest

from conftest import dispatch_of, phase_rel_l2, rel_l2, report
from oracle import hgs_oracle as orc
from slmsuite_amd import _lib as L
from slmsuite_amd import synth
from slmsuite_amd.batch import HologramBatch
from slmsuite_amd.holography.algorithms import Hologram, SpotHologram

pytestmark = pytest.mark.gpu

GEOMETRIES = {4096: ((4096, 256), (1152, 120)), 2048: ((2048, 256), (1080, 120))}


def spots(n, cols=(5, 130, 255)):
    """Eight spots in three columns (x, y).  A lane of the column kernel holds rows j, j + T, ... (T = n / 16) as 64
    contiguous bytes, fetched as four 16-byte quarters: row n - 1 is the last row of the pad (last lane, last quarter, the
    end of the column's buffer resource), row 13 T + 17 is alone in the last quarter of lane 17, rows 40 and 2 T + 40 share
    lane 40 in other quarters.  Column 255 is the last byte of the last flag word."""
    t = n // 16
    a, b, c = cols
    xy = [(a, n - 1), (a, 100), (a, 7 * t + 3), (b, 13 * t + 17), (b, 40), (b, 2 * t + 40), (c, n // 2), (c, 9)]
    return np.array(xy, dtype=float).T


def options(on):
    return {L.OPT_SPARSE_COLUMNS: 0, L.OPT_EMPTY_COL_LOADS: 1 if on else 0}


def spot_hologram(n, on, seed=3, cols=(5, 130, 255)):
    shape, slm = GEOMETRIES[n]
    return SpotHologram(shape, spots(n, cols), basis="knm", slm_shape=slm, phase=synth.seed_phase(seed, slm), engine_options=options(on))


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_pair(on, off, what, updates):
    """phase and weights of the two holograms agree byte for byte; both ran col_tile2_kernel, `on` with the flags wherever
    the pass followed a current scan (every launch here), `off` never."""
    d_on, d_off = dispatch_of(on), dispatch_of(off)
    assert d_on.count("col_tile2_kernel") == updates and d_off.count("col_tile2_kernel") == updates, (what, d_on, d_off)
    # (the flags go with the 4096-row instances; the 2048-row form keeps its plain loads: it measured slower with them)
    assert d_on.count("col_tile2_kernel", flags=["col_flags"], N=4096) == d_on.count("col_tile2_kernel", N=4096), (what, d_on)
    assert d_on.count("col_tile2_kernel", flags=["col_flags"], N=2048) == 0, (what, d_on)
    assert d_off.count("col_tile2_kernel", flags=["col_flags"]) == 0, (what, d_off)
    assert same_bytes(on.phase, off.phase), what
    assert same_bytes(on.weights, off.weights), what


@pytest.mark.parametrize("method", ["WGS-Leonardo", "GS"])
@pytest.mark.parametrize("n", [4096, 2048])
def test_on_and_off_agree_byte_for_byte(n, method):
    on, off = spot_hologram(n, True), spot_hologram(n, False)
    for h in (on, off):
        h.optimize(method, maxiter=3, verbose=False)
    assert_pair(on, off, (n, method), 3)


def test_headline_instance_is_the_one_that_takes_the_flags():
    h = spot_hologram(4096, True)
    h.optimize("WGS-Leonardo", maxiter=3, verbose=False)
    d = dispatch_of(h)
    assert d.count("col_tile2_kernel", flags=["col_flags"], N=4096, NR=5, PARK="true", NXF="true") == 3, d
    w = h.weights
    xy = spots(4096).astype(int)
    assert np.count_nonzero(w) == 8 and np.all(w[xy[1], xy[0]] > 0)       # the eight spots kept their weights, nothing else has one


def test_batch_of_two_with_different_targets():
    """Flags are per hologram: column 130 holds spots of hologram 0 and nothing of hologram 1, column 77 the reverse."""
    shape, slm = GEOMETRIES[4096]
    cols = [(5, 130, 255), (77, 201, 255)]
    targets = np.zeros((2,) + shape, dtype=np.float32)
    for b in range(2):
        xy = spots(4096, cols[b]).astype(int)
        targets[b, xy[1], xy[0]] = 1 + 0.1 * np.arange(xy.shape[1])
    phases = np.stack([synth.seed_phase(60 + b, slm) for b in range(2)])
    out = []
    for on in (True, False):
        hb = HologramBatch(shape, slm, targets, phases)
        for opt, val in options(on).items():
            hb.set_option(opt, val)
        hb.optimize("WGS-Leonardo", 3)
        d = dispatch_of(hb)
        assert d.count("col_tile2_kernel", flags=["batch"], N=4096, PARK="false") == 3, d
        assert d.count("col_tile2_kernel", flags=["batch", "col_flags"]) == (3 if on else 0), d
        out.append((hb.phases(), hb.engine.get(L.WEIGHTS)))
        hb.close()
    assert same_bytes(out[0][0], out[1][0]) and same_bytes(out[0][1], out[1][1])
    w = out[0][1]
    for b in range(2):
        xy = spots(4096, cols[b]).astype(int)
        assert np.count_nonzero(w[b]) == 8 and np.all(w[b][xy[1], xy[0]] > 0), b


@pytest.mark.parametrize("n", [4096, 2048])
def test_state_changes_between_calls(n):
    """Whatever writes weights or target between two calls makes the next call scan again: a weight (finite, then NaN) put
    into a column that held nothing, spots moved with the old weights kept, weights reset."""
    on, off = spot_hologram(n, True), spot_hologram(n, False)
    pair = (on, off)

    def run(what, bodies=2):
        for h in pair:
            h.optimize("WGS-Leonardo", maxiter=bodies, verbose=False)
        assert_pair(on, off, (n, what), bodies)

    run("start", 3)
    for col, value, what in ((64, 0.37, "weight in an empty column"), (190, np.nan, "NaN weight in an empty column")):
        for h in pair:
            w = np.array(h.weights, copy=True)
            assert not w[:, col].any() and not h.target[:, col].any()
            w[n - 1, col] = value
            h.set_weights(w)
        run(what)
        assert on.weights[n - 1, col] != 0           # (the pixel took part: a weight the rule keeps, or 1e-4 for the NaN)
    for h in pair:                                    # spots move three columns to the right (the last column wraps to 2)
        h.spot_knm = spots(n, (8, 133, 2))
        h.set_target(reset_weights=False)
    run("spots moved")
    for h in pair:
        h.reset_weights()
    run("weights reset")
    assert np.count_nonzero(on.weights) == 8


def test_flags_return_after_spot_feedback():
    """The N-vector rule of the spot feedback modes writes weights at the spot pixels behind the scan's back (sparse columns on:
    the spot columns as a list).  The flags are withheld from then on, and the next dense call scans again before it passes
    them: it runs with the flags, and on and off agree byte for byte."""
    n = 4096
    shape, slm = GEOMETRIES[n]
    t = n // 16
    xy = np.array([(5, n - 3), (5, 100), (5, 7 * t + 3), (130, 13 * t + 17), (130, 40), (130, 2 * t + 40), (250, n // 2), (250, 9)], dtype=float).T
    pair = [SpotHologram(shape, xy, basis="knm", slm_shape=slm, phase=synth.seed_phase(5, slm), engine_options={L.OPT_EMPTY_COL_LOADS: v})
            for v in (1, 0)]
    on, off = pair
    for h in pair:
        h.optimize("WGS-Leonardo", maxiter=3, verbose=False, feedback="computational_spot")
    d = dispatch_of(on)
    assert d.count("col_fused_kernel", flags=["list"]) == 3 and d.count("col_tile2_kernel") == 0, d
    dispatch_of(off)
    for h in pair:
        h.engine_options[L.OPT_SPARSE_COLUMNS] = 0
        h._engine.set_option(L.OPT_SPARSE_COLUMNS, 0)
        h.optimize("WGS-Leonardo", maxiter=2, verbose=False, feedback="computational")
    assert_pair(on, off, "dense call after spot feedback", 2)


def test_dense_image_is_left_alone():
    """A dense random image never receives the flags: the option changes neither the dispatch record nor a byte."""
    shape, slm = GEOMETRIES[4096]
    out = []
    for on in (True, False):
        h = Hologram(synth.random_target(11, shape, 0.2, 1.0), phase=synth.seed_phase(4, slm), slm_shape=slm, engine_options=options(on))
        h.optimize("WGS-Leonardo", maxiter=3, verbose=False)
        d = dispatch_of(h)
        assert d.count("col_tile2_kernel", N=4096, PARK="true", NXF="false") == 3 and d.count("col_tile2_kernel", flags=["col_flags"]) == 0, d
        out.append((sorted((r["name"], tuple(sorted(r["flags"])), r["count"]) for r in d.records), h.phase, h.weights))
    assert out[0][0] == out[1][0]
    assert same_bytes(out[0][1], out[1][1]) and same_bytes(out[0][2], out[1][2])


def test_one_body_against_the_oracle():
    """One teacher-forced WGS-Leonardo body (the third: it updates the weights) with the flags on, against the CPU oracle
    from the same state; bounds of tests/test_gpu_parity.py::test_single_step_matches_reference (phase phasors 5e-6,
    weights 3e-6, relative L2)."""
    n = 4096
    shape, slm = GEOMETRIES[n]
    phase0 = synth.seed_phase(3, slm)
    o = orc.OracleSpotHologram(shape, spots(n), slm_shape=slm, phase=phase0.copy())
    o.optimize("WGS-Leonardo", maxiter=2, populate=False)
    p2, w2 = o.phase.copy(), o.weights.copy()
    o.optimize("WGS-Leonardo", maxiter=1, populate=False)
    h = spot_hologram(n, True)
    h.phase, h.weights, h.iter = p2.copy(), w2.copy(), 2
    h.stats["method"] = ["WGS-Leonardo"] * 2
    h.stats["flags"]["fixed_phase"] = [False] * 2
    h.optimize("WGS-Leonardo", maxiter=1, verbose=False)
    d = dispatch_of(h)
    assert d.count("col_tile2_kernel", flags=["col_flags"], RULE=1, NXF="true") == 1, d
    ep, ew = phase_rel_l2(h.phase, o.phase), rel_l2(h.weights, o.weights)
    report("empty-column loads, one body vs oracle", phase=ep, weights=ew)
    assert ep < 5e-6 and ew < 3e-6
