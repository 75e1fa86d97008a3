"""
Empty columns of the half-width tile kernel skip their inverse transform (``-m gpu``): in a column whose scan byte has bit 0
clear every pixel's weight and target are zero, the constrained farfield of the column is exactly zero, and so is its
inverse transform.  With ``HGS_OPT_EMPTY_COL_INVERSE`` (default on) ``col_tile2_kernel`` skips the rule block and the
inverse of such a column and writes ``+0`` into H where the inverse would have written ``+-0``.  With the option off the
kernel takes the same flags and runs every inverse, so everything here is compared BYTE FOR BYTE between the two, next to
the dispatch record (``zero_inv`` says that the launch skips).

A skipped column that left its forward-transformed G in H, or that wrote nothing, changes the phase after the row pass: the
byte comparison of the phase is the check that zeros are written.  Every row of H also holds non-zero columns, so the sign of
a zero in H does not reach the sums of the row transform.

Geometry of ``test_gpu_empty_column_loads.py``: pad 4096 x 256, SLM 1152 x 120 (five register slots).  Sparse columns off,
empty-column loads on, on both sides of every pair.
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

N = 4096
SHAPE, SLM = (N, 256), (1152, 120)
T = N // 16
# A tile is four columns, a workgroup transforms one half of it (two columns) at a time.
#   columns 0 and 3: tile 0 has half 0 as (flagged, empty) and half 1 as (empty, flagged)
#   columns 128 and 129: both columns of one half flagged
#   column 255: the last byte of the last flag word
#   every other tile is entirely empty
COLS = (0, 3, 128, 129, 255)


def spots(cols=COLS):
    """Ten spots in five columns (x, y): row N - 1 is the last row of the pad, row 13 T + 17 is alone in the last quarter
    of lane 17 (as in test_gpu_empty_column_loads.py)."""
    a, b, c, d, e = cols
    xy = [(a, N - 1), (a, 100), (a, 7 * T + 3), (b, 13 * T + 17), (b, 40), (c, 2 * T + 40), (c, N // 2), (d, 9),
          (d, 5 * T + 77), (e, N // 2 + 1), (e, 300)]
    return np.array(xy, dtype=float).T


def options(on):
    return {L.OPT_SPARSE_COLUMNS: 0, L.OPT_EMPTY_COL_LOADS: 1, L.OPT_EMPTY_COL_INVERSE: 1 if on else 0}


def spot_hologram(on, seed=3, cols=COLS):
    return SpotHologram(SHAPE, spots(cols), basis="knm", slm_shape=SLM, phase=synth.seed_phase(seed, SLM), engine_options=options(on))


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_pair(on, off, what, bodies):
    """phase and weights agree byte for byte; both sides ran the parked next-tile-ahead instance with the flags, `on` with
    zero_inv on every launch, `off` on none."""
    d_on, d_off = dispatch_of(on), dispatch_of(off)
    for d in (d_on, d_off):
        assert d.count("col_tile2_kernel") == bodies, (what, d)
        assert d.count("col_tile2_kernel", flags=["col_flags"], N=4096, NR=5, PARK="true", NXF="true") == bodies, (what, d)
    assert d_on.count("col_tile2_kernel", flags=["zero_inv"]) == bodies, (what, d_on)
    assert d_off.count("col_tile2_kernel", flags=["zero_inv"]) == 0, (what, d_off)
    assert same_bytes(on.phase, off.phase), what
    assert same_bytes(on.weights, off.weights), what


@pytest.mark.parametrize("method", ["WGS-Leonardo", "GS"])
def test_on_and_off_agree_byte_for_byte(method):
    on, off = spot_hologram(True), spot_hologram(False)
    for h in (on, off):
        h.optimize(method, maxiter=3, verbose=False)
    assert_pair(on, off, method, 3)
    xy = spots().astype(int)
    w = on.weights
    assert np.count_nonzero(w) == xy.shape[1] and np.all(w[xy[1], xy[0]] > 0)
    assert np.all(np.isfinite(on.phase)) and np.ptp(on.phase) > 1      # (a phase, not a constant)


def test_batch_of_two_with_different_columns():
    """The register form; flags are per hologram: columns 3 and 128 are flagged in hologram 0 and empty in hologram 1,
    columns 2 and 77 the reverse (2 and 3 share a half tile)."""
    cols = [COLS, (0, 2, 77, 129, 255)]
    targets = np.zeros((2,) + SHAPE, dtype=np.float32)
    for b in range(2):
        xy = spots(cols[b]).astype(int)
        targets[b, xy[1], xy[0]] = 1 + 0.1 * np.arange(xy.shape[1])
    phases = np.stack([synth.seed_phase(60 + b, SLM) for b in range(2)])
    out = []
    for on in (True, False):
        hb = HologramBatch(SHAPE, SLM, targets, phases)
        for opt, val in options(on).items():
            hb.set_option(opt, val)
        hb.optimize("WGS-Leonardo", 3)
        d = dispatch_of(hb)
        assert d.count("col_tile2_kernel") == 3, d
        assert d.count("col_tile2_kernel", flags=["batch", "col_flags"], N=4096, NR=5, PARK="false") == 3, d
        assert d.count("col_tile2_kernel", flags=["batch", "col_flags", "zero_inv"]) == (3 if on else 0), d
        out.append((hb.phases(), hb.engine.get(L.WEIGHTS)))
        hb.close()
    assert same_bytes(out[0][0], out[1][0]) and same_bytes(out[0][1], out[1][1])
    w = out[0][1]
    for b in range(2):
        xy = spots(cols[b]).astype(int)
        assert np.count_nonzero(w[b]) == xy.shape[1] and np.all(w[b][xy[1], xy[0]] > 0), b


def test_weight_written_into_an_empty_column():
    """set_weights puts one finite weight into a column that was empty: the next call scans again, the column is flagged
    and its inverse runs."""
    on, off = spot_hologram(True), spot_hologram(False)
    pair = (on, off)
    for h in pair:
        h.optimize("WGS-Leonardo", maxiter=3, verbose=False)
    assert_pair(on, off, "start", 3)
    col = 64
    for h in pair:
        w = np.array(h.weights, copy=True)
        assert not w[:, col].any() and not h.target[:, col].any()
        w[N - 1, col] = 0.37
        h.set_weights(w)
        h.optimize("WGS-Leonardo", maxiter=2, verbose=False)
    assert_pair(on, off, "weight in an empty column", 2)
    assert on.weights[N - 1, col] != 0            # (the pixel took part)


def test_one_body_against_the_oracle():
    """One teacher-forced WGS-Leonardo body (the third: it updates the weights) with the skip on, against the CPU oracle
    from the same state; bounds of tests/test_gpu_parity.py::test_single_step_matches_reference (phase phasors 5e-6,
    weights 3e-6, relative L2)."""
    phase0 = synth.seed_phase(3, SLM)
    o = orc.OracleSpotHologram(SHAPE, spots(), slm_shape=SLM, phase=phase0.copy())
    o.optimize("WGS-Leonardo", maxiter=2, populate=False)
    p2, w2 = o.phase.copy(), o.weights.copy()
    o.optimize("WGS-Leonardo", maxiter=1, populate=False)
    h = spot_hologram(True)
    h.phase, h.weights, h.iter = p2.copy(), w2.copy(), 2
    h.stats["method"] = ["WGS-Leonardo"] * 2
    h.stats["flags"]["fixed_phase"] = [False] * 2
    h.optimize("WGS-Leonardo", maxiter=1, verbose=False)
    d = dispatch_of(h)
    assert d.count("col_tile2_kernel", flags=["col_flags", "zero_inv"], RULE=1, NXF="true") == 1, d
    ep, ew = phase_rel_l2(h.phase, o.phase), rel_l2(h.weights, o.weights)
    report("empty-column inverse, one body vs oracle", phase=ep, weights=ew)
    assert ep < 5e-6 and ew < 3e-6


def test_dense_image_is_left_alone():
    """A dense random image never receives the flags: the option changes neither the dispatch record nor a byte."""
    out = []
    for on in (True, False):
        h = Hologram(synth.random_target(11, SHAPE, 0.2, 1.0), phase=synth.seed_phase(4, SLM), slm_shape=SLM, engine_options=options(on))
        h.optimize("WGS-Leonardo", maxiter=3, verbose=False)
        d = dispatch_of(h)
        assert d.count("col_tile2_kernel", N=4096, PARK="true", NXF="false") == 3, d
        assert d.count("col_tile2_kernel", flags=["col_flags"]) == 0 and d.count("col_tile2_kernel", flags=["zero_inv"]) == 0, d
        out.append((sorted((r["name"], tuple(sorted(r["flags"])), r["count"]) for r in d.records), h.phase, h.weights))
    assert out[0][0] == out[1][0]
    assert same_bytes(out[0][1], out[1][1]) and same_bytes(out[0][2], out[1][2])
