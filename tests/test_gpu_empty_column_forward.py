"""
Empty columns of the half-width tile kernel are not transformed forward (``-m gpu``).  In the plain instances of
``col_tile2_kernel`` the farfield of a column is read by that column's weight rule only; where the inverse skip
(``HGS_OPT_EMPTY_COL_INVERSE``) drops the rule and the inverse of a column the scan found empty, ``HGS_OPT_EMPTY_COL_FORWARD``
(default on) also drops its forward transform, and a half tile of two empty columns requests no G rows, touches no LDS, passes
no barrier and only stores its zeros into H.  With the option off the kernel behaves as before, so everything here is compared
BYTE FOR BYTE between the two, next to the dispatch record (``zero_fwd`` says that the launch skips).

A skipped half tile that wrote nothing, or that left G in H, changes the phase after the row pass: the byte comparison of the
phase is the check that the zeros are written.

Geometry of ``test_gpu_empty_column_inverse.py``: pad 4096 x 256, SLM 1152 x 120 (five register slots); sparse columns off,
empty-column loads and inverse on.  At this pad the natural grid is 128 workgroups of ONE half tile each: the walk from half
tile to half tile (the flag word of the next one, the rows requested ahead, the weight / target request chain) never runs.
``HGS_TILE2_BLOCKS=16`` (read per engine when it is created) makes the grid 16 workgroups; workgroup (xcd x, half h) then walks
tiles x, x + 8, ..., x + 56 -- eight half tiles, columns 4 (x + 8 k) + 2 h + {0, 1}.  The spot columns give single workgroups
every transition:

    workgroup (0, 0)  k = 0 empty (the FIRST half tile), k = 1 column 32 (column 0 only), k = 2 column 65 (column 1 only),
                      k = 3 columns 96 and 97, k = 4, 5 empty (two in a row), k = 6 column 192, k = 7 empty (the LAST one)
    workgroup (1, 1)  k = 0 column 6 (first half tile full), k = 7 column 231 (last half tile full)
    workgroup (7, 1)  k = 7 column 255 (the last byte of the last flag word)
    every other workgroup: eight empty half tiles
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
COLS = (32, 65, 96, 97, 192, 6, 231, 255)
# rows of the existing empty-column tests: the last row of the pad, a pixel alone in the last quarter of lane 17, ...
ROWS = (N - 1, 13 * T + 17, 7 * T + 3, 100, 40, 2 * T + 40, N // 2, 9, 5 * T + 77, N // 2 + 1, 300)


def spots(cols=COLS):
    """One spot per column, a second one in the first three: (x, y), rows taken from ROWS in turn."""
    xy = [(c, ROWS[i % len(ROWS)]) for i, c in enumerate(cols)]
    xy += [(c, ROWS[(i + 8) % len(ROWS)]) for i, c in enumerate(cols[:3])]
    assert len(set(xy)) == len(xy)
    return np.array(xy, dtype=float).T


def options(fwd, inv=True):
    return {L.OPT_SPARSE_COLUMNS: 0, L.OPT_EMPTY_COL_LOADS: 1, L.OPT_EMPTY_COL_INVERSE: 1 if inv else 0,
            L.OPT_EMPTY_COL_FORWARD: 1 if fwd else 0}


def spot_hologram(fwd, seed=3, cols=COLS, inv=True):
    return SpotHologram(SHAPE, spots(cols), basis="knm", slm_shape=SLM, phase=synth.seed_phase(seed, SLM), engine_options=options(fwd, inv))


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(params=[16, None], ids=["walk", "natural"])
def grid(request, monkeypatch):
    """HGS_TILE2_BLOCKS per hologram: 16 (eight half tiles per workgroup) or the natural grid (one each)."""
    if request.param is None:
        monkeypatch.delenv("HGS_TILE2_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("HGS_TILE2_BLOCKS", str(request.param))
    return request.param


@pytest.fixture
def walk(monkeypatch):
    monkeypatch.setenv("HGS_TILE2_BLOCKS", "16")


def assert_pair(on, off, what, bodies):
    """phase and weights agree byte for byte; both sides ran the parked next-tile-ahead instance with the flags and the inverse
    skip, `on` with zero_fwd on every launch, `off` on none."""
    d_on, d_off = dispatch_of(on), dispatch_of(off)
    for d in (d_on, d_off):
        assert d.count("col_tile2_kernel") == bodies, (what, d)
        assert d.count("col_tile2_kernel", flags=["col_flags", "zero_inv"], N=4096, NR=5, PARK="true", NXF="true") == bodies, (what, d)
    assert d_on.count("col_tile2_kernel", flags=["zero_fwd"]) == bodies, (what, d_on)
    assert d_off.count("col_tile2_kernel", flags=["zero_fwd"]) == 0, (what, d_off)
    assert same_bytes(on.phase, off.phase), what
    assert same_bytes(on.weights, off.weights), what


@pytest.mark.parametrize("method", ["WGS-Leonardo", "GS"])
def test_on_and_off_agree_byte_for_byte(method, grid):
    on, off = spot_hologram(True), spot_hologram(False)
    for h in (on, off):
        h.optimize(method, maxiter=3, verbose=False)
    assert_pair(on, off, method, 3)
    xy = spots().astype(int)
    w = on.weights
    assert np.count_nonzero(w) == xy.shape[1] and np.all(w[xy[1], xy[0]] > 0)
    assert np.all(np.isfinite(on.phase)) and np.ptp(on.phase) > 1      # (a phase, not a constant)


@pytest.mark.parametrize("blocks", [32, None], ids=["walk", "natural"])
def test_batch_of_two_with_different_columns(blocks, monkeypatch):
    """The register form; flags are per hologram.  Hologram 1 holds other columns than hologram 0 (98 and 99 share a half tile
    as 96 and 97 do in hologram 0; its workgroup (0, 0) starts with a full half tile).  HGS_TILE2_BLOCKS counts the workgroups
    of the whole batch: 32 are 16 per hologram."""
    if blocks is None:
        monkeypatch.delenv("HGS_TILE2_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("HGS_TILE2_BLOCKS", str(blocks))
    cols = [COLS, (1, 34, 64, 98, 99, 200, 229, 253)]
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
        assert d.count("col_tile2_kernel", flags=["batch", "col_flags", "zero_inv"], N=4096, NR=5, PARK="false") == 3, d
        assert d.count("col_tile2_kernel", flags=["zero_fwd"]) == (3 if on else 0), d
        out.append((hb.phases(), hb.engine.get(L.WEIGHTS)))
        hb.close()
    assert same_bytes(out[0][0], out[1][0]) and same_bytes(out[0][1], out[1][1])
    w = out[0][1]
    for b in range(2):
        xy = spots(cols[b]).astype(int)
        assert np.count_nonzero(w[b]) == xy.shape[1] and np.all(w[b][xy[1], xy[0]] > 0), b


def test_weight_written_into_an_empty_half_tile(walk):
    """set_weights puts one finite weight into column 130, whose half tile (130, 131) was skipped whole: the next call scans
    again, the column is flagged, and it is loaded, transformed and updated."""
    on, off = spot_hologram(True), spot_hologram(False)
    pair = (on, off)
    for h in pair:
        h.optimize("WGS-Leonardo", maxiter=3, verbose=False)
    assert_pair(on, off, "start", 3)
    col = 130
    for h in pair:
        w = np.array(h.weights, copy=True)
        assert not w[:, col:col + 2].any() and not h.target[:, col:col + 2].any()
        w[N - 1, col] = 0.37
        h.set_weights(w)
        h.optimize("WGS-Leonardo", maxiter=2, verbose=False)
    assert_pair(on, off, "weight in an empty half tile", 2)
    w = on.weights[N - 1, col]
    print("weight set to 0.37 is now", repr(w))
    assert w != 0 and w != np.float32(0.37)            # (the pixel took part: the rule and the norm changed it)


def test_one_body_against_the_oracle(walk):
    """One teacher-forced WGS-Leonardo body (the third: it updates the weights) with the skip on and the walk override,
    against the CPU oracle from the same state; bounds of tests/test_gpu_parity.py::test_single_step_matches_reference (phase
    phasors 5e-6, weights 3e-6, relative L2)."""
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
    assert d.count("col_tile2_kernel", flags=["col_flags", "zero_inv", "zero_fwd"], RULE=1, NXF="true") == 1, d
    ep, ew = phase_rel_l2(h.phase, o.phase), rel_l2(h.weights, o.weights)
    report("empty-column forward, one body vs oracle", phase=ep, weights=ew)
    print(f"one body vs oracle: phase {ep:.3e} weights {ew:.3e}")
    assert ep < 5e-6 and ew < 3e-6


def _records(d):
    return sorted((r["name"], tuple(sorted(r["flags"])), r["count"]) for r in d.records)


def test_inverse_off_takes_the_forward_skip_with_it(walk):
    """The forward skip rests on the inverse skip: with HGS_OPT_EMPTY_COL_INVERSE = 0 no launch carries zero_fwd and the option
    changes neither the dispatch record nor a byte."""
    out = []
    for fwd in (True, False):
        h = spot_hologram(fwd, inv=False)
        h.optimize("WGS-Leonardo", maxiter=3, verbose=False)
        d = dispatch_of(h)
        assert d.count("col_tile2_kernel", flags=["col_flags"], NXF="true") == 3, d
        assert d.count("col_tile2_kernel", flags=["zero_inv"]) == 0 and d.count("col_tile2_kernel", flags=["zero_fwd"]) == 0, d
        out.append((_records(d), h.phase, h.weights))
    assert out[0][0] == out[1][0]
    assert same_bytes(out[0][1], out[1][1]) and same_bytes(out[0][2], out[1][2])


def test_dense_image_is_left_alone():
    """A dense random image never receives the flags: the option changes neither the dispatch record nor a byte."""
    out = []
    for fwd in (True, False):
        h = Hologram(synth.random_target(11, SHAPE, 0.2, 1.0), phase=synth.seed_phase(4, SLM), slm_shape=SLM, engine_options=options(fwd))
        h.optimize("WGS-Leonardo", maxiter=3, verbose=False)
        d = dispatch_of(h)
        assert d.count("col_tile2_kernel", N=4096, PARK="true", NXF="false") == 3, d
        assert d.count("col_tile2_kernel", flags=["col_flags"]) == 0 and d.count("col_tile2_kernel", flags=["zero_fwd"]) == 0, d
        out.append((_records(d), h.phase, h.weights))
    assert out[0][0] == out[1][0]
    assert same_bytes(out[0][1], out[1][1]) and same_bytes(out[0][2], out[1][2])


def test_kim_fixed_phase_launches_are_left_alone(walk):
    """WGS-Kim with its phase fixed runs the phase-READING instance (PHASE 2), which keeps its code: those launches carry no
    zero_fwd, and the option changes no byte of the loop."""
    out = []
    for fwd in (True, False):
        h = spot_hologram(fwd)
        h.optimize("WGS-Kim", maxiter=5, verbose=False, fix_phase_iteration=2)
        d = dispatch_of(h)
        assert d.count("col_tile2_kernel", PHASE=2) >= 2, d
        assert d.count("col_tile2_kernel", flags=["zero_fwd"], PHASE=2) == 0 and d.count("col_tile2_kernel", flags=["zero_inv"], PHASE=2) == 0, d
        out.append((h.phase, h.weights))
    assert same_bytes(out[0][0], out[1][0]) and same_bytes(out[0][1], out[1][1])
