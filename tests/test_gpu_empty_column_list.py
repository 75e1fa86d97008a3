"""
Weight-norm partials per half tile and the walk over the scan's tile list (``-m gpu``).

The flag-reading instances of ``col_tile2_kernel`` used to leave one weight-norm partial per WORKGROUP, so which workgroup took
which half tile decided the association of ``sum w'^2`` and with it the last bits of ``wscale``.  They now leave one slot per
(hologram, tile, half, wave), which the row launch folds in a fixed order: the results do not depend on the grid
(``HGS_TILE2_BLOCKS``) any more.  On top of that, where H of the empty columns is pre-zeroed (``prezero``), the workgroups walk
the positions of the ascending list of tiles that hold anything (``HGS_OPT_EMPTY_COL_LIST``, default on; dispatch flag
``tile_list``) instead of every tile.  Everything here is compared BYTE FOR BYTE -- grid against grid, list on against list off,
pre-zero on against off -- next to the dispatch record, and once against the CPU oracle.

Geometry of ``test_gpu_empty_column_prezero.py``: pad 4096 x 256, SLM 1152 x 120 (five register slots), the smallest shape at
which the 4096-row instances run: 64 tiles, a natural grid of 128 workgroups (64 pairs).  ``HGS_TILE2_BLOCKS=16`` are eight
pairs: pair i owns list positions i, i + 8, i + 16, ...
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
COLS_B = (1, 34, 64, 98, 99, 200, 229, 253)
ROWS = (N - 1, 13 * T + 17, 7 * T + 3, 100, 40, 2 * T + 40, N // 2, 9, 5 * T + 77, N // 2 + 1, 300)

# The wrapping list: 22 of the 64 tiles hold something, so at eight positions per round (HGS_TILE2_BLOCKS=16) pair i owns
# positions i, i + 8 and i + 16 (pairs 0 - 5) and a workgroup visits up to three half tiles.
TILES_BOTH = (0, 10, 30, 63)                            # both halves (columns 4 t + 1 and 4 t + 2): the first and the last tile
TILES_H0 = (2, 5, 11, 17, 20, 23, 33, 36, 40)           # half 0 only (column 4 t)
TILES_H1 = (3, 8, 14, 26, 44, 47, 50, 55, 58)           # half 1 only (column 4 t + 3)
# listed: 0 2 3 5 8 10 11 14 | 17 20 23 26 30 33 36 40 | 44 47 50 55 58 63 -- 2, 3 and 10, 11 adjacent; 59 - 62 and 27 - 29 runs
# of empty tiles; pair 5 owns tiles 10 (both), 33 (half 0), 63 (both): its half-0 workgroup visits three, its half-1 workgroup
# passes 33; pair 0 owns 0, 17, 44: half 0 visits 0 and 17 and passes 44, half 1 passes 17
COLS_WRAP = tuple(sorted([4 * t + 1 for t in TILES_BOTH] + [4 * t + 2 for t in TILES_BOTH] + [4 * t for t in TILES_H0] +
                         [4 * t + 3 for t in TILES_H1]))
assert len(set(c // 4 for c in COLS_WRAP)) == 22


def spots(cols=COLS):
    """One spot per column, a second one in the first three: (x, y), rows taken from ROWS in turn."""
    xy = [(c, ROWS[i % len(ROWS)]) for i, c in enumerate(cols)]
    xy += [(c, ROWS[(i + 8) % len(ROWS)]) for i, c in enumerate(cols[:3])]
    assert len(set(xy)) == len(xy)
    return np.array(xy, dtype=float).T


def options(listed=True, prezero=True, empty=True):
    e = 1 if empty else 0
    return {L.OPT_SPARSE_COLUMNS: 0, L.OPT_EMPTY_COL_LOADS: e, L.OPT_EMPTY_COL_INVERSE: e, L.OPT_EMPTY_COL_FORWARD: e,
            L.OPT_EMPTY_COL_PREZERO: 1 if (prezero and empty) else 0, L.OPT_EMPTY_COL_LIST: 1 if listed else 0}


def spot_hologram(opts, seed=3, cols=COLS, shape=SHAPE, slm=SLM):
    return SpotHologram(shape, spots(cols), basis="knm", slm_shape=slm, phase=synth.seed_phase(seed, slm), engine_options=opts)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def set_grid(monkeypatch, blocks):
    if blocks is None:
        monkeypatch.delenv("HGS_TILE2_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("HGS_TILE2_BLOCKS", str(blocks))


def assert_flags(d, bodies, listed, prezero, what, **inst):
    """One call of `bodies` plain bodies: with pre-zero on all column launches but the first carry `prezero`, and with the list
    on exactly those carry `tile_list`; never one without the other."""
    inst = dict(dict(N=4096, NR=5, PARK="true", NXF="true"), **inst)
    assert d.count("col_tile2_kernel", **inst) == bodies, (what, d.records)
    assert d.count("col_tile2_kernel") == bodies, (what, d.records)
    assert d.count("col_tile2_kernel", flags=["prezero"]) == (bodies - 1 if prezero else 0), (what, d.records)
    assert d.count("col_tile2_kernel", flags=["prezero", "tile_list"]) == (bodies - 1 if prezero and listed else 0), (what, d.records)
    assert d.count("col_tile2_kernel", flags=["tile_list"], without=["prezero"]) == 0, (what, d.records)


def run(monkeypatch, blocks, opts, cols=COLS, bodies=4, method="WGS-Leonardo", **kw):
    set_grid(monkeypatch, blocks)
    h = spot_hologram(opts, cols=cols, **kw)
    h.optimize(method, maxiter=bodies, verbose=False)
    return h, dispatch_of(h)


def test_results_depend_neither_on_the_grid_nor_on_the_options(monkeypatch):
    """WGS-Leonardo, four bodies, at 16 / 32 / 128 (natural) workgroups, each with the defaults, with the list off and with
    every empty-column option off: phase and weights of all nine runs byte-identical (one sweep, every run compared with the
    first: the session's time budget is shared with every other GPU test)."""
    out = []
    for blocks in (16, 32, None):
        for opts in (options(), options(listed=False), options(empty=False)):
            h, d = run(monkeypatch, blocks, opts)
            assert_flags(d, 4, bool(opts[L.OPT_EMPTY_COL_LIST]), bool(opts[L.OPT_EMPTY_COL_PREZERO]), (blocks, opts))
            out.append((h.phase, h.weights))
    for k, o in enumerate(out[1:]):
        assert same_bytes(out[0][0], o[0]) and same_bytes(out[0][1], o[1]), k + 1
    xy = spots().astype(int)
    w = out[0][1]
    assert np.count_nonzero(w) == xy.shape[1] and np.all(w[xy[1], xy[0]] > 0)
    assert np.all(np.isfinite(out[0][0])) and np.ptp(out[0][0]) > 1


@pytest.fixture(scope="module")
def wrap_oracle():
    phase0 = synth.seed_phase(3, SLM)
    o = orc.OracleSpotHologram(SHAPE, spots(COLS_WRAP), slm_shape=SLM, phase=phase0.copy())
    o.optimize("WGS-Leonardo", maxiter=4, populate=False)
    return o.phase.copy(), o.weights.copy()


def test_wrapping_list(monkeypatch, wrap_oracle):
    """22 listed tiles on eight pairs: workgroups take up to three list positions and pass the ones whose half is empty.  Bytes
    equal to list off and to pre-zero off, the flag on bodies - 1 launches, and four bodies against the CPU oracle with the metric
    and bounds test_gpu_empty_column_prezero.py uses at this geometry (phase phasors 5e-6, weights 3e-6, relative L2)."""
    on, d = run(monkeypatch, 16, options(), cols=COLS_WRAP)
    assert_flags(d, 4, True, True, "wrap")
    off, d = run(monkeypatch, 16, options(listed=False), cols=COLS_WRAP)
    assert_flags(d, 4, False, True, "wrap, list off")
    plain, d = run(monkeypatch, 16, options(prezero=False), cols=COLS_WRAP)
    assert_flags(d, 4, True, False, "wrap, prezero off")
    for h in (off, plain):
        assert same_bytes(on.phase, h.phase) and same_bytes(on.weights, h.weights)
    xy = spots(COLS_WRAP).astype(int)
    assert np.count_nonzero(on.weights) == xy.shape[1] and np.all(on.weights[xy[1], xy[0]] > 0)
    ep, ew = phase_rel_l2(on.phase, wrap_oracle[0]), rel_l2(on.weights, wrap_oracle[1])
    report("empty-column tile list, wrapping, four bodies vs oracle", phase=ep, weights=ew)
    print(f"wrapping list, four bodies vs oracle: phase {ep:.3e} weights {ew:.3e}")
    assert ep < 5e-6 and ew < 3e-6


@pytest.mark.parametrize("blocks", [32, None], ids=["walk", "natural"])
def test_batch_of_two_with_different_columns(blocks, monkeypatch):
    """The register form: lists, lengths and slots are per hologram.  HGS_TILE2_BLOCKS counts the workgroups of the whole batch:
    32 are 16 per hologram, on which the 22 tiles of the first hologram wrap."""
    set_grid(monkeypatch, blocks)
    cols = [COLS_WRAP, COLS_B]
    targets = np.zeros((2,) + SHAPE, dtype=np.float32)
    for b in range(2):
        xy = spots(cols[b]).astype(int)
        targets[b, xy[1], xy[0]] = 1 + 0.1 * np.arange(xy.shape[1])
    phases = np.stack([synth.seed_phase(60 + b, SLM) for b in range(2)])
    out = []
    for listed in (True, False):
        hb = HologramBatch(SHAPE, SLM, targets, phases)
        for opt, val in options(listed=listed).items():
            hb.set_option(opt, val)
        hb.optimize("WGS-Leonardo", 4)
        d = dispatch_of(hb)
        assert_flags(d, 4, listed, True, "batch", PARK="false", NXF="false")
        assert d.count("col_tile2_kernel", flags=["batch", "col_flags", "zero_fwd"]) == 4, d.records
        out.append((hb.phases(), hb.engine.get(L.WEIGHTS)))
        hb.close()
    for b in range(2):
        assert same_bytes(out[0][0][b], out[1][0][b]) and same_bytes(out[0][1][b], out[1][1][b]), b
        xy = spots(cols[b]).astype(int)
        w = out[0][1][b]
        assert np.count_nonzero(w) == xy.shape[1] and np.all(w[xy[1], xy[0]] > 0), b


def test_new_target_between_two_calls(monkeypatch):
    """Other spot columns uploaded between two calls: list and slots are renewed with the scan, the first body on the new target
    carries neither `prezero` nor `tile_list`, and the bytes are those of the list off."""
    set_grid(monkeypatch, 16)

    def image(cols):
        xy = spots(cols).astype(int)
        target = np.zeros(SHAPE, dtype=np.float32)
        target[xy[1], xy[0]] = 1 + 0.1 * np.arange(xy.shape[1])
        return target

    out = []
    for listed in (True, False):
        h = Hologram(image(COLS_WRAP), phase=synth.seed_phase(3, SLM), slm_shape=SLM, engine_options=options(listed=listed))
        h.optimize("WGS-Leonardo", maxiter=3, verbose=False)
        assert_flags(dispatch_of(h), 3, listed, True, "old target")
        h.set_target(image(COLS_B), reset_weights=True)
        h.optimize("WGS-Leonardo", maxiter=3, verbose=False)
        assert_flags(dispatch_of(h), 3, listed, True, "new target")
        out.append((h.phase, h.weights))
        assert np.count_nonzero(h.weights[:, list(COLS_B)]) > 0
        assert np.count_nonzero(h.weights) == np.count_nonzero(image(COLS_B))
    assert same_bytes(out[0][0], out[1][0]) and same_bytes(out[0][1], out[1][1])


def test_square_pad_prefetching_row_and_parked_column_instances(monkeypatch):
    """4096 x 4096, SLM 1152 x 1920, eight spot columns, three bodies: the headline's pair of instances -- the fold of 8192 slots
    in the row-less block of the prefetching row kernel, eight listed tiles on 384 pairs."""
    set_grid(monkeypatch, None)
    shape, slm = (N, N), (1152, 1920)
    cols = (32, 65, 96, 97, 1000, 2050, 3001, 4095)
    out = []
    for listed in (True, False):
        h = spot_hologram(options(listed=listed), seed=5, cols=cols, shape=shape, slm=slm)
        h.optimize("WGS-Leonardo", maxiter=3, verbose=False)
        d = dispatch_of(h)
        assert_flags(d, 3, listed, True, "4096 x 4096")
        assert d.count("row_kernel", flags=["zero_mask"], N=4096, MODE=2, NS=8, PREF="true") == 2, d.records
        out.append((h.phase, h.weights))
    assert same_bytes(out[0][0], out[1][0]) and same_bytes(out[0][1], out[1][1])
    xy = spots(cols).astype(int)
    w = out[0][1]
    assert np.count_nonzero(w) == xy.shape[1] and np.all(w[xy[1], xy[0]] > 0)
