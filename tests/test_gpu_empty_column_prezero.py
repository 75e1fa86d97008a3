"""
H of the empty columns written by the row launch, empty half tiles walked past by the column launch (``-m gpu``).  Where
``HGS_OPT_EMPTY_COL_FORWARD`` acts, an empty half tile of ``col_tile2_kernel`` did nothing but store zeros into H.  With
``HGS_OPT_EMPTY_COL_PREZERO`` (default on) the row launch that closes the body BEFORE stores those zeros instead of G in the
columns the scan found empty (dispatch flag ``zero_mask``), and the column launch visits only the half tiles that are not empty
(``prezero``).  Inside one engine call only: the first column launch of a call runs the plain form, the last row launch of a
call leaves G of every column.  With the option off every launch is the one it was, so everything here is compared BYTE FOR
BYTE between the two, next to the dispatch record.

A half tile that was walked past although nothing had zeroed it leaves G in H, and a zero-masked column that is read as G
loses a spot column: either changes the phase after the next row pass, so the byte comparison of phase and weights is the check.

Geometry, spot columns and grids of ``test_gpu_empty_column_forward.py``: pad 4096 x 256, SLM 1152 x 120 (five register
slots), the smallest shape at which the 4096-row instances run; ``HGS_TILE2_BLOCKS=16`` makes workgroup (xcd x, half h) walk
tiles x, x + 8, ..., x + 56 -- eight half tiles, columns 4 (x + 8 k) + 2 h + {0, 1}:

    workgroup (0, 0)  k = 0 empty (the FIRST half tile), k = 1 column 32 (column 0 only), k = 2 column 65 (column 1 only),
                      k = 3 columns 96 and 97, k = 4, 5 empty (two in a row), k = 6 column 192, k = 7 empty (the LAST one)
    workgroup (1, 1)  k = 0 column 6 (first half tile full), k = 7 column 231 (last half tile full)
    workgroup (7, 1)  k = 7 column 255 (the last byte of the last flag word)
    every other workgroup: eight empty half tiles (it runs its loop zero times and still writes its weight-norm partial)
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
COLS_B = (1, 34, 64, 98, 99, 200, 229, 253)       # the second column set of the batch test of test_gpu_empty_column_forward.py
ROWS = (N - 1, 13 * T + 17, 7 * T + 3, 100, 40, 2 * T + 40, N // 2, 9, 5 * T + 77, N // 2 + 1, 300)


def spots(cols=COLS):
    """One spot per column, a second one in the first three: (x, y), rows taken from ROWS in turn."""
    xy = [(c, ROWS[i % len(ROWS)]) for i, c in enumerate(cols)]
    xy += [(c, ROWS[(i + 8) % len(ROWS)]) for i, c in enumerate(cols[:3])]
    assert len(set(xy)) == len(xy)
    return np.array(xy, dtype=float).T


def options(prezero):
    return {L.OPT_SPARSE_COLUMNS: 0, L.OPT_EMPTY_COL_LOADS: 1, L.OPT_EMPTY_COL_INVERSE: 1, L.OPT_EMPTY_COL_FORWARD: 1,
            L.OPT_EMPTY_COL_PREZERO: 1 if prezero else 0}


def spot_hologram(prezero, seed=3, cols=COLS, shape=SHAPE, slm=SLM):
    return SpotHologram(shape, spots(cols), basis="knm", slm_shape=slm, phase=synth.seed_phase(seed, slm), engine_options=options(prezero))


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


def assert_call(d, bodies, prezero, what, **inst):
    """One engine call of `bodies` plain bodies: every column launch is the flag-reading instance with zero_fwd; with the option
    on all but the first carry `prezero` and all MODE 2 row launches `zero_mask`, the closing one (MODE 3) never."""
    inst = dict(dict(N=4096, NR=5, PARK="true", NXF="true"), **inst)
    assert d.count("col_tile2_kernel") == bodies, (what, d.records)
    assert d.count("col_tile2_kernel", flags=["col_flags", "zero_inv", "zero_fwd"], **inst) == bodies, (what, d.records)
    assert d.count("col_tile2_kernel", flags=["prezero"]) == (bodies - 1 if prezero else 0), (what, d.records)
    assert d.count("row_kernel", MODE=2) == bodies - 1, (what, d.records)
    assert d.count("row_kernel", flags=["zero_mask"], MODE=2) == (bodies - 1 if prezero else 0), (what, d.records)
    assert d.count("row_kernel", flags=["zero_mask"]) == (bodies - 1 if prezero else 0), (what, d.records)
    assert d.count("row_kernel", MODE=3, without=["zero_mask"]) == 1, (what, d.records)


@pytest.mark.parametrize("method", ["WGS-Leonardo", "GS"])
def test_on_and_off_agree_byte_for_byte(method, grid):
    on, off = spot_hologram(True), spot_hologram(False)
    for h in (on, off):
        h.optimize(method, maxiter=4, verbose=False)
    assert_call(dispatch_of(on), 4, True, method)
    assert_call(dispatch_of(off), 4, False, method)
    assert same_bytes(on.phase, off.phase), method
    assert same_bytes(on.weights, off.weights), method
    xy = spots().astype(int)
    w = on.weights
    assert np.count_nonzero(w) == xy.shape[1] and np.all(w[xy[1], xy[0]] > 0)
    assert np.all(np.isfinite(on.phase)) and np.ptp(on.phase) > 1      # (a phase, not a constant)


def test_two_calls_walk_like_one(walk):
    """The closing launch of a call leaves G of every column and the next call starts in the plain form: 3 + 3 bodies are the
    bytes of 6, with the option on and off."""
    out = {}
    for prezero in (True, False):
        two, one = spot_hologram(prezero), spot_hologram(prezero)
        two.optimize("WGS-Leonardo", maxiter=3, verbose=False)
        assert_call(dispatch_of(two), 3, prezero, "first call")
        two.optimize("WGS-Leonardo", maxiter=3, verbose=False)
        d = dispatch_of(two)
        assert_call(d, 3, prezero, "second call")
        one.optimize("WGS-Leonardo", maxiter=6, verbose=False)
        assert_call(dispatch_of(one), 6, prezero, "one call")
        assert same_bytes(two.phase, one.phase) and same_bytes(two.weights, one.weights), prezero
        out[prezero] = (two.phase, two.weights)
    assert same_bytes(out[True][0], out[False][0]) and same_bytes(out[True][1], out[False][1])


def test_new_target_between_two_calls(walk):
    """Other spot columns uploaded between two calls: the scan runs again, the first body on the new target carries no
    `prezero` (and no row launch of the first call zero-masked on its behalf), and the bytes are those of the option off."""
    def image(cols):
        xy = spots(cols).astype(int)
        target = np.zeros(SHAPE, dtype=np.float32)
        target[xy[1], xy[0]] = 1 + 0.1 * np.arange(xy.shape[1])
        return target

    out = []
    for prezero in (True, False):
        h = Hologram(image(COLS), phase=synth.seed_phase(3, SLM), slm_shape=SLM, engine_options=options(prezero))
        h.optimize("WGS-Leonardo", maxiter=3, verbose=False)
        assert_call(dispatch_of(h), 3, prezero, "old target")
        h.set_target(image(COLS_B), reset_weights=True)
        h.optimize("WGS-Leonardo", maxiter=3, verbose=False)
        d = dispatch_of(h)
        assert d.count("col_tile2_kernel", flags=["col_flags", "zero_fwd"]) == 3, d.records
        assert d.count("col_tile2_kernel", flags=["prezero"]) == (2 if prezero else 0), d.records
        assert d.count("col_tile2_kernel", flags=["zero_fwd"], without=["prezero"]) == (1 if prezero else 3), d.records
        assert d.count("row_kernel", flags=["zero_mask"]) == (2 if prezero else 0), d.records
        out.append((h.phase, h.weights))
        assert np.count_nonzero(h.weights[:, list(COLS_B)]) > 0
    assert same_bytes(out[0][0], out[1][0]) and same_bytes(out[0][1], out[1][1])


@pytest.mark.parametrize("blocks", [32, None], ids=["walk", "natural"])
def test_batch_of_two_with_different_columns(blocks, monkeypatch):
    """The register form of the column kernel and the 16-byte stores of the one-row row kernel; flags and masks are per
    hologram.  HGS_TILE2_BLOCKS counts the workgroups of the whole batch: 32 are 16 per hologram."""
    if blocks is None:
        monkeypatch.delenv("HGS_TILE2_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("HGS_TILE2_BLOCKS", str(blocks))
    cols = [COLS, COLS_B]
    targets = np.zeros((2,) + SHAPE, dtype=np.float32)
    for b in range(2):
        xy = spots(cols[b]).astype(int)
        targets[b, xy[1], xy[0]] = 1 + 0.1 * np.arange(xy.shape[1])
    phases = np.stack([synth.seed_phase(60 + b, SLM) for b in range(2)])
    out = []
    for prezero in (True, False):
        hb = HologramBatch(SHAPE, SLM, targets, phases)
        for opt, val in options(prezero).items():
            hb.set_option(opt, val)
        hb.optimize("WGS-Leonardo", 4)
        d = dispatch_of(hb)
        assert d.count("col_tile2_kernel") == 4, d.records
        assert d.count("col_tile2_kernel", flags=["batch", "col_flags", "zero_inv", "zero_fwd"], N=4096, NR=5, PARK="false") == 4, d.records
        assert d.count("col_tile2_kernel", flags=["prezero"]) == (3 if prezero else 0), d.records
        assert d.count("row_kernel", flags=["batch", "zero_mask"], MODE=2, PREF="false") == (3 if prezero else 0), d.records
        assert d.count("row_kernel", flags=["zero_mask"]) == (3 if prezero else 0), d.records
        out.append((hb.phases(), hb.engine.get(L.WEIGHTS)))
        hb.close()
    for b in range(2):
        assert same_bytes(out[0][0][b], out[1][0][b]) and same_bytes(out[0][1][b], out[1][1][b]), b
        xy = spots(cols[b]).astype(int)
        w = out[0][1][b]
        assert np.count_nonzero(w) == xy.shape[1] and np.all(w[xy[1], xy[0]] > 0), b


def test_kim_bodies_outside_the_plain_instance_are_left_alone(walk):
    """WGS-Kim: the bodies that store the farfield phase run col_tile_kernel, those with the phase fixed the PHASE 2 instance of
    col_tile2_kernel.  Neither reads the flags, so neither carries `prezero`, and no row launch zero-masks ahead of them: every
    zero-masked row launch is followed by a column launch that counts on it."""
    out = []
    for prezero in (True, False):
        h = spot_hologram(prezero)
        h.optimize("WGS-Kim", maxiter=6, verbose=False, fix_phase_iteration=2)
        d = dispatch_of(h)
        assert d.count("col_tile2_kernel", PHASE=2) >= 2, d.records
        assert d.count("col_tile2_kernel", flags=["prezero"], PHASE=2) == 0 and d.count("col_tile_kernel", flags=["prezero"]) == 0, d.records
        n_pre = d.count("col_tile2_kernel", flags=["prezero"], PHASE=0)
        assert d.count("row_kernel", flags=["zero_mask"]) == n_pre, d.records
        if not prezero:
            assert n_pre == 0, d.records
        out.append((h.phase, h.weights))
    assert same_bytes(out[0][0], out[1][0]) and same_bytes(out[0][1], out[1][1])


def test_square_pad_prefetching_row_and_parked_column_instances():
    """4096 x 4096, SLM 1152 x 1920, eight spot columns: the only shape at which the prefetching row instance (8-byte stores,
    several rows per workgroup) and the parked next-tile-ahead column instance run together -- the headline's pair."""
    shape, slm = (N, N), (1152, 1920)
    cols = (32, 65, 96, 97, 1000, 2050, 3001, 4095)
    out = []
    for prezero in (True, False):
        h = spot_hologram(prezero, seed=5, cols=cols, shape=shape, slm=slm)
        h.optimize("WGS-Leonardo", maxiter=3, verbose=False)
        d = dispatch_of(h)
        assert_call(d, 3, prezero, "4096 x 4096")
        assert d.count("row_kernel", N=4096, MODE=2, NS=8, PREF="true") == 2, d.records
        assert d.count("row_kernel", flags=["zero_mask"], N=4096, MODE=2, NS=8, PREF="true") == (2 if prezero else 0), d.records
        out.append((h.phase, h.weights))
    assert same_bytes(out[0][0], out[1][0]) and same_bytes(out[0][1], out[1][1])
    xy = spots(cols).astype(int)
    w = out[0][1]
    assert np.count_nonzero(w) == xy.shape[1] and np.all(w[xy[1], xy[0]] > 0)


def test_four_bodies_against_the_oracle(walk):
    """The WGS-Leonardo case of test_on_and_off_agree_byte_for_byte (four bodies in one call, three of them on pre-zeroed H)
    against the CPU oracle from the same seed, with the metric and the bounds test_gpu_empty_column_forward.py applies to this
    geometry (phase phasors 5e-6, weights 3e-6, relative L2)."""
    phase0 = synth.seed_phase(3, SLM)
    o = orc.OracleSpotHologram(SHAPE, spots(), slm_shape=SLM, phase=phase0.copy())
    o.optimize("WGS-Leonardo", maxiter=4, populate=False)
    h = spot_hologram(True)
    h.optimize("WGS-Leonardo", maxiter=4, verbose=False)
    assert_call(dispatch_of(h), 4, True, "oracle")
    ep, ew = phase_rel_l2(h.phase, o.phase), rel_l2(h.weights, o.weights)
    report("empty-column prezero, four bodies vs oracle", phase=ep, weights=ew)
    print(f"four bodies vs oracle: phase {ep:.3e} weights {ew:.3e}")
    assert ep < 5e-6 and ew < 3e-6
