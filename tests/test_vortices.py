"""
remove_vortices(): farfield phase-vortex removal on the engine (include/hgs.h, hgs_remove_vortices) against fixtures recorded
from the reference's ``analysis.image_vortices`` / ``image_vortices_coordinates`` / ``image_remove_vortices`` on the CPU
(tools/make_golden.py, case set ``vortex``).

* Lists are compared EXACTLY (as sorted sets): the recorder refuses a case whose float32 and float64 reference runs find
  different vortices, so no wrap-boundary tie hides behind a tolerance.
* float64 cleaned phase: relative L2 against the fixture <= max(1e-9, 3 * d64), d64 = the distance of the NumPy restatement
  below from the same fixture (the reference subtracts vortex by vortex, the engine and the restatement's check sum first).
* float32: what the engine subtracted against what the float64 reference subtracted, relative to the latter, within
  3 * d32, d32 = the same distance for the reference's OWN float32 run (fixture ``cleaned_f32``).  The margin of 3: the
  summation order and the atan2 differ, not the order of magnitude.
* Case E: a float64 WGS-Kim run whose callback cleans the fixed phase once, on the fused and on the general loop, final
  ``phase`` and ``phase_ff`` within the 1e-9 (unit phasors) a float64 WGS-Kim run is held to in tests/test_gpu_parity.py.
  The recorder keeps that bound meaningful: it refuses the case unless the reference's own result moves by less than
  1e-10 under one ulp of the seed phase.

Measured on the MI355X: the table in DESIGN.md 6.7; printed with -s.
"""
import functools

import numpy as np
import pytest

from conftest import dispatch_of, force_stepwise, load_golden, phase_rel_l2, rel_l2
from slmsuite_amd import _lib as L
from slmsuite_amd.hardware import SimpleFourierSLM, SimpleSLM
from slmsuite_amd.holography.algorithms import CompressedSpotHologram, Hologram, MultiplaneHologram, SpotHologram

CASES = ("A", "B", "C", "D")


# ---- NumPy restatement of the three analysis functions (analysis/__init__.py:1207-1309) ----------------------------------
def np_winding(phase):
    dd = [np.mod(np.diff(phase, axis=a, prepend=np.nan) - np.pi, 2 * np.pi) for a in range(2)]
    with np.errstate(invalid="ignore"):
        w = -(dd[0] - dd[1] - np.roll(dd[0], 1, axis=1) + np.roll(dd[1], 1, axis=0)) / (2 * np.pi)
    w[np.isnan(w)] = 0
    return np.rint(w)


def np_eroded(mask):
    """binary_erosion(mask, ones((5, 5))) with a zero border: the whole 5 x 5 neighbourhood inside the grid and set."""
    h, w = mask.shape
    padded = np.zeros((h + 4, w + 4), dtype=bool)
    padded[2:-2, 2:-2] = mask
    out = np.ones((h, w), dtype=bool)
    for dy in range(5):
        for dx in range(5):
            out &= padded[dy:dy + h, dx:dx + w]
    return out


def np_vortices(phase, target):
    w = np_winding(phase)
    with np.errstate(invalid="ignore"):
        w[~np_eroded(target > 0)] = 0
    rows, cols = np.nonzero(w)
    return rows, cols, w[rows, cols]


def np_remove(phase, target):
    """Returns (cleaned phase, rows, cols, weights); the vortices are summed in chunks before they are subtracted."""
    rows, cols, wts = np_vortices(phase, target)
    h, w = phase.shape
    X, Y = np.meshgrid(np.arange(w, dtype=float), np.arange(h, dtype=float))
    total = np.zeros((h, w))
    for k0 in range(0, len(rows), 256):
        sl = slice(k0, k0 + 256)
        total += np.sum(wts[sl, None, None] * np.arctan2(X[None] - cols[sl, None, None], Y[None] - rows[sl, None, None]), axis=0)
    return phase - total, rows, cols, wts


def as_set(rows, cols, wts):
    return sorted(zip(np.asarray(rows).tolist(), np.asarray(cols).tolist(), np.asarray(wts).astype(int).tolist()))


@functools.lru_cache(maxsize=None)
def restated(case):
    _, gold = load_golden(f"vortex_{case}")
    return np_remove(gold["phase_ff"].astype(np.float64), gold["target"])


@functools.lru_cache(maxsize=None)
def yardsticks(case):
    """(d64, d32): restatement-to-reference distance of the cleaned float64 phase; the reference's float32 run against its
    float64 run on what was subtracted."""
    _, gold = load_golden(f"vortex_{case}")
    p = gold["phase_ff"].astype(np.float64)
    sub64 = p - gold["cleaned_f64"]
    return rel_l2(restated(case)[0], gold["cleaned_f64"]), rel_l2(p - gold["cleaned_f32"].astype(np.float64), sub64)


def make_hologram(case, dtype):
    meta, gold = load_golden(f"vortex_{case}")
    dt = np.dtype(dtype).type
    h = Hologram(gold["target"].astype(dt), slm_shape=tuple(meta["slm_shape"]), dtype=dt)
    h.phase_ff = gold["phase_ff"].astype(dt)
    return h, meta, gold


# ---- CPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_numpy_restatement_reproduces_reference(case):
    meta, gold = load_golden(f"vortex_{case}")
    p = gold["phase_ff"].astype(np.float64)
    assert np.array_equal(np_winding(p), gold["winding"].astype(np.float64))
    assert np.array_equal(np_winding(gold["phase_ff"]), gold["winding"].astype(np.float32))       # float32 arithmetic too
    cleaned, rows, cols, wts = restated(case)
    want = as_set(gold["rows"], gold["cols"], gold["weights"])
    assert as_set(rows, cols, wts) == want and len(want) == meta["n"]
    assert rel_l2(cleaned, gold["cleaned_f64"]) < 1e-13
    # the list the reference finds on its own output
    assert as_set(*np_vortices(gold["cleaned_f64"], gold["target"])) == as_set(gold["res_rows"], gold["res_cols"], gold["res_weights"])
    if case == "C":
        assert meta["n"] > 1024             # crosses the chunk of the list staging
    if case == "D":
        planted = meta["planted"]
        assert sorted((r, c) for r, c, _ in want) == sorted((y, x) for y, x, _, inside in planted if inside)
        assert all(gold["winding"][y, x] == 0 for y, x, _, _ in planted if y == 0 or x == 0)     # row / column 0: never found
        assert all(gold["winding"][y, x] != 0 for y, x, _, _ in planted if y > 0 and x > 0)


def test_no_phase_ff_is_a_no_op():
    h = Hologram(np.ones((64, 64), dtype=np.float32), slm_shape=(32, 32))
    assert h.remove_vortices() == 0 and h._remove_vortices() == 0
    assert h._engine is None and h.phase_ff is None
    (rows, cols), wts = h.get_vortices()
    assert len(rows) == len(cols) == len(wts) == 0


def test_spot_holograms_do_not_consider_vortices():
    vec = np.array([[20, 30, 40], [20, 34, 28]], dtype=float)
    s = SpotHologram((64, 64), vec, basis="knm", slm_shape=(32, 32))
    assert s.remove_vortices() == 0 and s._engine is None
    meta, gold = load_golden("compressed_2d50")
    fs = SimpleFourierSLM(SimpleSLM(tuple(meta["slm_shape"]), pitch_um=(8, 8), wav_um=0.78))
    c = CompressedSpotHologram(gold["spot_vectors"], basis="kxy", cameraslm=fs)
    assert c.remove_vortices() == 0 and c._engine is None
    a, b = Hologram(np.ones((64, 64)), slm_shape=(32, 32)), Hologram(np.ones((64, 64)), slm_shape=(32, 32))
    assert MultiplaneHologram([a, b]).remove_vortices() == 0 and a._engine is None and b._engine is None


def test_plot_is_refused():
    h = Hologram(np.ones((64, 64), dtype=np.float32), slm_shape=(32, 32))
    with pytest.raises(NotImplementedError, match="plot"):
        h._remove_vortices(plot=True)


def test_library_exports_the_call():
    import ctypes
    import os
    import slmsuite_amd
    assert "hgs_remove_vortices" in L.EXPORTS and L.VORTICES == 19
    lib = ctypes.CDLL(os.path.join(os.path.dirname(slmsuite_amd.__file__), "libhgs.so"))
    assert hasattr(lib, "hgs_remove_vortices")


# ---- GPU: fixtures A - D -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", CASES)
def test_matches_reference(case, dtype):
    """
    Measured on the MI355X, engine / yardstick: float64 A 5.6e-16 / 3.8e-16, B 1.8e-15 / 1.4e-15, C 3.7e-15 /
    3.0e-15, D 1.2e-16 / 1.1e-16; float32 A 1.0e-7 / 2.1e-7, B 1.7e-7 / 6.3e-7, C 2.5e-7 / 1.3e-6, D 6.7e-8 / 9.7e-8.
    """
    h, meta, gold = make_hologram(case, dtype)
    n = h.remove_vortices()
    (rows, cols), wts = h.get_vortices()
    d = dispatch_of(h)
    assert d.count("vortex_find_kernel") >= 1 and d.count("vortex_remove_kernel") == 1, d
    assert n == meta["n"] and wts.dtype == np.dtype(dtype)
    assert as_set(rows, cols, wts) == as_set(gold["rows"], gold["cols"], gold["weights"])
    got = np.array(h.phase_ff, dtype=np.float64)
    d64, d32 = yardsticks(case)
    if dtype is np.float64:
        err = rel_l2(got, gold["cleaned_f64"])
        print(f"vortex {case} f64: K {n}  engine {err:.3g}  d64 {d64:.3g}")
        assert err <= max(1e-9, 3 * d64), (err, d64)
    else:
        p = gold["phase_ff"].astype(np.float64)
        err = rel_l2(p - got, p - gold["cleaned_f64"])
        print(f"vortex {case} f32: K {n}  engine {err:.3g}  d32 {d32:.3g}")
        assert err <= 3 * d32, (err, d32)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_second_call_finds_the_reference_residual(dtype):
    """Removing a vortex leaves the neighbourhood changed: a second call finds what the reference finds on its own output."""
    h, meta, gold = make_hologram("A", dtype)
    assert h.remove_vortices() == meta["n"]
    assert h.remove_vortices() == meta["n_residual"]
    (rows, cols), wts = h.get_vortices()
    assert as_set(rows, cols, wts) == as_set(gold["res_rows"], gold["res_cols"], gold["res_weights"])


# ---- GPU: shapes the fixtures miss -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(45, 51), (32, 128), (128, 16)])
def test_odd_and_oblong_shapes_against_the_restatement(shape, dtype):
    """
    A pixel count that is no multiple of four or of the block (45 x 51: the tail lanes of both kernels, general layout) and
    oblong power-of-two grids (the lane-major column layout with Ph != Pw, either way round) against the restatement, which
    the CPU test ties to the reference: the list exactly -- the engine evaluates the winding in double in the same order
    of operations --, the cleaned phase to 1e-9 in float64; in float32 within 3 * d32, d32 taken here as the distance of
    a float32 vortex-by-vortex subtraction (what the reference does in float32) from the float64 one.
    """
    from slmsuite_amd import synth
    dt = np.dtype(dtype).type
    target = np.ones(shape, dtype=dt)
    target[:, shape[1] // 2] = np.nan                       # an MRAF column: outside the mask, like zero
    phase32 = synth.seed_phase(900 + shape[0], shape)
    h = Hologram(target, slm_shape=(max(shape[0] // 2, 8), max(shape[1] // 2, 8)), dtype=dt)
    h.phase_ff = phase32.astype(dt)
    cleaned, rows, cols, wts = np_remove(phase32.astype(np.float64), target)
    n = h.remove_vortices()
    (r, c), w = h.get_vortices()
    assert n == len(rows) > 20 and as_set(r, c, w) == as_set(rows, cols, wts)
    assert not np.any(np.abs(cols - shape[1] // 2) <= 2)
    got = np.array(h.phase_ff, dtype=np.float64)
    if dtype is np.float64:
        assert rel_l2(got, cleaned) <= 1e-9
    else:
        canvas = phase32.copy()
        X, Y = np.meshgrid(np.arange(shape[1], dtype=float), np.arange(shape[0], dtype=float))
        for x, y, wt in zip(cols, rows, wts):
            canvas -= wt * np.arctan2(X - x, Y - y)
        p = phase32.astype(np.float64)
        d32, err = rel_l2(p - canvas.astype(np.float64), p - cleaned), rel_l2(p - got, p - cleaned)
        print(f"vortex {shape} f32: K {n}  engine {err:.3g}  d32 {d32:.3g}")
        assert err <= 3 * d32, (err, d32)


# ---- GPU: other -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(64, 64), (48, 80)])
def test_nothing_inside_the_mask(shape, dtype):
    """Vortices only outside the eroded mask (and a smooth phase inside): 0, and phase_ff is untouched to the bit."""
    _, gold = load_golden("vortex_B")
    rng_phase = gold["phase_ff"][:shape[0], :shape[1]] if shape == (48, 80) else load_golden("vortex_C")[1]["phase_ff"][:64, :64]
    target = np.zeros(shape, dtype=dtype)
    target[20:30, 24:40] = 1
    phase = np.array(rng_phase, dtype=dtype)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    phase[18:32, 22:42] = (0.05 * yy + 0.03 * xx)[18:32, 22:42]            # smooth over the mask and its rim
    h = Hologram(target, slm_shape=(shape[0] // 2, shape[1] // 2), dtype=dtype)
    h.phase_ff = phase.copy()
    assert np.count_nonzero(np_winding(phase.astype(np.float64))) > 100      # plenty of vortices, all outside
    assert h.remove_vortices() == 0
    assert len(h.get_vortices()[1]) == 0
    assert np.array_equal(h.phase_ff.view(np.uint8), phase.view(np.uint8))


@pytest.mark.gpu
def test_two_calls_from_the_same_state_agree_to_the_bit():
    outs = []
    for _ in range(2):
        h, meta, gold = make_hologram("C", np.float32)
        assert h.remove_vortices() == meta["n"]
        outs.append((h._engine.get_vortices().copy(), np.array(h.phase_ff, copy=True)))
    assert np.array_equal(outs[0][0], outs[1][0])                          # the list, in the engine's own order
    assert np.array_equal(outs[0][1].view(np.uint8), outs[1][1].view(np.uint8))


@pytest.mark.gpu
def test_engine_refusals():
    h = Hologram(np.ones((64, 64), dtype=np.float32), slm_shape=(32, 32))
    e = h._get_engine()
    with pytest.raises(L.HgsError, match="phase_ff"):
        e.remove_vortices()
    meta, gold = load_golden("compressed_2d50")
    fs = SimpleFourierSLM(SimpleSLM(tuple(meta["slm_shape"]), pitch_um=(8, 8), wav_um=0.78))
    c = CompressedSpotHologram(gold["spot_vectors"], basis="kxy", cameraslm=fs)
    with pytest.raises(NotImplementedError, match="padded-grid"):
        c._get_engine().remove_vortices()


@pytest.mark.gpu
@pytest.mark.parametrize("loop", ["fused", "general"])
def test_callback_run_matches_reference(loop):
    """
    Case E through optimize(callback=...): WGS-Kim in float64, the phase fixed at iteration 3, its vortices removed once at
    iteration 5, ten bodies.  Final phase and phase_ff within 1e-9 as unit phasors.  The callback never reads phase_ff: on
    the fused loop no host copy of it exists until the run is over.  Measured on the MI355X: phase / phase_ff 1.4e-12 /
    4.2e-12 (fused), 1.5e-12 / 4.5e-12 (general); the reference itself moves by 3.3e-13 / 9.3e-13 under one ulp of the seed.
    """
    meta, gold = load_golden("vortex_E")
    h = Hologram(gold["target"].astype(np.float64), phase=gold["phase0"].astype(np.float64), slm_shape=tuple(meta["slm_shape"]),
                 dtype=np.float64)
    if loop == "general":
        force_stepwise(h)
    seen = {}

    def cb(hh):
        if hh.iter == meta["clean_at"]:
            assert hh.flags["fixed_phase"]
            seen["n"] = hh.remove_vortices()
            seen["host_copy"] = hh._host.get("phase_ff") is not None and "phase_ff" not in hh._stale
        return False

    h.optimize("WGS-Kim", maxiter=meta["maxiter"], verbose=False, fix_phase_iteration=meta["fix_phase_iteration"], callback=cb)
    assert seen["n"] > 0 and not seen["host_copy"]
    ep, ef = phase_rel_l2(h.phase, gold["final_phase"]), phase_rel_l2(h.phase_ff, gold["final_phase_ff"])
    print(f"vortex E {loop}: removed {seen['n']}  phase {ep:.3g}  phase_ff {ef:.3g}  (reference under one ulp: {meta['own_sensitivity']})")
    assert ep < 1e-9 and ef < 1e-9, (ep, ef)


@pytest.mark.gpu
@pytest.mark.parametrize("method,kw,clean_at", [("WGS-Kim", {"fix_phase_iteration": 3}, 5), ("GS", {}, 2)])
def test_reads_after_cleaning_agree_between_the_loops(method, kw, clean_at):
    """
    What a callback READS after it has cleaned: right away, and -- while the phase stays fixed -- in the next invocation
    (the cleaned array, not one formed afresh from the previous phase).  The device-resident loop against the general one,
    float64.  With a free phase (GS) the fused bodies store no farfield phase: it is formed on demand, then cleaned, and the
    next body describes a new one.
    """
    meta, gold = load_golden("vortex_E")
    got = {}
    for loop in ("fused", "general"):
        h = Hologram(gold["target"].astype(np.float64), phase=gold["phase0"].astype(np.float64),
                     slm_shape=tuple(meta["slm_shape"]), dtype=np.float64)
        if loop == "general":
            force_stepwise(h)
        seen = {}

        def cb(hh):
            if hh.iter == clean_at:
                seen["n"] = hh.remove_vortices()
                seen["now"] = np.array(hh.phase_ff, copy=True)
            elif hh.iter == clean_at + 1:
                seen["next"] = np.array(hh.phase_ff, copy=True)
            return False

        h.optimize(method, maxiter=clean_at + 3, verbose=False, callback=cb, **kw)
        got[loop] = seen
    f, g = got["fused"], got["general"]
    assert f["n"] == g["n"] > 0
    assert rel_l2(f["now"], g["now"]) < 1e-9
    if method == "WGS-Kim":
        assert rel_l2(f["next"], g["next"]) < 1e-9 and rel_l2(f["next"], f["now"]) < 1e-12       # fixed: it stays what it was
        assert len(np_vortices(f["next"], gold["target"])[0]) < f["n"]
    else:
        assert phase_rel_l2(f["next"], g["next"]) < 1e-9
