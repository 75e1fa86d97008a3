"""
GPU tests of the gratings, lenses and Gaussian-mode masks of toolbox.phase against the recorded reference
(tests/golden/pattern_*.npz, tools/make_golden_patterns.py).  Every raster asserts from the dispatch record which
pattern_kernel or poly_kernel instance ran.

Continuous values (blaze, sinusoid, lens, axicon, quadrants, the l-only Laguerre mask, bahtinov with blaze or sinusoid), relative L2:
    float64 grid   <= 1e-9 from ref64 (the project's float64 discriminator)
    float32 grid   <= max(3 d32, 2^-23) from ref64, d32 = ||ref32 - ref64|| / ||ref64|| (the reference's own float32 error;
                   2^-23: one rounding to float32 of a double evaluation)
    an identically zero ref64: array equality
Threshold values (binary, hermite_gaussian, Laguerre masks with p != 0, bahtinov with binary): array equality with the fixture
of the grid's type outside the marginal set 0 < |q| <= 1e-9 max|q| (binary: | |d| - 1e-8 | <= 1e-9), which is empty for
every recorded case.  laguerre_gaussian(l != 0, p != 0) adds a step to a continuous angle, whose last bit two math libraries
need not share: there the STEP SET (value minus l atan2(x, y), against pi / 2) is compared as arrays and the values by the
continuous bound.
The kernel makes one trip over its pixels (no grid-stride loop), so no case is sized by the CU count.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import dispatch_of, rel_l2
from pattern_cases import FUNCTIONS, call, case_ids, expected_launch, get_case, grid, is_threshold, marginal, reference, result_dtype
from slmsuite_amd import _lib as L
from slmsuite_amd import synth
from slmsuite_amd.engine import Engine
from slmsuite_amd.hardware import DisplaySLM
from slmsuite_amd.holography.algorithms import Hologram
from slmsuite_amd.holography.toolbox import phase

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)


def assert_launch(rec, case, dtype):
    family, args, flags = expected_launch(case, dtype)
    assert len(rec) == 1 and rec[0]["kernel"] == family and rec[0]["count"] == 1, rec
    assert rec[0]["args"] == args and rec[0]["flags"] == flags, (rec, args, flags)


@functools.lru_cache(maxsize=None)
def raster(case_id, dtype):
    """The recorded call on the GPU, once per (case, precision), with the instance the launch went to asserted."""
    case = get_case(case_id)
    phase.dispatch_read()
    out = call(phase, case, dtype)
    assert_launch(phase.dispatch_read(), case, dtype)
    assert isinstance(out, np.ndarray) and out.dtype == result_dtype(case, dtype) and out.shape == case["ref64"].shape, case_id
    out.setflags(write=False)
    return out


def check_continuous(case_id, got64, got32):
    case = get_case(case_id)
    ref = case["ref64"]
    if not ref.any():
        assert np.array_equal(got64, ref) and np.array_equal(got32, ref), case_id
        return
    d32 = rel_l2(case["ref32"], ref)
    e64, e32 = rel_l2(got64, ref), rel_l2(got32, ref)
    print(f"{case_id}: f64 err {e64:.3e} (bound 1e-9)  f32 err {e32:.3e}  d32 {d32:.3e}  bound {max(3 * d32, 2.0 ** -23):.3e}")
    assert e64 <= 1e-9, case_id
    assert e32 <= max(3 * d32, 2.0 ** -23), case_id


def check_threshold(case_id):
    case = get_case(case_id)
    keep = ~marginal(case)
    assert keep.mean() >= 0.999, case_id
    kw = case["call"]["kwargs"]
    stepped_angle = case["call"]["fn"] == "laguerre_gaussian" and kw["l"] != 0
    for dtype in DTYPES:
        got, ref = raster(case_id, dtype), reference(case, dtype)
        if stepped_angle:
            x, y = grid(case["call"]["grid"], dtype)
            angle = kw["l"] * np.arctan2(x.astype(np.float64), y.astype(np.float64))
            assert np.array_equal((got - angle > np.pi / 2)[keep], (ref - angle > np.pi / 2)[keep]), (case_id, dtype)
            print(f"{case_id} {np.dtype(dtype).name}: steps equal, {int(np.sum(got != ref))} of {got.size} values differ in the last bits")
        else:
            differ = int(np.sum((got != ref) & keep))
            print(f"{case_id} {np.dtype(dtype).name}: {differ} of {int(keep.sum())} compared pixels differ, {int((~keep).sum())} marginal")
            assert differ == 0, (case_id, dtype, np.argwhere((got != ref) & keep)[:5])
    if stepped_angle:
        check_continuous(case_id, raster(case_id, np.float64), raster(case_id, np.float32))


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_against_the_recorded_reference(fn):
    """Every recorded case of the function, 3 x 5 and 1 x 1 and the rotated (full-array) grid included, in both grid types."""
    ids = case_ids(fn)
    assert {c.rsplit("@")[1] for c in ids} >= {"slm", "odd", "rot", "tiny35", "tiny11"}
    for case_id in ids:
        if is_threshold(get_case(case_id)):
            check_threshold(case_id)
        else:
            check_continuous(case_id, raster(case_id, np.float64), raster(case_id, np.float32))


def test_lens_with_one_infinite_component():
    """Deliberately not the reference, which returns zeros here: against the NumPy expression."""
    for dtype in DTYPES:
        x, y = grid("rot", dtype)
        want = np.pi * np.square(x.astype(np.float64)) / 35.0
        phase.dispatch_read()
        got = phase.lens((x, y), (35.0, np.inf))
        rec = phase.dispatch_read()
        assert len(rec) == 1 and rec[0]["kernel"] == "poly_kernel" and rec[0]["args"]["PROD"] == "false", rec
        assert got.dtype == dtype and rel_l2(got, want) <= (1e-9 if dtype == np.float64 else 2.0 ** -23)


def test_zero_mode_mask_is_zeros_of_the_grid_type():
    for dtype in DTYPES:
        phase.dispatch_read()
        got = phase.laguerre_gaussian(grid("odd", dtype), 0, 0)
        rec = phase.dispatch_read()
        assert len(rec) == 1 and rec[0]["kernel"] == "pattern_kernel" and rec[0]["args"]["MODE"] == str(L.PATTERN_LG), rec
        assert got.dtype == dtype and got.shape == (37, 53) and not got.any()


# ---- tails and alignment -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", FUNCTIONS)
def test_unaligned_destinations(fn):
    """out= a torch view that starts 1, 2 and 3 elements into its storage, at 37 x 53: the loose values before the first and
    after the last aligned quad are written, nothing beside the view is."""
    import torch
    case_id = case_ids(fn, "odd")[0]
    case = get_case(case_id)
    for dtype in DTYPES:
        want = raster(case_id, dtype)
        assert want.size == 37 * 53 and want.dtype.kind == "f"
        for shift in (1, 2, 3):
            buf = torch.full((want.size + 8,), 7.0, dtype=getattr(torch, want.dtype.name), device="cuda")
            out = buf[shift:shift + want.size].view(want.shape)
            phase.dispatch_read()
            assert call(phase, case, dtype, out=out) is out
            assert_launch(phase.dispatch_read(), case, dtype)
            np.testing.assert_array_equal(out.cpu().numpy(), want)
            assert bool((buf[:shift] == 7).all()) and bool((buf[shift + want.size:] == 7).all())


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_routes(fn):
    """get=False: a CUDA tensor; out= a NumPy array; lazy=True: the descriptor rasters to the same bits; a prepared grid: the
    same bits again."""
    import torch
    case_id = case_ids(fn, "rot")[0]
    case = get_case(case_id)
    for dtype in DTYPES:
        want = raster(case_id, dtype)
        phase.dispatch_read()
        g = call(phase, case, dtype, get=False)
        assert_launch(phase.dispatch_read(), case, dtype)
        assert isinstance(g, torch.Tensor) and g.is_cuda and tuple(g.shape) == want.shape
        np.testing.assert_array_equal(g.cpu().numpy(), want)
        a = np.full(want.shape, 3.0, dtype=want.dtype)
        assert np.shares_memory(call(phase, case, dtype, out=a), a)
        np.testing.assert_array_equal(a, want)
        lazy = call(phase, case, dtype, lazy=True)
        assert isinstance(lazy, phase.PolynomialMask if fn in ("blaze", "lens") else phase.PatternMask)
        np.testing.assert_array_equal(np.asarray(lazy), want)
        phase.dispatch_read()
        np.testing.assert_array_equal(call(phase, case, dtype, prepare=True), want)
        assert_launch(phase.dispatch_read(), case, dtype)


def test_integer_levels():
    case = get_case("binary/ints@slm")
    got = raster("binary/ints@slm", np.float32)
    assert got.dtype == np.int64 and set(np.unique(got)) == {1, 3}
    out = np.zeros(got.shape, dtype=np.int64)
    assert call(phase, case, np.float32, out=out) is out and np.array_equal(out, got)
    with pytest.raises(ValueError, match="int64"):
        call(phase, case, np.float32, out=np.zeros(got.shape))


# ---- prepared grids ------------------------------------------------------------------------------------------------------------------
def test_prepared_grid_gives_the_same_bits():
    for name in ("slm", "rot"):
        for dtype in DTYPES:
            g = grid(name, dtype)
            p = phase.prepare_grid(g)
            w = np.array([0.5, -1.0, 2.0, 0.25], dtype=dtype)
            phase.dispatch_read()
            a = phase.zernike_sum(p, [2, 1, 4, 7], w, aperture="circular")
            rec = phase.dispatch_read()
            assert len(rec) == 1 and rec[0]["kernel"] == "poly_kernel" and rec[0]["args"]["PROD"] == ("true" if name == "slm" else "false"), rec
            np.testing.assert_array_equal(a, phase.zernike_sum(g, [2, 1, 4, 7], w, aperture="circular"))
            np.testing.assert_array_equal(phase.binary(p, (0.0031, 0.0017), 0.4, duty_cycle=0.3), phase.binary(g, (0.0031, 0.0017), 0.4, duty_cycle=0.3))
            np.testing.assert_array_equal(phase.laguerre_gaussian(p, 3, 2), phase.laguerre_gaussian(g, 3, 2))
            rec = phase.dispatch_read()
            assert [r["kernel"] for r in rec] == ["poly_kernel", "pattern_kernel", "pattern_kernel"] and [r["count"] for r in rec] == [1, 2, 2], rec


# ---- consumers -----------------------------------------------------------------------------------------------------------------------
def pattern_launches(engine, **args):
    return dispatch_of(engine).count("pattern_kernel", **args)


def masks(g, l=3, shift=0.4, scale=1):
    """One Laguerre-Gauss and one binary mask over ``g``; ``scale``: 250 for the small coordinates of the rotated grid."""
    return (phase.laguerre_gaussian(g, l, 2, lazy=True),
            phase.binary(g, (0.0031 * scale, 0.0017 * scale), shift, duty_cycle=0.3, lazy=True))


def test_get_display():
    g = grid("slm", np.float64)
    h = Hologram(synth.random_target(1, (64, 64)), slm_shape=(48, 64), phase=synth.seed_phase(19, (48, 64), dtype=np.float32))
    e = h._get_engine()
    for mask, mode in zip(masks(g), (L.PATTERN_LG, L.PATTERN_BINARY)):
        dispatch_of(e)
        got = h.get_display(phase_correction=mask)
        assert pattern_launches(e, R="double", OUT_BYTES=8, PROD=True, MODE=mode) == 1
        via_host = h.get_display(phase_correction=np.asarray(mask))
        assert got.dtype == np.uint8 and got.shape == (48, 64) and len(np.unique(got)) > 16
        np.testing.assert_array_equal(got, via_host)
    # a float32 grid fills the double correction with the values the host route stores
    for mask in masks(grid("slm", np.float32)) + (phase.bahtinov(grid("slm", np.float32), 0.006, lazy=True),):
        np.testing.assert_array_equal(h.get_display(phase_correction=mask), h.get_display(phase_correction=np.asarray(mask)))
    # slm.source["phase"] = mask on a DisplaySLM
    slm = DisplaySLM((48, 64), bitdepth=10)
    slm.source["phase"] = masks(g)[0]
    b = h.get_display(slm)
    slm.source["phase"] = np.asarray(masks(g)[0])
    np.testing.assert_array_equal(b, h.get_display(slm))
    with pytest.raises(ValueError, match="SLM shape"):
        h.get_display(phase_correction=phase.binary((g[0][:, :-1], g[1][:, :-1]), (0.003, 0.001), lazy=True))


def test_get_farfield():
    h = Hologram(synth.random_target(2, (64, 64)), slm_shape=(33, 50), phase=synth.seed_phase(3, (33, 50)))
    for dtype in DTYPES:
        for mask, mode in zip(masks(grid("rot", dtype), scale=250), (L.PATTERN_LG, L.PATTERN_BINARY)):
            assert len(np.unique(np.asarray(mask))) > 1
            ff = h.get_farfield(propagation_kernel=mask)
            side = h._ff_engines[(64, 64)]["engine"]
            assert pattern_launches(side, R={4: "float", 8: "double"}[np.dtype(dtype).itemsize], OUT_BYTES=4, PROD=False, MODE=mode) == 1
            want = h.get_farfield(propagation_kernel=np.asarray(mask))
            assert ff.dtype == np.complex64 and np.abs(ff).max() > 0
            np.testing.assert_array_equal(ff, want)
    assert not np.array_equal(h.get_farfield(propagation_kernel=0), ff)
    with pytest.raises(ValueError, match="SLM shape"):
        h.get_farfield(propagation_kernel=masks(grid("slm", np.float64))[0])


def test_upload_on_change():
    g = grid("slm", np.float64)
    h = Hologram(synth.random_target(1, (64, 64)), slm_shape=(48, 64), phase=synth.seed_phase(19, (48, 64), dtype=np.float32))
    e = h._get_engine()
    for which in (0, 1):
        dispatch_of(e)
        first = h.get_display(phase_correction=masks(g)[which])
        assert pattern_launches(e) == 1
        again = h.get_display(phase_correction=masks(g)[which])           # an equal mask, another object: nothing is formed
        assert dispatch_of(e).count("pattern_kernel") == 0
        np.testing.assert_array_equal(first, again)
        changed = h.get_display(phase_correction=masks(g, l=4, shift=0.9)[which])
        assert pattern_launches(e) == 1 and not np.array_equal(changed, first)
    # the same for the side engine's kernel slot
    h.get_farfield(propagation_kernel=masks(g)[0])
    side = h._ff_engines[(64, 64)]["engine"]
    assert pattern_launches(side) == 1
    h.get_farfield(propagation_kernel=masks(g)[0])
    assert pattern_launches(side) == 0
    h.get_farfield(propagation_kernel=masks(g, l=4)[0])
    assert pattern_launches(side) == 1


# ---- status codes --------------------------------------------------------------------------------------------------------------------
def test_status_codes():
    lib = L.load()
    x, y = np.meshgrid(np.linspace(-1, 1, 6), np.linspace(-1, 1, 4))
    e = Engine((64, 64), (4, 6), np.float32)

    def message():
        return lib.hgs_last_error().decode()

    ok, keep = phase.hermite_gaussian((x, y), 2, 1, lazy=True).params(out_bytes=8)
    wrong, keepw = phase.hermite_gaussian((x[:, :5], y[:, :5]), 2, 1, lazy=True).params()
    assert lib.hgs_set_array_pattern(e._h, L.PHASE, C.byref(wrong)) == L.HGS_ERR_ARG and "(4, 5)" in message() and "(4, 6)" in message()
    assert lib.hgs_set_array_pattern(e._h, L.TARGET, C.byref(ok)) == L.HGS_ERR_ARG and "HGS_PROP_KERNEL" in message()
    assert lib.hgs_set_array_pattern(None, L.PHASE, C.byref(ok)) == L.HGS_ERR_ARG
    # HGS_PHASE is filled and read back
    assert lib.hgs_set_array_pattern(e._h, L.PHASE, C.byref(ok)) == 0
    np.testing.assert_array_equal(e.get(L.PHASE)[0], phase.hermite_gaussian((x, y), 2, 1).astype(np.float32))
    out = np.zeros(23, dtype=np.float64)
    assert lib.hgs_pattern_eval(C.byref(ok), out.ctypes.data_as(C.c_void_p), out.nbytes, 0) == L.HGS_ERR_ARG
    assert "bad size 184 (192 expected" in message()
    full = np.zeros(24, dtype=np.float64)
    assert lib.hgs_pattern_eval(C.byref(ok), None, 192, 0) == L.HGS_ERR_ARG
    ok.n = L.PATTERN_MAX_ORDER + 1
    assert lib.hgs_pattern_eval(C.byref(ok), full.ctypes.data_as(C.c_void_p), full.nbytes, 0) == L.HGS_ERR_UNSUPPORTED
    assert f"limit of {L.PATTERN_MAX_ORDER}" in message()
    ok.n = -1
    assert lib.hgs_pattern_eval(C.byref(ok), full.ctypes.data_as(C.c_void_p), full.nbytes, 0) == L.HGS_ERR_ARG and "negative" in message()
    ok.n, ok.radius = 2, 0.0
    assert lib.hgs_pattern_eval(C.byref(ok), full.ctypes.data_as(C.c_void_p), full.nbytes, 0) == L.HGS_ERR_ARG and "radius" in message()
    ok.radius, ok.mode = 1.0, 9
    assert lib.hgs_pattern_eval(C.byref(ok), full.ctypes.data_as(C.c_void_p), full.nbytes, 0) == L.HGS_ERR_ARG and "unknown mode" in message()
    ok.mode, ok.quad = L.PATTERN_HG, 1
    assert lib.hgs_pattern_eval(C.byref(ok), full.ctypes.data_as(C.c_void_p), full.nbytes, 0) == L.HGS_ERR_ARG and "quadrants" in message()
    ok.quad, ok.x_axis = 0, None
    assert lib.hgs_pattern_eval(C.byref(ok), full.ctypes.data_as(C.c_void_p), full.nbytes, 0) == L.HGS_ERR_ARG and "axis vectors" in message()
    e.close()
