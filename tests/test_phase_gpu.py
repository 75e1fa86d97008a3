"""
GPU tests of toolbox.phase: the masks poly_kernel rasters against the recorded reference (tests/golden/phase_*.npz,
tools/make_golden_phase.py).  Yardsticks, as tests/test_cg.py sets them:

    d64 = rel_l2(ref64_alt, ref64)   two orders of evaluation of the reference in float64
    d32 = rel_l2(ref32, ref64)       the reference's own float32 error

float64 output lies within max(1e-9, 3 d64) of ref64; float32 output within 3 d32 of ref64 and within 2^-23 of ref64_on32
(float64 arithmetic on the widened float32 inputs: one rounding to float32 is 2^-24, the factor two is for the double
evaluation).  The masked SET is compared as arrays.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN, dispatch_of, rel_l2
from phase_cases import SlmGrid, call, case_ids, get_case, grids
from slmsuite_amd import _lib as L
from slmsuite_amd import synth
from slmsuite_amd.engine import Engine
from slmsuite_amd.hardware import DisplaySLM
from slmsuite_amd.holography.algorithms import Hologram
from slmsuite_amd.holography.toolbox import phase

pytestmark = pytest.mark.gpu

CASES = case_ids()
MASKED = [c for c in CASES if get_case(c)["call"].get("use_mask", "False") != "False"]


def rname(dtype):
    return {4: "float", 8: "double"}[np.dtype(dtype).itemsize]


def is_product(case):
    x, y = case["x"], case["y"]
    return x.ndim == 2 and bool(np.all(x == x[:1]) and np.all(y == y[:, :1]))


@functools.lru_cache(maxsize=None)
def raster(case_id, dtype):
    """The recorded call on the GPU, once per (case, precision), with the instance the launch went to asserted."""
    case = get_case(case_id)
    phase.dispatch_read()
    out = call(phase, case, dtype)
    rec = phase.dispatch_read()
    assert len(rec) == 1 and rec[0]["kernel"] == "poly_kernel" and rec[0]["count"] == 1, rec
    n = 1 if out.ndim == case["x"].ndim else out.shape[0]
    assert rec[0]["args"] == {"R": rname(dtype), "OUT_BYTES": str(np.dtype(dtype).itemsize), "PROD": "true" if is_product(case) else "false"}, rec
    assert rec[0]["flags"] == ({"batch"} if n > 1 else set()), rec
    assert isinstance(out, np.ndarray) and out.dtype == dtype
    out.setflags(write=False)
    return out


def test_both_grid_paths_are_covered():
    kinds = {is_product(get_case(c)) for c in CASES}
    assert kinds == {True, False}


# ---- accuracy and the masked set, one test per fixture file (every case of it is checked; the first that misses names itself) ---
def check_float64(case_id):
    case = get_case(case_id)
    got = raster(case_id, np.float64)
    assert got.shape == case["ref64"].shape, case_id
    d64 = rel_l2(case["ref64_alt"], case["ref64"])
    err = rel_l2(got, case["ref64"])
    print(f"{case_id}: f64 err {err:.3e}  d64 {d64:.3e}  bound {max(1e-9, 3 * d64):.3e}")
    assert np.array_equal(np.isnan(got), np.isnan(case["ref64"])), case_id
    assert err <= max(1e-9, 3 * d64), case_id


def check_float32(case_id):
    case = get_case(case_id)
    got = raster(case_id, np.float32)
    assert got.shape == case["ref32"].shape, case_id
    d32 = rel_l2(case["ref32"], case["ref64"])
    err = rel_l2(got, case["ref64"])
    inside = np.broadcast_to(case["mask32"], got.shape) if case_id in MASKED else np.ones(got.shape, dtype=bool)
    one = rel_l2(got[inside], case["ref64_on32"].reshape(got.shape)[inside])
    print(f"{case_id}: f32 err {err:.3e}  d32 {d32:.3e}  vs float64 on the float32 inputs {one:.3e} (2^-23 = {2.0 ** -23:.3e})")
    assert np.array_equal(np.isnan(got), np.isnan(case["ref32"])), case_id
    assert err <= 3 * d32, case_id
    assert one <= 2.0 ** -23, case_id


def check_mask_set(case_id):
    """the positions of exact zeros (use_mask=True) and of NaN equal the recorded mask as arrays, in both precisions"""
    case = get_case(case_id)
    for dtype, tag in ((np.float64, ""), (np.float32, "32")):
        got = raster(case_id, dtype)
        outside = np.broadcast_to(~case["mask" + tag], got.shape)
        if case["call"]["use_mask"] == "nan":
            assert np.array_equal(np.isnan(got), outside), case_id
        else:
            assert not np.isnan(got).any() and np.array_equal(got == 0, outside), case_id
        assert np.array_equal(call(phase, case, dtype, use_mask="return"), case["mask" + tag]), case_id


GROUPS = sorted({c.split("/")[0] for c in CASES})


@pytest.mark.parametrize("group", GROUPS)
def test_accuracy_and_mask_set(group):
    ids = [c for c in CASES if c.split("/")[0] == group]
    assert ids
    for case_id in ids:
        check_float64(case_id)
        check_float32(case_id)
        if case_id in MASKED:
            check_mask_set(case_id)


def test_every_case_is_checked():
    assert sorted(c for g in GROUPS for c in CASES if c.split("/")[0] == g) == sorted(CASES) and len(CASES) == 29
    assert len(MASKED) == 20


def test_masked_cases_cut_pixels():
    """every masked case but the circumscribed pupil ("cropped") and the single pixel has pixels on both sides of the edge"""
    for case_id in MASKED:
        m = get_case(case_id)["mask"]
        assert m.any() and ((~m).any() or case_id.endswith("/cropped") or case_id == "tiny/one"), case_id


# ---- the vortex plate ------------------------------------------------------------------------------------------------------------
def test_vortex():
    case = get_case("poly/terms")
    terms, w = case["terms"], case["weights"]
    assert tuple(terms[-1]) == (-1, 0) and w[-1, 0] > 0 > w[-1, 1]
    for dtype in (np.float64, np.float32):
        x, y = grids(case, dtype)
        with_plate = raster("poly/terms", dtype)
        without = phase.polynomial((x, y), w[:-1].astype(dtype), terms[:-1])
        np.testing.assert_array_equal(with_plate[1], without[1])          # a negative weight contributes nothing
        plate = with_plate[0].astype(np.float64) - without[0]
        want = w[-1, 0] * np.arctan2(y.astype(np.float64), x.astype(np.float64))
        assert rel_l2(plate, want) < (1e-12 if dtype == np.float64 else 1e-5)


# ---- shapes: every residue of the pixel count modulo a lane's four values, strides of a stack, unaligned destinations ------------
def test_edge_shapes():
    import torch
    sizes = {c: get_case(c)["x"].shape for c in ("tiny/one", "tiny/three_by_five", "stack/default_basis", "rot/rot", "prod_true/slm")}
    assert {s[0] * s[1] % 4 for s in sizes.values()} == {0, 1, 2, 3} and sizes["tiny/one"] == (1, 1)
    assert sizes["stack/default_basis"][1] == 53 and sizes["rot/rot"][1] == 50 and get_case("stack/default_basis")["ref64"].shape[0] == 3
    for case_id in sizes:
        case = get_case(case_id)
        for dtype in (np.float64, np.float32):
            want = raster(case_id, dtype)
            # the same masks into a destination that starts one, two and three elements past an aligned address
            for shift in (1, 2, 3):
                buf = torch.full((want.size + 8,), 7.0, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
                out = buf[shift:shift + want.size].view(want.shape)
                assert call(phase, case, dtype, out=out) is out
                np.testing.assert_array_equal(out.cpu().numpy(), want)
                assert bool((buf[:shift] == 7).all()) and bool((buf[shift + want.size:] == 7).all())     # nothing beside it
    # width 33: the rotated grid transposed (50 x 33, still no product grid)
    case = get_case("rot/rot")
    for dtype, ref in ((np.float64, "ref64"), (np.float32, "ref32")):
        x, y = grids(case, dtype)
        xt, yt = np.ascontiguousarray(x.T), np.ascontiguousarray(y.T)
        c = case["call"]
        got = phase.zernike_sum((xt, yt), c["indices"], case["weights"].astype(dtype), tuple(c["aperture"]), True)
        assert got.shape == (2, 50, 33)
        np.testing.assert_array_equal(got, raster("rot/rot", dtype).transpose(0, 2, 1))
    # W < 4 on a product grid
    x, y = np.meshgrid(np.array([-0.5, 0.0, 0.5]), np.linspace(-1, 1, 7))
    got = phase.zernike_sum((x, y), [2, 1, 4], [0.5, -1.0, 2.0], aperture=1.0, use_mask=False)
    np.testing.assert_allclose(got, 0.5 * x - y + 2.0 * (2 * x * x + 2 * y * y - 1), rtol=0, atol=1e-14)


# ---- routes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_in_place_and_lazy_routes(dtype):
    import torch
    case = get_case("stack/default_basis")
    want = raster("stack/default_basis", dtype)
    # out= a torch tensor: filled in place, returned
    t = torch.zeros(want.shape, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
    ptr = t.data_ptr()
    assert call(phase, case, dtype, out=t) is t and t.data_ptr() == ptr
    np.testing.assert_array_equal(t.cpu().numpy(), want)
    # out= a NumPy array
    a = np.full(want.shape, 3.0, dtype=dtype)
    back = call(phase, case, dtype, out=a)
    assert np.shares_memory(back, a)
    np.testing.assert_array_equal(a, want)
    # get=False: a CUDA tensor
    g = call(phase, case, dtype, get=False)
    assert isinstance(g, torch.Tensor) and g.is_cuda and tuple(g.shape) == want.shape
    np.testing.assert_array_equal(g.cpu().numpy(), want)
    # lazy: the descriptor rasters to the same bits
    lazy = call(phase, case, dtype, lazy=True)
    assert isinstance(lazy, phase.PolynomialMask) and lazy.shape == want.shape
    np.testing.assert_array_equal(np.asarray(lazy), want)
    # one mask of a zernike_sum drops the stack axis, polynomial keeps it
    one = get_case("prod_true/circular")
    assert np.asarray(call(phase, one, dtype, lazy=True)).shape == one["x"].shape
    assert raster("poly/cantor", dtype).shape == (2,) + get_case("poly/cantor")["x"].shape
    # zernike(): a single term
    x, y = grids(one, dtype)
    np.testing.assert_array_equal(phase.zernike((x, y), 4, 0.5, aperture="circular"),
                                  phase.zernike_sum((x, y), [4], [0.5], aperture="circular"))


# ---- consumers -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def display_case():
    d = np.load(os.path.join(GOLDEN, "phase_display.npz"))          # (plain arrays, no cases)
    return {k: d[k] for k in d.files}


def poly_launches(engine, **args):
    return dispatch_of(engine).count("poly_kernel", **args)


def test_get_display(display_case):
    d = display_case
    x, y, scaling = d["x"], d["y"], float(d["slm_scaling"])
    h = Hologram(synth.random_target(1, (64, 64)), slm_shape=x.shape, phase=d["phase"])
    lazy = phase.zernike_sum(SlmGrid(x, y, scaling), d["indices"], d["weights"], lazy=True)
    e = h._get_engine()
    dispatch_of(e)
    got = h.get_display(bitdepth=int(d["bitdepth"]), phase_scaling=float(d["scaling"]), phase_correction=lazy)
    assert poly_launches(e, R="double", OUT_BYTES=8, PROD=True) == 1
    via_host = h.get_display(bitdepth=int(d["bitdepth"]), phase_scaling=float(d["scaling"]), phase_correction=np.asarray(lazy))
    np.testing.assert_array_equal(got, via_host)
    np.testing.assert_array_equal(got, d["display"])                      # the reference SLM's levels
    assert rel_l2(np.asarray(lazy), d["correction"]) < 1e-12
    # a float32 mask fills the double correction with its float32 values, as the host route stores them
    lazy32 = phase.zernike_sum(SlmGrid(x.astype(np.float32), y.astype(np.float32), scaling), d["indices"],
                               d["weights"].astype(np.float32), lazy=True)
    dispatch_of(e)
    a = h.get_display(phase_correction=lazy32)
    assert poly_launches(e, R="float", OUT_BYTES=8, PROD=True) == 1
    np.testing.assert_array_equal(a, h.get_display(phase_correction=np.asarray(lazy32)))
    # slm.source["phase"] = mask on a DisplaySLM
    slm = DisplaySLM(x.shape, bitdepth=10)
    slm.source["phase"] = lazy
    b = h.get_display(slm)
    slm.source["phase"] = np.asarray(lazy)
    np.testing.assert_array_equal(b, h.get_display(slm))
    with pytest.raises(ValueError, match="SLM shape"):
        h.get_display(phase_correction=phase.zernike_sum((x[:, :-1], y[:, :-1]), [4], [1.0], lazy=True))


def test_get_farfield():
    case = get_case("rot/rot")                       # a full-grid mask into the side engine's kernel slot
    x, y = grids(case, np.float64)
    h = Hologram(synth.random_target(2, (64, 64)), slm_shape=x.shape, phase=synth.seed_phase(3, x.shape))
    for gx, gy in ((x, y), (x.astype(np.float32), y.astype(np.float32))):
        lazy = phase.zernike_sum((gx, gy), [2, 1, 4, 3], [3.0, -2.0, 5.0, 1.0], aperture=tuple(case["call"]["aperture"]),
                                 use_mask=False, lazy=True)
        ff = h.get_farfield(propagation_kernel=lazy)
        side = h._ff_engines[(64, 64)]["engine"]
        assert poly_launches(side, R=rname(gx.dtype), OUT_BYTES=4, PROD=False) == 1
        want = h.get_farfield(propagation_kernel=np.asarray(lazy))
        assert ff.dtype == np.complex64 and np.abs(ff).max() > 0
        np.testing.assert_array_equal(ff, want)
    plain = h.get_farfield(propagation_kernel=0)
    assert not np.array_equal(plain, ff)
    with pytest.raises(ValueError, match="SLM shape"):
        h.get_farfield(propagation_kernel=phase.zernike_sum((x, y), [2, 1], np.ones((2, 2)), lazy=True))


def test_upload_on_change(display_case):
    d = display_case
    x, y = d["x"], d["y"]
    h = Hologram(synth.random_target(1, (64, 64)), slm_shape=x.shape, phase=d["phase"])

    def mask(w0):
        return phase.zernike_sum((x, y), [2, 1, 4], [w0, 1.0, -2.0], aperture="circular", lazy=True)

    e = h._get_engine()
    dispatch_of(e)
    first = h.get_display(phase_correction=mask(0.5))
    assert poly_launches(e) == 1
    again = h.get_display(phase_correction=mask(0.5))                     # an equal mask, another object: nothing is formed
    assert poly_launches(e) == 0
    np.testing.assert_array_equal(first, again)
    changed = h.get_display(phase_correction=mask(2.5))
    assert poly_launches(e) == 1 and not np.array_equal(changed, first)
    # the same for the side engine's kernel slot
    h.get_farfield(propagation_kernel=mask(0.5))
    side = h._ff_engines[(64, 64)]["engine"]
    assert poly_launches(side) == 1
    h.get_farfield(propagation_kernel=mask(0.5))
    assert poly_launches(side) == 0
    h.get_farfield(propagation_kernel=mask(0.75))
    assert poly_launches(side) == 1


# ---- status codes ----------------------------------------------------------------------------------------------------------------
def test_status_codes():
    lib = L.load()
    x, y = np.meshgrid(np.linspace(-1, 1, 6), np.linspace(-1, 1, 4))
    e = Engine((64, 64), (4, 6), np.float32)

    def message():
        return lib.hgs_last_error().decode()

    def params(mask):
        prm, keep = mask.params()
        return prm, keep

    two, keep2 = params(phase.zernike_sum((x, y), [2, 1], np.ones((2, 2)), aperture=1.0, lazy=True))
    assert lib.hgs_set_array_poly(e._h, L.PROP_KERNEL, C.byref(two)) == L.HGS_ERR_ARG and "one mask" in message()
    wrong, keepw = params(phase.zernike_sum((x[:, :5], y[:, :5]), [2], [1.0], aperture=1.0, lazy=True))
    assert lib.hgs_set_array_poly(e._h, L.PHASE, C.byref(wrong)) == L.HGS_ERR_ARG and "(4, 5)" in message() and "(4, 6)" in message()
    ok, keepo = params(phase.zernike_sum((x, y), [2], [1.0], aperture=1.0, lazy=True))
    assert lib.hgs_set_array_poly(e._h, L.TARGET, C.byref(ok)) == L.HGS_ERR_ARG and "HGS_PROP_KERNEL" in message()
    assert lib.hgs_set_array_poly(None, L.PHASE, C.byref(ok)) == L.HGS_ERR_ARG
    # HGS_PHASE is filled and read back
    assert lib.hgs_set_array_poly(e._h, L.PHASE, C.byref(ok)) == 0
    np.testing.assert_array_equal(e.get(L.PHASE)[0], phase.zernike_sum((x, y), [2], [1.0], aperture=1.0).astype(np.float32))
    out = np.zeros(23, dtype=np.float64)
    assert lib.hgs_poly_eval(C.byref(ok), out.ctypes.data_as(C.c_void_p), out.nbytes, 0) == L.HGS_ERR_ARG
    assert "bad size 184 (192 expected" in message()
    assert lib.hgs_poly_eval(C.byref(ok), None, 192, 0) == L.HGS_ERR_ARG
    ok.degree = L.POLY_MAX_DEGREE + 1
    full = np.zeros(24, dtype=np.float64)
    assert lib.hgs_poly_eval(C.byref(ok), full.ctypes.data_as(C.c_void_p), full.nbytes, 0) == L.HGS_ERR_UNSUPPORTED
    assert f"limit of {L.POLY_MAX_DEGREE}" in message()
    ok.degree, ok.x_axis = 1, None
    assert lib.hgs_poly_eval(C.byref(ok), full.ctypes.data_as(C.c_void_p), full.nbytes, 0) == L.HGS_ERR_ARG and "axis vectors" in message()
    e.close()
