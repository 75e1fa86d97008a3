"""
CPU tests of the gratings, lenses and Gaussian-mode masks of toolbox.phase: argument handling, the polynomial folding of blaze
and lens against the recorded reference (tests/golden/pattern_*.npz, tools/make_golden_patterns.py), the descriptors and the
prepared grid.  Nothing here launches a kernel: the descriptors are built with ``lazy=True``.
"""
import numpy as np
import pytest

from conftest import rel_l2
from pattern_cases import FUNCTIONS, call, case_ids, get_case, grid, is_threshold, marginal, result_dtype
from phase_cases import table_eval
from slmsuite_amd import _lib as L
from slmsuite_amd.holography.toolbox import phase

GRID = grid("slm", np.float64)


class Slm:
    """An SLM as the functions see it: its grid and what it reports about its source."""

    def __init__(self, g, radius=None):
        self.grid = g
        if radius is not None:
            self.get_source_radius = lambda: radius


class Pair:
    def __init__(self, slm):
        self.slm, self.cam = slm, object()


def test_fixture_covers_the_issue():
    ids = case_ids()
    assert {c.split("/")[0] for c in ids} == set(FUNCTIONS)
    for fn in FUNCTIONS:                                 # every function at 3 x 5 and 1 x 1, on the rotated and the odd grid
        assert {c.rsplit("@")[1] for c in case_ids(fn)} >= {"slm", "odd", "rot", "tiny35", "tiny11"}, fn
    for c in ids:
        case = get_case(c)
        assert (case.get("q") is not None) == (is_threshold(case) and "zero_shift" not in c), c
        assert marginal(case).mean() <= 1e-3, c
    assert get_case("hermite_gaussian/n1_m0@odd")["q"][:, 26].tolist() == [0.0] * 37          # exact zeros of H_1 on the axis
    assert get_case("binary/ints@slm")["ref64"].dtype == np.int64


# ---- blaze and lens fold into the triangle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", case_ids("blaze") + case_ids("lens"))
def test_polynomial_folding(case_id):
    case = get_case(case_id)
    mask = call(phase, case, np.float64, lazy=True)
    assert isinstance(mask, phase.PolynomialMask) and mask.shape == case["ref64"].shape and mask.stack == 1
    kw = case["call"]["kwargs"]
    if case["call"]["fn"] == "blaze":
        v = kw["vector"]
        assert mask.degree == (2 if len(v) > 2 else 1 if any(v) else 0)
    else:
        assert mask.degree == 2 and mask.table.shape == (1, 6)
    got = table_eval(mask)[0]
    err = rel_l2(got, case["ref64"])
    assert err <= 1e-10 if np.any(case["ref64"]) else np.array_equal(got, case["ref64"]), (case_id, err)
    assert call(phase, case, np.float32, lazy=True).dtype == np.float32


def test_lens_with_one_infinite_component():
    x, y = GRID
    mask = phase.lens(GRID, (35.0, np.inf), lazy=True)              # (the reference returns zeros here: its dead branch)
    assert rel_l2(table_eval(mask)[0], np.pi * np.square(x) / 35.0) <= 1e-10
    mask = phase.lens(GRID, (np.inf, 35.0), lazy=True)
    assert rel_l2(table_eval(mask)[0], np.pi * np.square(y) / 35.0) <= 1e-10
    assert not table_eval(phase.lens(GRID, lazy=True)).any()
    assert phase.lens(GRID, 7, lazy=True).fingerprint == phase.lens(GRID, (7.0, 7.0), lazy=True).fingerprint


# ---- parsing and exception types ---------------------------------------------------------------------------------------------------
def test_focal_length_parsing():
    for fn in (phase.lens, phase.axicon):
        with pytest.raises(ValueError, match="zero"):
            fn(GRID, 0, lazy=True)
        with pytest.raises(ValueError, match="zero"):
            fn(GRID, (1.0, 0.0), lazy=True)
        with pytest.raises(ValueError, match="two terms"):
            fn(GRID, [1.0, 2.0, 3.0], lazy=True)
        with pytest.raises(ValueError, match="two terms"):
            fn(GRID, [1.0], lazy=True)
    m = phase.axicon(GRID, np.array([[3.0, 5.0]]), w=0.9, lazy=True)
    assert m.vectors[:2] == (0.9 / 3.0 / 2, 0.9 / 5.0 / 2) and m.mode == L.PATTERN_AXICON


def test_vector_parsing_and_descriptor_fields():
    m = phase.sinusoid(GRID, (0.004, 0.001), 0.7, 2.5, -0.5, lazy=True)
    assert isinstance(m, phase.PatternMask) and (m.mode, m.quad, m.shift, m.a, m.b) == (L.PATTERN_SINUSOID, False, 0.7, 2.5, -0.5)
    assert m.vectors == (0.004, 0.001) + (0.0,) * 6 and m.shape == GRID[0].shape and m.stack == 1
    with pytest.raises(ValueError, match="2-vector"):
        phase.sinusoid(GRID, (0.1, 0.2, 0.3), lazy=True)
    with pytest.raises(ValueError, match="2-vector"):
        phase.binary(GRID, (0.1,), lazy=True)
    b = phase.binary(GRID, (4, 6), duty_cycle=1.7, lazy=True)
    assert b.duty == 1.0 and phase.binary(GRID, (4, 6), duty_cycle=-3, lazy=True).duty == 0.0
    assert b.vectors[:2] == (4.0, 6.0)                   # (the library turns pixel periods into their reciprocals)
    # float64 scalars move the decision of a float32 grid to double, Python numbers do not (NumPy 2 promotion)
    g32 = grid("slm", np.float32)
    assert not phase.binary(g32, (0.003, 0.001), lazy=True).decision_double
    assert phase.binary(g32, np.array([0.003, 0.001]), lazy=True).decision_double
    assert phase.bahtinov(g32, lazy=True).decision_double


def test_result_types_follow_the_fixture():
    for case_id in case_ids(grid_name="slm"):
        case = get_case(case_id)
        for dtype in (np.float64, np.float32):
            mask = call(phase, case, dtype, lazy=True)
            want = result_dtype(case, dtype)
            got = mask.dtype if isinstance(mask, phase.PolynomialMask) else (mask.cast or mask.out_dtype)
            assert got == want, (case_id, dtype, got, want)
    zero = phase.laguerre_gaussian(grid("slm", np.float32), 0, 0, lazy=True)          # (the reference returns the integer 0)
    assert zero.out_dtype == np.float32 and (zero.l, zero.p) == (0, 0)


def test_quadrant_vectors_follow_the_reference_order():
    m = phase.quadrants(GRID, radius=0.004, center=(0.001, -0.0005), lazy=True)
    r = 0.004 / np.sqrt(2)
    want = [(r + 0.001, -r - 0.0005), (r + 0.001, r - 0.0005), (-r + 0.001, -r - 0.0005), (-r + 0.001, r - 0.0005)]
    assert m.quad and m.mode == L.PATTERN_BLAZE and np.allclose(np.reshape(m.vectors, (4, 2)), want, rtol=1e-15, atol=0)
    b = phase.bahtinov(GRID, radius=0.006, angle=0.3, grating=phase.sinusoid, lazy=True)
    s, c = 0.006 * np.sin(0.3), 0.006 * np.cos(0.3)
    assert b.mode == L.PATTERN_SINUSOID and np.allclose(np.reshape(b.vectors, (4, 2)), [(s, c), (s, -c), (0, 0.006), (0, 0.006)], rtol=1e-15, atol=0)
    assert phase.bahtinov(GRID, lazy=True).mode == L.PATTERN_BINARY and phase.bahtinov(GRID, grating=phase.blaze, lazy=True).mode == L.PATTERN_BLAZE
    for other in (np.sin, phase.lens, lambda grid, vector: 0):
        with pytest.raises(TypeError, match="binary, blaze or sinusoid"):
            phase.bahtinov(GRID, grating=other, lazy=True)
    with pytest.raises(ValueError, match="2-D"):
        phase.quadrants((GRID[0].ravel(), GRID[1].ravel()), lazy=True)


def test_not_implemented_functions_and_order_limit():
    for fn, args in ((phase.ince_gaussian, (3, 1)), (phase.matheui_gaussian, (1, 1)), (phase.airy, ())):
        with pytest.raises(NotImplementedError):
            fn(GRID, *args)
    limit = L.PATTERN_MAX_ORDER
    assert limit == L.POLY_MAX_DEGREE == 20
    phase.laguerre_gaussian(GRID, 1, limit, lazy=True)
    phase.hermite_gaussian(GRID, limit, limit, lazy=True)
    for make in (lambda: phase.laguerre_gaussian(GRID, 1, limit + 1, lazy=True), lambda: phase.hermite_gaussian(GRID, limit + 1, 0, lazy=True),
                 lambda: phase.hermite_gaussian(GRID, 0, limit + 1, lazy=True)):
        with pytest.raises(NotImplementedError, match=f"limit of {limit}"):
            make()
    with pytest.raises(ValueError, match="negative"):
        phase.laguerre_gaussian(GRID, 1, -1, lazy=True)
    with pytest.raises(ValueError, match="negative"):
        phase.hermite_gaussian(GRID, -2, 0, lazy=True)


# ---- the source radius ----------------------------------------------------------------------------------------------------------------
def test_source_radius_rule():
    x, y = GRID
    default = min(x.max(), y.max()) / 4
    assert phase.hermite_gaussian(GRID, 1, 1, lazy=True).radius == default
    assert phase.hermite_gaussian(GRID, 1, 1, w=0.25, lazy=True).radius == 0.25
    assert phase.hermite_gaussian(Slm(GRID), 1, 1, lazy=True).radius == default              # an SLM that reports none
    assert phase.hermite_gaussian(Slm(GRID, 0.5), 1, 1, lazy=True).radius == 0.5
    assert phase.laguerre_gaussian(Pair(Slm(GRID, 0.5)), 1, 2, lazy=True).radius == 0.5     # a camera-SLM pair: its SLM
    assert phase.axicon(Slm(GRID, 0.5), (2.0, 4.0), lazy=True).vectors[:2] == (0.125, 0.0625)
    assert phase.axicon(Slm(GRID, 0.5), (2.0, 4.0), w=1.0, lazy=True).vectors[:2] == (0.25, 0.125)
    g32 = grid("slm", np.float32)
    assert phase.hermite_gaussian(g32, 1, 1, lazy=True).radius == float(min(g32[0].max(), g32[1].max()) / np.float32(4))
    prepared = phase.prepare_grid(Slm(GRID, 0.5))
    assert prepared.radius == default and phase.hermite_gaussian(prepared, 1, 1, lazy=True).radius == 0.5


# ---- immutability and fingerprints -------------------------------------------------------------------------------------------------------
def test_descriptors_are_immutable():
    m = phase.binary(GRID, (0.003, 0.001), lazy=True)
    p = phase.prepare_grid(GRID)
    for obj, name in ((m, "a"), (m, "vectors"), (m, "fingerprint"), (p, "radius"), (p, "axes"), (p, "x")):
        with pytest.raises(AttributeError, match="immutable"):
            setattr(obj, name, 1)
    with pytest.raises(AttributeError):
        m.other = 1
    for a in (p.x, p.y) + p.axes:
        with pytest.raises(ValueError):
            a[...] = 0
    x = GRID[0].copy()
    q = phase.prepare_grid((x, GRID[1]))
    x[0, 0] += 1.0                                       # the prepared grid keeps its own copy
    assert q.x[0, 0] == GRID[0][0, 0] and phase.prepare_grid(q) is q


def test_fingerprints():
    base = dict(vector=(0.003, 0.001), shift=0.4, a=np.pi, b=0.5, duty_cycle=0.3)
    fp = phase.binary(GRID, lazy=True, **base).fingerprint
    assert phase.binary((GRID[0].copy(), GRID[1].copy()), lazy=True, **base).fingerprint == fp
    assert phase.binary(phase.prepare_grid(GRID), lazy=True, **base).fingerprint == fp
    seen = {fp}
    for key, value in (("vector", (0.003, 0.002)), ("shift", 0.5), ("a", 3.0), ("b", 0.25), ("duty_cycle", 0.31)):
        other = phase.binary(GRID, lazy=True, **{**base, key: value}).fingerprint
        assert other not in seen, key
        seen.add(other)
    assert phase.binary(grid("slm", np.float32), lazy=True, **base).fingerprint not in seen
    assert phase.binary(grid("odd", np.float64), lazy=True, **base).fingerprint not in seen
    assert phase.sinusoid(GRID, (0.003, 0.001), 0.4, np.pi, 0.5, lazy=True).fingerprint not in seen
    rot = grid("rot", np.float64)
    moved = (rot[0] + 1e-9, rot[1])
    lg = [phase.laguerre_gaussian(g, l, p, w=w, lazy=True).fingerprint
          for g, l, p, w in ((rot, 3, 2, 0.1), (rot, 3, 2, 0.1), (rot, -3, 2, 0.1), (rot, 3, 1, 0.1), (rot, 3, 2, 0.11), (moved, 3, 2, 0.1))]
    assert lg[0] == lg[1] and len(set(lg)) == 5
    hg = {phase.hermite_gaussian(GRID, n, m, lazy=True).fingerprint for n, m in ((1, 2), (2, 1), (1, 1))}
    assert len(hg) == 3
    quads = {phase.quadrants(GRID, r, c, lazy=True).fingerprint for r, c in ((0.004, (0, 0)), (0.005, (0, 0)), (0.004, (0.001, 0)))}
    assert len(quads) == 3


def test_prepared_grid_fields():
    p = phase.prepare_grid(GRID)
    assert p.shape == (48, 64) and p.dtype == np.float64 and p.axes is not None and p.hardware is None
    assert np.array_equal(p.axes[0], GRID[0][0]) and np.array_equal(p.axes[1], GRID[1][:, 0])
    r = phase.prepare_grid(grid("rot", np.float32))
    assert r.axes is None and r.dtype == np.float32 and r.grid[0] is r.x
    slm = Slm(GRID, 0.5)
    assert phase.prepare_grid(Pair(slm)).hardware is slm
    # the four polynomial functions take it and build the descriptor they build from the raw grid
    w = [0.5, -1.0, 2.0]
    for g in (GRID, grid("rot", np.float64)):
        raw = phase.zernike_sum(g, [2, 1, 4], w, aperture="circular", lazy=True)
        pre = phase.zernike_sum(phase.prepare_grid(g), [2, 1, 4], w, aperture="circular", lazy=True)
        assert raw.fingerprint == pre.fingerprint and np.array_equal(raw.table, pre.table) and (raw.x_scale, raw.y_scale) == (pre.x_scale, pre.y_scale)
        assert phase.polynomial(phase.prepare_grid(g), w, lazy=True).fingerprint == phase.polynomial(g, w, lazy=True).fingerprint
        assert phase.zernike(phase.prepare_grid(g), 4, 0.5, lazy=True).fingerprint == phase.zernike(g, 4, 0.5, lazy=True).fingerprint
        assert phase.zernike_aperture(phase.prepare_grid(g)) == phase.zernike_aperture(g)
        assert np.array_equal(phase.zernike_sum(phase.prepare_grid(g), [4], [1.0], use_mask="return"), phase.zernike_sum(g, [4], [1.0], use_mask="return"))
