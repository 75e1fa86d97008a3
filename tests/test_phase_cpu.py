"""
toolbox.phase on the host: what the parser hands the kernel.  No GPU here -- the coefficient triangle of a lazy
``PolynomialMask`` is summed with NumPy in float64 and held against the recorded reference (tools/make_golden_phase.py),
the pupil scales against the recorded ones, the argument errors against the reference's exception types.
"""
import numpy as np
import pytest

from conftest import rel_l2
from phase_cases import call, case_ids, get_case, grids, table_eval
from slmsuite_amd import _lib as L
from slmsuite_amd.holography.toolbox import phase


GROUPS = sorted({c.split("/")[0] for c in case_ids()})


def in_group(group, kind=None):
    ids = [c for c in case_ids() if c.split("/")[0] == group and kind in (None, get_case(c)["call"]["kind"])]
    return ids


def test_every_case_is_in_a_group():
    assert sorted(c for g in GROUPS for c in in_group(g)) == sorted(case_ids()) and len(case_ids()) == 29


@pytest.mark.parametrize("group", GROUPS)
def test_host_table_reproduces_reference(group):
    """The triangle the host builds IS the recorded sum: <= 1e-10 relative L2 of ref64 inside the pupil (the table carries no
    mask), derivative and stack cases included.  One test per fixture file, every case of it."""
    for case_id in in_group(group):
        check_host_table(case_id)


def check_host_table(case_id):
    case = get_case(case_id)
    mask = call(phase, case, np.float64, lazy=True)
    assert isinstance(mask, phase.PolynomialMask) and mask.dtype == np.float64
    ref = case["ref64"]
    assert mask.shape == ref.shape
    got = table_eval(mask).reshape(ref.shape)
    if case["call"].get("use_mask", "False") != "False":
        inside = np.broadcast_to(case["mask"], ref.shape)
        assert mask.mask_mode == (L.POLY_MASK_ZERO if case["call"]["use_mask"] == "True" else L.POLY_MASK_NAN)
        got, ref = got[inside], ref[inside]
    else:
        assert mask.mask_mode == L.POLY_MASK_NONE
    err = rel_l2(got, ref)
    print(f"{case_id}: host table vs ref64 {err:.2e}")
    assert err <= 1e-10, case_id


@pytest.mark.parametrize("group", [g for g in GROUPS if in_group(g, "zernike")])
def test_aperture_scales_and_returned_mask(group):
    for case_id in in_group(group, "zernike"):
        check_scales_and_mask(case_id)


def check_scales_and_mask(case_id):
    case = get_case(case_id)
    for dtype, tag in ((np.float64, ""), (np.float32, "32")):
        x, y = grids(case, dtype)
        c = case["call"]
        ap = c["aperture"]
        if ap == "slm":
            from phase_cases import SlmGrid
            got = phase.zernike_aperture(SlmGrid(x, y, float(case["slm_scaling"])))
        else:
            got = phase.zernike_aperture((x, y), tuple(ap) if isinstance(ap, list) else ap)
        assert np.array_equal(np.asarray(got, dtype=dtype), case["scale" + tag]), case_id
        lazy = call(phase, case, dtype, lazy=True)
        assert (lazy.x_scale, lazy.y_scale) == tuple(float(s) for s in case["scale" + tag]), case_id
        returned = call(phase, case, dtype, use_mask="return")
        assert returned.dtype == bool and np.array_equal(returned, case["mask" + tag]), case_id


def test_product_and_full_grids_are_told_apart():
    prod = call(phase, get_case("prod_true/circular"), np.float32, lazy=True)
    rot = call(phase, get_case("rot/rot"), np.float32, lazy=True)
    assert prod.axes is not None and prod.grids is None and prod.axes[0].shape == (64,) and prod.axes[1].shape == (48,)
    assert rot.axes is None and rot.grids[0].shape == (33, 50)
    assert prod.dtype == np.float32 and rot.stack == 2 and rot.shape == (2, 33, 50)


def test_derivative_is_the_power_rule():
    """d/dx of Z4 = 2 x^2 + 2 y^2 - 1 is 4 x; d2/dy2 is 4; the mixed one vanishes."""
    x, y = np.meshgrid(np.linspace(-1, 1, 5), np.linspace(-1, 1, 4))
    for d, want in (((1, 0), 4 * x), ((0, 2), 4 + 0 * x), ((1, 1), 0 * x)):
        m = phase.zernike_sum((x, y), [4], [1.0], aperture=1.0, use_mask=False, derivative=d, lazy=True)
        assert np.allclose(table_eval(m)[0], want, atol=1e-14)


def test_vortex_term_counts_only_positive_weights():
    case = get_case("poly/terms")
    m = call(phase, case, np.float64, lazy=True)
    w = case["weights"][-1]
    assert w[0] > 0 > w[1] and np.array_equal(m.vortex, [w[0], 0.0])


def test_default_basis_and_cantor_terms():
    x, y = np.meshgrid(np.linspace(-1, 1, 6), np.linspace(-1, 1, 4))
    w = np.arange(1.0, 7.0)
    a = phase.zernike_sum((x, y), None, w, aperture=1.0, lazy=True)
    b = phase.zernike_sum((x, y), [2, 1, 4, 3, 5, 6], w, aperture=1.0, lazy=True)
    assert a.fingerprint == b.fingerprint
    # Cantor index 7 is x^2 y (w = 3, y = 1), 0 the constant
    p = phase.polynomial((x, y), [1.0, 2.0], [0, 7], lazy=True)
    q = phase.polynomial((x, y), [1.0, 2.0], [[0, 0], [2, 1]], pathing=False, lazy=True)
    assert p.fingerprint == q.fingerprint and p.degree == 3 and p.shape == (1, 4, 6)
    assert phase.polynomial((x, y), [1.0, 2.0], lazy=True).degree == 1          # terms=None: Cantor 0, 1 = (0, 0), (1, 0)


def test_argument_errors_are_the_references():
    x, y = np.meshgrid(np.linspace(-1, 1, 6), np.linspace(-1, 1, 4))
    g = (x, y)
    with pytest.raises(ValueError, match="not implemented"):
        phase.zernike_aperture(g, "square")
    with pytest.raises(ValueError, match="not recognized"):
        phase.zernike_aperture(g, (1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match="derivative"):
        phase.zernike_sum(g, [1], [1.0], derivative=(1,), lazy=True)
    with pytest.raises(ValueError, match="common dimension"):
        phase.zernike_sum(g, [1, 2], [1.0, 2.0, 3.0], lazy=True)
    with pytest.raises(ValueError, match="1D or 2D"):
        phase.zernike_sum(g, [1, 2], np.ones((2, 2, 2)), lazy=True)
    with pytest.raises(ValueError, match="common size"):
        phase.zernike_sum(g, [1, 2, 3], np.ones((2, 2)), lazy=True)
    with pytest.raises(ValueError, match="Unrecognized terms"):
        phase.zernike_sum(g, [1, -2], [1.0, 1.0], lazy=True)
    with pytest.raises(ValueError, match="shape"):
        phase.polynomial(g, [1.0], [[1, 2, 3]], lazy=True)
    with pytest.raises(ValueError, match="common dimension"):
        phase.polynomial(g, [1.0, 2.0], [[1, 2]], lazy=True)
    with pytest.raises(ValueError, match="1D or 2D"):
        phase.polynomial(g, np.ones((1, 1, 1)), [[1, 2]], lazy=True)
    with pytest.raises(ValueError, match="Unrecognized terms"):
        phase.polynomial(g, [1.0], [[-2, 0]], lazy=True)
    with pytest.raises(ValueError, match="same size"):
        phase.zernike_sum(g, [1], [1.0], out=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="same type"):
        phase.zernike_sum(g, [1], [1.0], out=np.zeros((4, 6), dtype=np.float32))


def test_degree_limit_is_refused():
    x, y = np.meshgrid(np.linspace(-1, 1, 6), np.linspace(-1, 1, 4))
    top = L.POLY_MAX_DEGREE
    assert phase.polynomial((x, y), [1.0], [[top, 0]], lazy=True).degree == top
    assert phase.polynomial((x, y), [1.0, 0.0], [[1, 0], [top + 5, 0]], lazy=True).degree == 1      # a zero weight adds no term
    with pytest.raises(NotImplementedError, match=f"limit of {top}"):
        phase.polynomial((x, y), [1.0], [[top, 1]], lazy=True)
    # radial order 10 -- ANSI 0 .. 65, 66 monomials -- is inside it
    assert phase.zernike_sum((x, y), list(range(66)), np.ones(66), aperture=1.0, lazy=True).degree == 10 <= top


def test_fingerprints():
    x, y = np.meshgrid(np.linspace(-1, 1, 6), np.linspace(-1, 1, 4))
    w = np.array([0.5, -1.0, 0.25])

    def make(grid=(x, y), weights=w, **kw):
        return phase.zernike_sum(grid, [2, 1, 4], weights, **dict(dict(aperture=0.9), **kw), lazy=True)

    base = make()
    assert make().fingerprint == base.fingerprint and make((x.copy(), y.copy()), w.copy()).fingerprint == base.fingerprint
    w2 = w.copy()
    w2[1] = np.nextafter(w2[1], 0)
    others = [make(weights=w2), make(aperture=0.91), make(use_mask=False), make(use_mask=np.nan), make(derivative=(1, 0)),
              make((x.astype(np.float32), y.astype(np.float32))), make((x * 1.5, y)),
              make((x + 0.01 * y, y))]                                            # (the last: no product grid any more)
    prints = [m.fingerprint for m in others] + [base.fingerprint]
    assert len(set(prints)) == len(prints)
    with pytest.raises(AttributeError):
        base.degree = 3
    with pytest.raises(ValueError):
        base.table[0, 0] = 1.0
