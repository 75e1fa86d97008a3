"""
Phase masks formed on the GPU, with the signatures and argument handling of the reference's ``toolbox.phase``:

* polynomials (phase.py:683-1166, :1672-1795, :37-75, :409-452): ``polynomial``, ``zernike_sum``, ``zernike``,
  ``zernike_aperture``, ``blaze`` and ``lens``.  The host only parses: terms and weights are folded into a dense triangle of
  monomial coefficients (``PolynomialMask``) and ``hgs_poly_eval`` rasters it -- Horner's scheme in double for either grid
  type, one rounding to the grid's type (include/hgs.h, csrc/poly_kernels.hpp).
* gratings, lenses that are no polynomials and Gaussian-mode masks (phase.py:78-389, :455-498, :1800-1935): ``sinusoid``,
  ``binary``, ``quadrants``, ``bahtinov``, ``axicon``, ``laguerre_gaussian``, ``hermite_gaussian``.  A few dozen numbers
  describe one (``PatternMask``) and ``hgs_pattern_eval`` rasters it (csrc/pattern_kernels.hpp): ``sin``, ``sqrt``, ``atan2``
  and the Laguerre / Hermite recurrences in double; the decision quantity of ``binary`` with NumPy's own roundings, so the
  pixels that receive ``a`` are the reference's.  ``ince_gaussian``, ``matheui_gaussian`` and ``airy`` raise
  ``NotImplementedError``, as in the reference.

Every function takes ``out=None, get=True, lazy=False`` (see :func:`polynomial`); ``lazy=True`` returns the immutable
descriptor, which ``Hologram.get_display(phase_correction=)`` and ``get_farfield(propagation_kernel=)`` accept in place of an
SLM-sized host array.  ``prepare_grid(grid)`` parses a grid once (``PreparedGrid``); every function accepts the result as
``grid`` and skips the parse.  There is no CPU route: without a GPU the functions raise ``HgsError``; only ``lazy=True``,
``use_mask="return"`` and ``zernike_aperture`` need none.

Where this differs from the reference on purpose:

* float32 grids are evaluated in double from the widened coordinates and rounded once where the values are continuous, and
  the monomial coefficients are not rounded to float32 first; the reference multiplies float32 arrays.  The result is the
  closer one to exact.
* Result types follow the reference under NumPy 2 (``binary`` and ``hermite_gaussian`` return float64 for either grid,
  ``axicon`` and ``laguerre_gaussian(l=0)`` too, ``binary`` with two Python ints int64), except that the polynomials
  ``blaze`` and ``lens`` keep the grid's type like every polynomial here.
* ``lens(grid, (fx, inf))`` is ``pi x^2 / fx``; the reference returns zeros there (its second branch repeats the first
  condition, phase.py:445-452).
* ``laguerre_gaussian(l=0, p=0)`` is a zero array of the grid's type; the reference returns the integer 0.
* ``sinusoid`` and ``binary`` take 2-vectors whose components count as Python floats (float64 scalars or arrays move the
  decision quantity of ``binary`` on a float32 grid to double, as NumPy 2 promotes them); ``shift`` counts as a Python float.
* Orders ``p``, ``n``, ``m`` above 20 raise ``NotImplementedError`` (the limit of the polynomial degree here).
* ``polynomial(terms=None)`` takes the Cantor indices ``0 .. D-1`` as the reference documents (its code raises there).
* ``pathing`` is accepted and ignored: the order of evaluation is Horner's.
"""
import ctypes as C
import hashlib
import sys

import numpy as np

from slmsuite_amd import _lib as L
from slmsuite_amd.holography import toolbox

__all__ = ["PolynomialMask", "PatternMask", "PreparedGrid", "prepare_grid", "polynomial", "zernike", "zernike_sum",
           "zernike_aperture", "blaze", "sinusoid", "binary", "bahtinov", "quadrants", "lens", "axicon", "laguerre_gaussian",
           "hermite_gaussian", "ince_gaussian", "matheui_gaussian", "airy"]


# ---- grids --------------------------------------------------------------------------------------------------------
def _product_axes(x, y):
    """(x[W], y[H]) when x varies along the last axis only and y along the first only, else None."""
    if x.ndim != 2 or x.size == 0:
        return None
    if np.array_equal(x, np.broadcast_to(x[:1, :], x.shape)) and np.array_equal(y, np.broadcast_to(y[:, :1], y.shape)):
        return x[0, :].copy(), y[:, 0].copy()
    return None


class PreparedGrid:
    """
    A grid parsed once: ``x`` and ``y`` as float32 / float64 arrays of one shape and one type (``grid`` is the pair),
    ``dtype``, ``shape``, ``axes`` -- the two axis vectors when it is a product grid, else ``None`` --, ``radius`` -- the
    default source radius, a quarter of the smaller of the two largest coordinates (phase.py:1838-1839) -- and ``hardware``,
    the SLM it came from (asked for its source radius and Zernike scaling as the reference asks the SLM).  Immutable.
    :func:`prepare_grid` makes one; every function of this module takes it as ``grid`` and skips the parse.
    """

    __slots__ = ("x", "y", "grid", "dtype", "shape", "axes", "radius", "hardware", "_hash")

    def __init__(self, grid, copy=True):
        hardware = grid.slm if hasattr(grid, "slm") and hasattr(grid, "cam") else grid
        x, y = toolbox.process_grid(grid)
        x, y = np.asarray(x), np.asarray(y)
        if x.shape != y.shape:
            raise ValueError(f"x_grid {x.shape} and y_grid {y.shape} differ in shape")
        dt = np.result_type(x.dtype, y.dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            dt = np.dtype(np.float64)
        x, y = np.ascontiguousarray(x, dtype=dt), np.ascontiguousarray(y, dtype=dt)
        axes = _product_axes(x, y)
        if copy or axes is None:                    # (its own: the caller may go on editing the grid)
            x, y = x.copy(), y.copy()
            x.setflags(write=False)
            y.setflags(write=False)
        h = hashlib.sha1(repr((dt.str, tuple(x.shape), axes is not None)).encode())
        for a in axes if axes is not None else (x, y):
            a.setflags(write=False)
            h.update(memoryview(a).cast("B") if a.size else b"")
            h.update(b"|")
        lead = axes if axes is not None else (x, y)
        put = object.__setattr__
        put(self, "x", x)
        put(self, "y", y)
        put(self, "grid", (x, y))
        put(self, "dtype", dt)
        put(self, "shape", tuple(x.shape))
        put(self, "axes", axes)
        put(self, "radius", np.min([np.amax(lead[0]), np.amax(lead[1])]) / 4 if x.size else dt.type(np.nan))
        put(self, "hardware", None if isinstance(hardware, (tuple, list)) else hardware)
        put(self, "_hash", h)

    def __setattr__(self, name, value):
        raise AttributeError("PreparedGrid is immutable")

    def __repr__(self):
        return f"PreparedGrid(shape={self.shape}, dtype={self.dtype.name}, {'product' if self.axes is not None else 'full'} grid)"


def prepare_grid(grid):
    """The grid parsed once (:class:`PreparedGrid`): pass the result as ``grid`` to any function of this module."""
    return grid if isinstance(grid, PreparedGrid) else PreparedGrid(grid)


def _prepared(grid):
    """``grid`` as a PreparedGrid: itself when it is one, else parsed for this call."""
    return grid if isinstance(grid, PreparedGrid) else PreparedGrid(grid, copy=False)


def _hardware(grid):
    """What the reference asks for source properties: the SLM of a cameraslm, the SLM, or the grid itself."""
    if isinstance(grid, PreparedGrid):
        return grid.hardware
    return grid.slm if hasattr(grid, "slm") and hasattr(grid, "cam") else grid


def _raster_shape(shape):
    """(H, W) the kernel walks for a grid of ``shape``: the grid itself when 2-D, one row of all its values otherwise."""
    if len(shape) == 2:
        return int(shape[0]), int(shape[1])
    return 1, int(np.prod(shape, dtype=np.int64))


# ---- the descriptor -----------------------------------------------------------------------------------------------
def _row_start(degree, b):
    """Where row ``b`` (the coefficients of y^b, x ascending) starts in the triangle of ``degree``."""
    return b * (degree + 1) - b * (b - 1) // 2


def _fold_terms(terms, weights):
    """
    (degree, table [N, T], vortex [N] or None) from terms (M, 2) and weights (M, N): ``table[n, row(b) + a]`` sums the
    weights of x^a y^b; the pseudo-term (-1, 0) is the vortex plate and counts where its weight is positive
    (phase.py:1783-1791).  Terms whose weights all vanish add nothing, as in the reference, and do not raise the degree.
    """
    M, N = weights.shape
    for index, (nx, ny) in enumerate(terms):
        if nx < 0 and not (nx == -1 and ny == 0) or ny < 0:
            raise ValueError(f"Unrecognized terms {(int(nx), int(ny))} for index {index}.")
    live = [m for m in range(M) if terms[m, 0] >= 0 and np.any(weights[m] != 0)]
    degree = max([int(terms[m, 0] + terms[m, 1]) for m in live], default=0)
    if degree > L.POLY_MAX_DEGREE:
        raise NotImplementedError(f"polynomial mask: degree {degree} is beyond the limit of {L.POLY_MAX_DEGREE}")
    table = np.zeros((N, (degree + 1) * (degree + 2) // 2), dtype=np.float64)
    for m in live:
        table[:, _row_start(degree, int(terms[m, 1])) + int(terms[m, 0])] += weights[m]
    vortex = None
    for m in range(M):
        if terms[m, 0] == -1:
            vortex = np.zeros(N, dtype=np.float64) if vortex is None else vortex
            vortex += np.where(weights[m] > 0, weights[m], 0.0)
    return degree, table, vortex


class PolynomialMask:
    """
    A stack of ``stack`` polynomial phase masks over a grid, not yet rastered: the coefficient triangle, the vortex
    weights, the pupil scales and mask mode, and the coordinates -- two axis vectors for a product grid, the two arrays
    otherwise.  Immutable; ``fingerprint`` identifies the content, so consumers that hold a device copy
    (``Hologram.get_display(phase_correction=mask)``, ``get_farfield(propagation_kernel=mask)``) form it again only when
    it changed.  ``np.asarray(mask)`` rasters it with the kernel the eager functions use.
    """

    __slots__ = ("shape", "grid_shape", "stack", "dtype", "degree", "table", "vortex", "mask_mode", "x_scale", "y_scale",
                 "axes", "grids", "fingerprint", "_squeeze")

    def __init__(self, grid, terms, weights, x_scale=1.0, y_scale=1.0, mask_mode=L.POLY_MASK_NONE, squeeze=False):
        terms = np.asarray(terms, dtype=np.int64).reshape(-1, 2)
        weights = np.asarray(weights, dtype=np.float64)
        degree, table, vortex = _fold_terms(terms, weights)
        put = object.__setattr__
        put(self, "dtype", grid.dtype)
        put(self, "grid_shape", grid.shape)
        put(self, "stack", int(weights.shape[1]))
        put(self, "_squeeze", bool(squeeze) and weights.shape[1] == 1)
        put(self, "shape", self.grid_shape if self._squeeze else (self.stack,) + self.grid_shape)
        put(self, "degree", degree)
        put(self, "mask_mode", int(mask_mode))
        # the scales meet the grid in its type (NumPy: a Python float times a float32 array is a float32 product)
        put(self, "x_scale", float(np.asarray(x_scale, dtype=grid.dtype)))
        put(self, "y_scale", float(np.asarray(y_scale, dtype=grid.dtype)))
        put(self, "axes", grid.axes)
        put(self, "grids", None if grid.axes is not None else grid.grid)
        h = grid._hash.copy()                      # (the coordinates are in it already)
        h.update(repr(("poly", self.stack, degree, self.mask_mode, self.x_scale, self.y_scale, self._squeeze)).encode())
        for a in (table, vortex):
            if a is not None:
                a.setflags(write=False)
                h.update(memoryview(a).cast("B"))
            h.update(b"|")
        put(self, "table", table)
        put(self, "vortex", vortex)
        put(self, "fingerprint", h.hexdigest())

    def __setattr__(self, name, value):
        raise AttributeError("PolynomialMask is immutable")

    def __repr__(self):
        return (f"PolynomialMask(shape={self.shape}, dtype={self.dtype.name}, degree={self.degree}, "
                f"{'product' if self.axes is not None else 'full'} grid, fingerprint={self.fingerprint[:12]})")

    def params(self, out_bytes=0, device=0):
        """(hgs_poly_params, the arrays it points into -- keep them until the call returned)."""
        h, w = _raster_shape(self.grid_shape)
        keep = [self.table, self.vortex, self.axes, self.grids]
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        ax, gr = self.axes or (None, None), self.grids or (None, None)
        prm = L.hgs_poly_params(h=h, w=w, n=self.stack, degree=self.degree, grid_bytes=self.dtype.itemsize,
                                out_bytes=int(out_bytes), mask_mode=self.mask_mode, device=int(device),
                                x_scale=self.x_scale, y_scale=self.y_scale, table=ptr(self.table), vortex=ptr(self.vortex),
                                x_axis=ptr(ax[0]), y_axis=ptr(ax[1]), x_grid=ptr(gr[0]), y_grid=ptr(gr[1]))
        return prm, keep

    def _eval(self, pointer, nbytes, on_device, device):
        prm, keep = self.params(device=device)
        L.check(L.load().hgs_poly_eval(C.byref(prm), pointer, nbytes, int(on_device)))

    def raster(self, out=None, get=True, device=0):
        """The masks, as ``polynomial`` / ``zernike_sum`` return them (see their ``out`` and ``get``)."""
        return _raster(self, self.dtype, out, get, device)

    def __array__(self, dtype=None, copy=None):
        a = self.raster()
        return a if dtype is None else a.astype(dtype, copy=False)


def _is_device_tensor(value):
    return type(value).__module__.split(".")[0] == "torch" and bool(getattr(value, "is_cuda", False))


def _wait_for_torch(tensor):
    """The library writes on its own stream: what torch still has in flight for this block must have landed first."""
    sys.modules["torch"].cuda.current_stream(tensor.device).synchronize()


def _raster(mask, dtype, out, get, device):
    """``mask`` (its ``shape``, its ``_eval``) as ``dtype`` values: into ``out`` (NumPy array or torch CUDA tensor of that size
    and type), else a new NumPy array, or for ``get=False`` a new torch CUDA tensor where the process works with torch."""
    size = int(np.prod(mask.shape, dtype=np.int64))
    if out is not None and _is_device_tensor(out):
        if out.numel() != size:
            raise ValueError("out must have same size as the stacked grid.")
        if str(out.dtype).split(".")[-1] != dtype.name:
            raise ValueError("out must have same type as grid.")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous.")
        _wait_for_torch(out)
        mask._eval(C.c_void_p(out.data_ptr()), out.numel() * out.element_size(), True, out.device.index or 0)
        return out
    if out is not None:
        if out.size != size:
            raise ValueError("out must have same size as the stacked grid.")
        if out.dtype != dtype:
            raise ValueError("out must have same type as grid.")
        if out.flags.c_contiguous:
            host = view = out.reshape(mask.shape)
        else:                                    # filled through a temporary
            host, view = np.empty(mask.shape, dtype), out
    elif not get and "torch" in sys.modules:     # stays on the GPU where the process works with torch (as get_farfield)
        import torch
        t = torch.empty(mask.shape, dtype=getattr(torch, dtype.name), device=torch.device("cuda", int(device)))
        return _raster(mask, dtype, t, get, device)
    else:
        host = view = np.empty(mask.shape, dtype=dtype)
    mask._eval(host.ctypes.data_as(C.c_void_p), host.nbytes, False, device)
    if host is not view:
        view[...] = host.reshape(view.shape)
    return view


def dispatch_read():
    """hgs_poly_dispatch_read: the kernel instances (``poly_kernel``, ``pattern_kernel``) the eager functions launched on this
    thread since the previous call, in the form of ``Engine.dispatch_read``."""
    lib = L.load()
    need = C.c_size_t(0)
    L.check(lib.hgs_poly_dispatch_read(None, 0, C.byref(need)))
    buf = C.create_string_buffer(max(1, need.value))
    L.check(lib.hgs_poly_dispatch_read(buf, len(buf), None))
    return L.parse_dispatch(buf.value.decode())


# ---- Cantor pairing (phase.py:1546-1576) -----------------------------------------------------------------------------
def _inverse_cantor(z):
    z = np.array(z, dtype=np.int64)
    if z.ndim != 1:
        raise ValueError("Expected a list of shape (D,)")
    zz = np.maximum(z, 0)
    w = (np.sqrt(8.0 * zz + 1) - 1) // 2
    w = w.astype(np.int64)
    w = np.where(w * (w + 1) // 2 > zz, w - 1, w)               # (guards the square root's rounding)
    ny = zz - w * (w + 1) // 2
    nx = w - ny
    special = z < 0                                             # negative: a pseudo-term (index, 0)
    return np.stack((np.where(special, z, nx), np.where(special, 0, ny)), axis=1)


# ---- polynomial -----------------------------------------------------------------------------------------------------
def polynomial(grid, weights, terms=None, pathing=None, out=None, *, get=True, lazy=False):
    r"""
    A sum of monomials :math:`\phi(x, y) = \sum_m w_m x^{a_m} y^{b_m}` (phase.py:1672-1795).

    ``weights``: ``(D,)`` or ``(D, N)`` for a stack of N; ``terms``: ``(D, 2)`` exponents, ``(D,)`` Cantor indices, or
    ``None`` for the Cantor indices ``0 .. D-1``.  The pseudo-term ``(-1, 0)`` adds ``w * atan2(y, x)`` where ``w > 0``.
    ``pathing`` does not change the result.  Returns ``(N,) + grid shape`` in the grid's type: a NumPy array; ``out``
    (NumPy array or torch CUDA tensor of that size and type) is filled in place and returned; ``get=False`` returns a
    torch CUDA tensor (NumPy in a process that has not imported torch); ``lazy=True`` returns the ``PolynomialMask``.
    """
    weights = np.array(weights)
    if terms is None:
        terms = np.arange(weights.shape[0] if weights.ndim else 1)
    terms = np.array(terms)
    if terms.ndim == 1:
        terms = _inverse_cantor(terms)
    if terms.ndim != 2 or terms.shape[1] != 2:
        raise ValueError("Terms must be of shape (D, 2) or (D,). Found {}.".format(terms.shape))
    D = terms.shape[0]
    if weights.ndim == 1:
        if len(weights) != D:
            raise ValueError("Expected weights to have a common dimension with indices.")
        weights = np.reshape(weights, (-1, 1))
    elif weights.ndim == 2:
        if weights.shape[0] != D:
            raise ValueError("Expected weights to have a common dimension with indices.")
    else:
        raise ValueError("Expected weights to be 1D or 2D.")
    mask = PolynomialMask(_prepared(grid), terms, weights)
    return mask if lazy else mask.raster(out=out, get=get)


# ---- Zernike --------------------------------------------------------------------------------------------------------
def zernike_aperture(grid, aperture=None):
    """
    ``(x_scale, y_scale)`` between the grid's units and the unit pupil (phase.py:683-780): ``"circular"``,
    ``"elliptical"``, ``"cropped"``, a scalar, a pair, or ``None`` -- the SLM's ``get_source_zernike_scaling()`` when
    ``grid`` is an SLM (or a cameraslm), ``"cropped"`` otherwise.
    """
    x_grid, y_grid = toolbox.process_grid(grid)
    if aperture is None:
        grid = _hardware(grid)
        aperture = grid.get_source_zernike_scaling() if hasattr(grid, "get_source_zernike_scaling") else "cropped"
    if isinstance(aperture, str):
        if aperture == "elliptical":
            return 1 / np.nanmax(x_grid), 1 / np.nanmax(y_grid)
        if aperture == "circular":
            scale = 1 / np.amin([np.nanmax(x_grid), np.nanmax(y_grid)])
            return scale, scale
        if aperture == "cropped":
            scale = 1 / np.sqrt(np.nanmax(np.square(x_grid) + np.square(y_grid)))
            return scale, scale
        raise ValueError(f"Aperture '{aperture}' is not implemented.")
    if np.isscalar(aperture):
        return aperture, aperture
    if isinstance(aperture, (list, tuple, np.ndarray)) and len(aperture) == 2:
        return aperture[0], aperture[1]
    raise ValueError("Aperture type {} not recognized.".format(type(aperture)))


def _indices_parse(indices, D):
    """The default basis [2, 1, 4, 3, 5, ...] and the size checks of phase._zernike_indices_parse (phase.py:923-961)."""
    if np.isscalar(indices):
        if D is not None and D != int(indices):
            raise ValueError(f"Expected data (dimension {D}) to have common size with indices (requested {int(indices)}).")
        D, indices = int(indices), None
    return toolbox.zernike_indices_parse(indices, D)


def _falling(p, k):
    """p (p - 1) ... (p - k + 1): the factor the k-th derivative of x^p carries; 0 for p < k."""
    out = 1
    for i in range(k):
        out *= p - i
    return out


def _zernike_terms(indices, weights, derivative=(0, 0)):
    """
    (terms (M, 2), weights (M, N)) of the monomials whose sum is ``d^dx/dx d^dy/dy sum_d weights[d] Z_indices[d]``: the
    power rule applied to the integer coefficients before anything is rastered (phase._zernike_get_cantor,
    phase.py:850-920).  Negative indices follow as pseudo-terms (index, 0) with their own weights, untouched.
    """
    dx, dy = int(derivative[0]), int(derivative[1])
    acc, special = {}, []
    for d, idx in enumerate(indices):
        if int(idx) < 0:
            special.append(((int(idx), 0), weights[d]))
            continue
        for (px, py), c in toolbox.zernike_cartesian(int(idx)).items():
            c = c * _falling(px, dx) * _falling(py, dy)
            if c != 0:
                key = (px - dx, py - dy)
                acc[key] = acc.get(key, 0) + c * weights[d]
    keys = sorted(acc, key=lambda k: (k[0] + k[1]) * (k[0] + k[1] + 1) // 2 + k[1])
    terms = keys + [k for k, _ in special]
    rows = [acc[k] for k in keys] + [w for _, w in special]
    N = weights.shape[1]
    return np.array(terms, dtype=np.int64).reshape(-1, 2), np.array(rows, dtype=np.float64).reshape(len(terms), N)


def zernike_sum(grid, indices, weights, aperture=None, use_mask=True, derivative=(0, 0), out=None, *, get=True, lazy=False):
    r"""
    :math:`\phi = \sum_k w_k Z_{J_k}`, ANSI ``indices`` (``None``: the basis ``[2, 1, 4, 3, 5, ...]`` of the weights'
    length), ``weights`` ``(D,)`` or ``(D, N)`` (phase.py:964-1166).  ``aperture``: see :func:`zernike_aperture`.
    ``use_mask``: ``True`` zeroes the values outside the unit pupil, ``np.nan`` writes NaN there, ``False`` leaves the
    polynomial uncropped, ``"return"`` returns the boolean pupil ``square(x s_x) + square(y s_y) <= 1`` itself (formed on
    the host, in the reference's expression).  ``derivative``: ``(dx, dy)`` orders, by power rule on the coefficients.
    Returns the grid's shape (N = 1) or ``(N,) + shape``; ``out``, ``get`` and ``lazy`` as in :func:`polynomial`.
    """
    grid = _prepared(grid)
    x, y = grid.grid
    x_scale, y_scale = zernike_aperture(grid, aperture)
    if len(derivative) != 2:
        raise ValueError("Expected derivative to be a (int, int)")
    weights = np.squeeze(weights)
    if weights.ndim <= 1:
        if weights.ndim == 0:
            weights = np.array([weights])
        D = None
        if indices is not None:
            indices = np.squeeze(indices)
            if indices.ndim == 0:
                indices = np.array([indices])
            D = len(indices)
        if D is not None and len(weights) != D:
            raise ValueError("Expected weights to have a common dimension with indices.")
        weights = np.reshape(weights, (-1, 1))
    elif weights.ndim != 2:
        raise ValueError("Expected weights to be 1D or 2D.")
    D, N = weights.shape
    indices = _indices_parse(indices, D)
    mode = L.POLY_MASK_NONE
    if use_mask is not False:
        sx, sy = np.asarray(x_scale, dtype=x.dtype)[()], np.asarray(y_scale, dtype=x.dtype)[()]
        if isinstance(use_mask, str):
            if use_mask == "return":
                return np.square(x * sx) + np.square(y * sy) <= 1
            raise ValueError(f"use_mask '{use_mask}' is not recognized.")
        if np.isnan(use_mask):
            mode = L.POLY_MASK_NAN
        elif use_mask:
            mode = L.POLY_MASK_ZERO
    terms, mono = _zernike_terms(indices, np.asarray(weights, dtype=np.float64), derivative)
    mask = PolynomialMask(grid, terms, mono, x_scale, y_scale, mode, squeeze=True)
    return mask if lazy else mask.raster(out=out, get=get)


def zernike(grid, index, weight=1, **kwargs):
    """One Zernike polynomial: ``zernike_sum`` with a single term (phase.py:783-814)."""
    return zernike_sum(grid, (int(index),), (float(weight),), **kwargs)


# ---- blaze and lens: polynomials --------------------------------------------------------------------------------------
def blaze(grid, vector=(0, 0), out=None, *, get=True, lazy=False):
    r"""
    A blazed grating :math:`\phi = 2\pi (v_x x + v_y y)`, plus :math:`\pi v_z (x^2 + y^2)` for a 3-vector (phase.py:37-75).
    A polynomial: ``lazy=True`` returns a ``PolynomialMask``; ``out`` and ``get`` as in :func:`polynomial`.
    """
    terms, weights = [(1, 0), (0, 1)], [2 * np.pi * vector[0], 2 * np.pi * vector[1]]
    if len(vector) > 2:
        terms, weights = terms + [(2, 0), (0, 2)], weights + [np.pi * vector[2]] * 2
    mask = PolynomialMask(_prepared(grid), terms, np.reshape(np.asarray(weights, dtype=np.float64), (-1, 1)), squeeze=True)
    return mask if lazy else mask.raster(out=out, get=get)


def _parse_focal_length(f):
    """(fx, fy) as float64: a scalar counts for both; a list holds two terms, none of them zero (phase.py:394-406)."""
    if isinstance(f, toolbox.REAL_TYPES):
        f = [f, f]
    if not isinstance(f, (list, tuple, np.ndarray)):
        raise ValueError("Expected a focal length or a list of two. Found {}.".format(f))
    f = np.squeeze(np.asarray(f, dtype=np.float64))
    if f.size != 2:
        raise ValueError("Expected two terms in focal list. Found {}.".format(f))
    if np.any(f == 0):
        raise ValueError("Cannot interpret a focal length of zero. Found {}.".format(f))
    return f.reshape(2)


def lens(grid, f=(np.inf, np.inf), out=None, *, get=True, lazy=False):
    r"""
    A thin parabolic lens :math:`\phi = \pi (x^2 / f_x + y^2 / f_y)` (phase.py:409-452); ``f`` a scalar or a pair, an infinite
    component contributes nothing (the other one still does).  A polynomial, as :func:`blaze`.
    """
    f = _parse_focal_length(f)
    mask = PolynomialMask(_prepared(grid), [(2, 0), (0, 2)], np.reshape(np.pi / f, (2, 1)), squeeze=True)
    return mask if lazy else mask.raster(out=out, get=get)


# ---- gratings, axicon and Gaussian modes: pattern_kernel -----------------------------------------------------------------------
_F64 = np.dtype(np.float64)
_MODE_NAMES = ("blaze", "sinusoid", "binary", "axicon", "laguerre_gaussian", "hermite_gaussian")


class PatternMask:
    """
    One grating, axicon or Gaussian-mode mask over a grid, not yet rastered: ``mode`` (``_lib.PATTERN_*``), ``quad`` (four
    windows, each with its own vector), ``vectors`` (eight numbers), ``shift``, ``a``, ``b``, ``duty``, ``radius``, the
    orders ``l``, ``p``, ``n``, ``m``, and the coordinates as in ``PolynomialMask``.  ``dtype`` is the grid's type,
    ``out_dtype`` the type of the values (``cast``: the type the host converts them to where the kernel has none, int64 for
    a binary grating between two ints).  Immutable; ``fingerprint`` identifies the content.  The contract of
    ``PolynomialMask``: ``raster``, ``np.asarray(mask)``, and the consumers that take one in place of an array.
    """

    __slots__ = ("shape", "grid_shape", "stack", "dtype", "out_dtype", "cast", "mode", "quad", "vectors", "shift", "a", "b",
                 "duty", "radius", "l", "p", "n", "m", "round_grid", "decision_double", "axes", "grids", "fingerprint")

    def __init__(self, grid, mode, vectors=(0.0, 0.0), quad=False, shift=0.0, a=np.pi, b=0.0, duty=0.5, radius=1.0,
                 l=0, p=0, n=0, m=0, out_dtype=None, cast=None, decision_double=False):
        vec = [float(v) for v in np.ravel(np.asarray(vectors, dtype=np.float64))]
        if len(vec) != (8 if quad else 2):
            raise ValueError(f"Expected {'four 2-vectors' if quad else 'one 2-vector'}. Found {np.shape(vectors)}.")
        if quad and len(grid.shape) != 2:
            raise ValueError(f"Quadrants need a 2-D grid. Found shape {grid.shape}.")
        for order in (p, n, m):
            if order < 0:
                raise ValueError(f"Polynomial order {order} must not be negative.")
            if order > L.PATTERN_MAX_ORDER:
                raise NotImplementedError(f"pattern mask: order {order} is beyond the limit of {L.PATTERN_MAX_ORDER}")
        out_dtype = grid.dtype if out_dtype is None else np.dtype(out_dtype)
        put = object.__setattr__
        put(self, "dtype", grid.dtype)
        put(self, "grid_shape", grid.shape)
        put(self, "shape", grid.shape)
        put(self, "stack", 1)
        put(self, "out_dtype", out_dtype)
        put(self, "cast", None if cast is None else np.dtype(cast))
        put(self, "mode", int(mode))
        put(self, "quad", bool(quad))
        put(self, "vectors", tuple(vec + [0.0] * (8 - len(vec))))
        for name, value in (("shift", shift), ("a", a), ("b", b), ("duty", duty), ("radius", radius)):
            put(self, name, float(value))
        for name, value in (("l", l), ("p", p), ("n", n), ("m", m)):
            put(self, name, int(value))
        put(self, "round_grid", out_dtype == grid.dtype)          # (else the values keep the double they were formed in)
        put(self, "decision_double", bool(decision_double))
        put(self, "axes", grid.axes)
        put(self, "grids", None if grid.axes is not None else grid.grid)
        h = grid._hash.copy()                      # (the coordinates are in it already)
        h.update(repr(("pattern", self.mode, self.quad, self.vectors, self.shift, self.a, self.b, self.duty, self.radius, self.l,
                       self.p, self.n, self.m, out_dtype.str, None if cast is None else self.cast.str, self.decision_double)).encode())
        put(self, "fingerprint", h.hexdigest())

    def __setattr__(self, name, value):
        raise AttributeError("PatternMask is immutable")

    def __repr__(self):
        return (f"PatternMask({_MODE_NAMES[self.mode]}{', quadrants' if self.quad else ''}, shape={self.shape}, "
                f"dtype={self.dtype.name}, {'product' if self.axes is not None else 'full'} grid, "
                f"fingerprint={self.fingerprint[:12]})")

    def params(self, out_bytes=0, device=0):
        """(hgs_pattern_params, the arrays it points into -- keep them until the call returned)."""
        h, w = _raster_shape(self.grid_shape)
        keep = [self.axes, self.grids]
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        ax, gr = self.axes or (None, None), self.grids or (None, None)
        prm = L.hgs_pattern_params(h=h, w=w, grid_bytes=self.dtype.itemsize, out_bytes=int(out_bytes), device=int(device),
                                   mode=self.mode, quad=int(self.quad), round_grid=int(self.round_grid),
                                   decision_double=int(self.decision_double), l=self.l, p=self.p, n=self.n, m=self.m,
                                   vec=(C.c_double * 8)(*self.vectors), shift=self.shift, a=self.a, b=self.b, duty=self.duty,
                                   radius=self.radius, x_axis=ptr(ax[0]), y_axis=ptr(ax[1]), x_grid=ptr(gr[0]), y_grid=ptr(gr[1]))
        return prm, keep

    def _eval(self, pointer, nbytes, on_device, device):
        prm, keep = self.params(out_bytes=self.out_dtype.itemsize, device=device)
        L.check(L.load().hgs_pattern_eval(C.byref(prm), pointer, nbytes, int(on_device)))

    def raster(self, out=None, get=True, device=0):
        """The mask as its function returns it: ``out_dtype`` values (see ``out`` and ``get`` of :func:`polynomial`); a mask
        with a ``cast`` is converted on the host and comes as a NumPy array."""
        if self.cast is None:
            return _raster(self, self.out_dtype, out, get, device)
        if out is not None and (_is_device_tensor(out) or out.dtype != self.cast):
            raise ValueError(f"out must be a NumPy array of type {self.cast.name}.")
        values = _raster(self, self.out_dtype, None, True, device).astype(self.cast)
        if out is None:
            return values
        if out.size != values.size:
            raise ValueError("out must have same size as the stacked grid.")
        out[...] = values.reshape(out.shape)
        return out

    def __array__(self, dtype=None, copy=None):
        a = self.raster()
        return a if dtype is None else a.astype(dtype, copy=False)


def _finish(mask, out, get, lazy):
    return mask if lazy else mask.raster(out=out, get=get)


def _vector2(vector):
    """The two components of a grating's vector, and whether NumPy would form the grating's products in double on a float32
    grid: float64 scalars do not give way to the array's type as Python numbers do."""
    if len(vector) != 2:
        raise ValueError("Expected a 2-vector. Found {}.".format(vector))
    strong = [v for v in (vector[0], vector[1]) if isinstance(v, np.generic)]
    return (float(vector[0]), float(vector[1])), bool(strong) and np.result_type(np.float32, *strong) == _F64


def sinusoid(grid, vector=(0, 0), shift=0, a=np.pi, b=0, out=None, *, get=True, lazy=False):
    r"""
    A sinusoidal grating :math:`\phi = \frac{a - b}{2} [1 + \sin(2\pi \vec k \cdot \vec x + s)] + b` (phase.py:78-128; the
    reference's code uses the sine too, its docstring says cosine).  ``lazy=True`` returns a ``PatternMask``.
    """
    vec, _ = _vector2(vector)
    return _finish(PatternMask(_prepared(grid), L.PATTERN_SINUSOID, vec, shift=shift, a=a, b=b), out, get, lazy)


def _binary_types(grid, vec, a, b):
    """(out_dtype, cast) of a binary grating: ``np.where(cond, a, b)``'s type -- float64 for Python floats whatever the
    grid's, int64 for two ints -- and the grid's type for a zero vector, which the reference fills a grid-typed array with."""
    if vec[0] == 0 and vec[1] == 0:
        return grid.dtype, None
    kind = np.result_type(a, b)
    if kind in (np.dtype(np.float32), _F64):
        return kind, None
    return _F64, kind


def binary(grid, vector=(0, 0), shift=0, a=np.pi, b=0, duty_cycle=.5, out=None, *, get=True, lazy=False):
    r"""
    A binary grating (phase.py:131-258): ``a`` where :math:`[2\pi \vec k \cdot \vec x + s] \bmod 2\pi` lies in the last
    ``duty_cycle`` (clipped to [0, 1]) of the period, else ``b``.  A vector with a component above 1 in magnitude is a period
    in pixels: the coordinates become the pixel indices and each component its reciprocal.  A zero vector gives ``b``
    everywhere, or ``a`` when ``shift != 0`` and ``mod(shift, 2 pi) > 2 pi duty_cycle``.  The set of pixels that receive
    ``a`` is the reference's: the decision is formed with NumPy's roundings.  The result has the type of
    ``np.where(cond, a, b)`` (float64 for Python floats, int64 for two ints), the grid's for a zero vector.
    """
    grid = _prepared(grid)
    vec, strong = _vector2(vector)
    out_dtype, cast = _binary_types(grid, vec, a, b)
    mask = PatternMask(grid, L.PATTERN_BINARY, vec, shift=shift, a=a, b=b, duty=np.clip(float(duty_cycle), 0, 1),
                       out_dtype=out_dtype, cast=cast, decision_double=strong)
    return _finish(mask, out, get, lazy)


def _quadrants(grid, vectors, grating, out, get, lazy):
    """Four 2-vectors (2, 4) in top-right, bottom-right, top-left, bottom-left order, each filling its window with ``grating``
    (phase.py:261-295).  The windows start at row ``H // 2`` and column ``W // 2``; their ends are clipped to ``H - 1`` and
    ``W - 1`` as the reference's ``window_slice`` clips them, so the last row and the last column stay 0 for an even side
    as for an odd one.  The vectors are float64 scalars to NumPy."""
    vectors = toolbox.format_2vectors(vectors)
    if vectors.shape != (2, 4):
        raise ValueError("Expected four 2-vectors (2,4). Found {}.".format(vectors.shape))
    modes = {blaze: L.PATTERN_BLAZE, sinusoid: L.PATTERN_SINUSOID, binary: L.PATTERN_BINARY}
    if grating not in modes:
        raise TypeError("grating must be this module's binary, blaze or sinusoid. Found {}.".format(grating))
    mask = PatternMask(_prepared(grid), modes[grating], vectors.T, quad=True, decision_double=True)
    return _finish(mask, out, get, lazy)


def bahtinov(grid, radius=.001, angle=10 * np.pi / 180, grating=binary, out=None, *, get=True, lazy=False):
    """
    A Bahtinov mask (phase.py:298-344): the right two quadrants hold gratings toward ``radius (sin a, +-cos a)``, the left
    two toward ``radius (0, 1)``.  ``grating``: this module's :func:`binary`, :func:`blaze` or :func:`sinusoid` with their
    default arguments (anything else raises ``TypeError``).  The last row and the last column stay 0, as in the reference.
    """
    s, c = np.sin(angle), np.cos(angle)
    return _quadrants(grid, radius * np.array([(s, c), (s, -c), (0, 1), (0, 1)]).T, grating, out, get, lazy)


def quadrants(grid, radius=.001, center=(0, 0), out=None, *, get=True, lazy=False):
    """
    A quadrant alignment mask (phase.py:347-389): each quadrant blazes toward its own corner,
    ``radius / sqrt(2) (+-1, +-1) + center``.  The last row and the last column stay 0, as in the reference.
    """
    vectors = toolbox.format_2vectors((radius / np.sqrt(2)) * np.array([(1, -1), (1, 1), (-1, -1), (-1, 1)]).T)
    return _quadrants(grid, vectors + toolbox.format_2vectors(center), blaze, out, get, lazy)


def _source_radius(grid, w=None):
    """The source radius ``w`` (phase.py:1800-1839) over the prepared ``grid``: given; else the SLM's
    ``get_source_radius()``; else a quarter of the smaller of the grid's two largest coordinates."""
    if w is not None:
        return w
    if hasattr(grid.hardware, "get_source_radius"):
        return grid.hardware.get_source_radius()
    return grid.radius


def axicon(grid, f=(np.inf, np.inf), w=None, out=None, *, get=True, lazy=False):
    r"""
    An axicon (phase.py:455-498): with :math:`\vec k = w / \vec f / 2`, :math:`\phi = 2\pi \sqrt{(x k_x)^2 + (y k_y)^2}`;
    :math:`2\pi k |x|` or :math:`2\pi k |y|` where the other component vanishes (an infinite focal length).  float64 for
    either grid type, as NumPy forms it; zeros of the grid's type where both vanish.
    """
    prepared = _prepared(grid)
    w = _source_radius(prepared, w)
    f = _parse_focal_length(f)
    k = (float(w / f[0] / 2), float(w / f[1] / 2))
    mask = PatternMask(prepared, L.PATTERN_AXICON, k, out_dtype=prepared.dtype if k == (0.0, 0.0) else _F64)
    return _finish(mask, out, get, lazy)


def laguerre_gaussian(grid, l, p=0, w=None, out=None, *, get=True, lazy=False):
    r"""
    The phase of a Laguerre-Gauss mode (phase.py:1842-1894): :math:`l\,\mathrm{atan2}(x, y) + \pi [L_p^{|l|}(16 r^2 / w^2) < 0]`
    -- note the argument order of the angle --, each term only for ``l != 0`` and ``p != 0``.  ``w``: the source radius
    (:func:`axicon`).  The grid's type with ``l != 0``, float64 for the rings alone; ``l = p = 0`` gives zeros.
    """
    prepared = _prepared(grid)
    l, p = int(l), int(p)
    w = _source_radius(prepared, w) if p != 0 else 1.0
    mask = PatternMask(prepared, L.PATTERN_LG, l=l, p=p, radius=w, out_dtype=_F64 if l == 0 and p != 0 else prepared.dtype)
    return _finish(mask, out, get, lazy)


def hermite_gaussian(grid, n, m, w=None, out=None, *, get=True, lazy=False):
    r"""
    The phase of a Hermite-Gauss mode (phase.py:1897-1935): :math:`\pi` where :math:`H_n(4x / w) H_m(4y / w) > 0`, else 0
    (``n = m = 0``: :math:`\pi` everywhere, as the reference returns it).  float64 for either grid type.
    """
    prepared = _prepared(grid)
    w = _source_radius(prepared, w)
    return _finish(PatternMask(prepared, L.PATTERN_HG, n=int(n), m=int(m), radius=w, out_dtype=_F64), out, get, lazy)


def ince_gaussian(grid, p, m, parity=1, ellipticity=1, w=None):
    """Not implemented, as in the reference (phase.py:1938-1992)."""
    raise NotImplementedError("ince_gaussian is not implemented (nor is it in the reference).")


def matheui_gaussian(grid, r, q, w=None):
    """Not implemented, as in the reference (phase.py:1995-2008)."""
    raise NotImplementedError("matheui_gaussian is not implemented (nor is it in the reference).")


def airy(grid, f=(np.inf, np.inf)):
    """Not implemented, as in the reference (phase.py:2011-)."""
    raise NotImplementedError("airy is not implemented (nor is it in the reference).")
