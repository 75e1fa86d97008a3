"""
Phase masks formed on the GPU: ``polynomial``, ``zernike_sum``, ``zernike`` and ``zernike_aperture`` with the signatures
and argument handling of the reference's ``toolbox.phase`` (phase.py:683-1166, :1672-1795).

The host only parses: terms and weights are folded into a dense triangle of monomial coefficients (``PolynomialMask``)
and ``hgs_poly_eval`` rasters it -- Horner's scheme in double for either grid type, one rounding to the grid's type
(include/hgs.h, csrc/poly_kernels.hpp).  There is no CPU route: without a GPU the functions raise ``HgsError``; only
``lazy=True``, ``use_mask="return"`` and ``zernike_aperture`` need none.

Where this differs from the reference on purpose:

* float32 grids are evaluated in double from the widened coordinates and rounded once, and the monomial coefficients are
  not rounded to float32 first; the reference multiplies float32 arrays.  The result is the closer one to exact.
* ``polynomial(terms=None)`` takes the Cantor indices ``0 .. D-1`` as the reference documents (its code raises there).
* ``pathing`` is accepted and ignored: the order of evaluation is Horner's.
"""
import ctypes as C
import hashlib
import sys

import numpy as np

from slmsuite_amd import _lib as L
from slmsuite_amd.holography import toolbox

__all__ = ["PolynomialMask", "polynomial", "zernike", "zernike_sum", "zernike_aperture"]


# ---- grids --------------------------------------------------------------------------------------------------------
def _grids(grid):
    """(x_grid, y_grid) as float32 / float64 arrays of one shape and one type."""
    x, y = toolbox.process_grid(grid)
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape:
        raise ValueError(f"x_grid {x.shape} and y_grid {y.shape} differ in shape")
    dt = np.result_type(x.dtype, y.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        dt = np.dtype(np.float64)
    return np.ascontiguousarray(x, dtype=dt), np.ascontiguousarray(y, dtype=dt)


def _raster_shape(shape):
    """(H, W) the kernel walks for a grid of ``shape``: the grid itself when 2-D, one row of all its values otherwise."""
    if len(shape) == 2:
        return int(shape[0]), int(shape[1])
    return 1, int(np.prod(shape, dtype=np.int64))


def _product_axes(x, y):
    """(x[W], y[H]) when x varies along the last axis only and y along the first only, else None."""
    if x.ndim != 2 or x.size == 0:
        return None
    if np.array_equal(x, np.broadcast_to(x[:1, :], x.shape)) and np.array_equal(y, np.broadcast_to(y[:, :1], y.shape)):
        return x[0, :].copy(), y[:, 0].copy()
    return None


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

    def __init__(self, x, y, terms, weights, x_scale=1.0, y_scale=1.0, mask_mode=L.POLY_MASK_NONE, squeeze=False):
        terms = np.asarray(terms, dtype=np.int64).reshape(-1, 2)
        weights = np.asarray(weights, dtype=np.float64)
        degree, table, vortex = _fold_terms(terms, weights)
        put = object.__setattr__
        put(self, "dtype", x.dtype)
        put(self, "grid_shape", tuple(x.shape))
        put(self, "stack", int(weights.shape[1]))
        put(self, "_squeeze", bool(squeeze) and weights.shape[1] == 1)
        put(self, "shape", self.grid_shape if self._squeeze else (self.stack,) + self.grid_shape)
        put(self, "degree", degree)
        put(self, "mask_mode", int(mask_mode))
        # the scales meet the grid in its type (NumPy: a Python float times a float32 array is a float32 product)
        put(self, "x_scale", float(np.asarray(x_scale, dtype=x.dtype)))
        put(self, "y_scale", float(np.asarray(y_scale, dtype=x.dtype)))
        axes = _product_axes(x, y)
        put(self, "axes", axes)
        grids = None if axes is not None else (x.copy(), y.copy())     # (its own: the caller may go on editing the grid)
        put(self, "grids", grids)
        h = hashlib.sha1(repr((self.dtype.str, self.grid_shape, self.stack, degree, self.mask_mode, self.x_scale, self.y_scale,
                               self._squeeze, axes is not None)).encode())
        for a in (table, vortex) + (axes if axes is not None else grids):
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

    def raster(self, out=None, get=True, device=0):
        """The masks, as ``polynomial`` / ``zernike_sum`` return them (see their ``out`` and ``get``)."""
        lib = L.load()
        if out is not None and _is_device_tensor(out):
            if out.numel() != int(np.prod(self.shape, dtype=np.int64)):
                raise ValueError("out must have same size as the stacked grid.")
            if str(out.dtype).split(".")[-1] != self.dtype.name:
                raise ValueError("out must have same type as grid.")
            if not out.is_contiguous():
                raise ValueError("out must be contiguous.")
            _wait_for_torch(out)
            prm, keep = self.params(device=out.device.index or 0)
            L.check(lib.hgs_poly_eval(C.byref(prm), C.c_void_p(out.data_ptr()), out.numel() * out.element_size(), 1))
            return out
        if out is not None:
            if out.size != int(np.prod(self.shape, dtype=np.int64)):
                raise ValueError("out must have same size as the stacked grid.")
            if out.dtype != self.dtype:
                raise ValueError("out must have same type as grid.")
            if out.flags.c_contiguous:
                host = view = out.reshape(self.shape)
            else:                                    # filled through a temporary
                host, view = np.empty(self.shape, self.dtype), out
        elif not get and "torch" in sys.modules:     # stays on the GPU where the process works with torch (as get_farfield)
            import torch
            t = torch.empty(self.shape, dtype=getattr(torch, self.dtype.name), device=torch.device("cuda", int(device)))
            return self.raster(out=t)
        else:
            host = view = np.empty(self.shape, dtype=self.dtype)
        prm, keep = self.params(device=device)
        L.check(lib.hgs_poly_eval(C.byref(prm), host.ctypes.data_as(C.c_void_p), host.nbytes, 0))
        if host is not view:
            view[...] = host.reshape(view.shape)
        return view

    def __array__(self, dtype=None, copy=None):
        a = self.raster()
        return a if dtype is None else a.astype(dtype, copy=False)


def _is_device_tensor(value):
    return type(value).__module__.split(".")[0] == "torch" and bool(getattr(value, "is_cuda", False))


def _wait_for_torch(tensor):
    """The library writes on its own stream: what torch still has in flight for this block must have landed first."""
    sys.modules["torch"].cuda.current_stream(tensor.device).synchronize()


def dispatch_read():
    """hgs_poly_dispatch_read: the kernel instances the eager functions launched on this thread since the previous call,
    in the form of ``Engine.dispatch_read``."""
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
    x, y = _grids(grid)
    mask = PolynomialMask(x, y, terms, weights)
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
        if hasattr(grid, "slm") and hasattr(grid, "cam"):
            grid = grid.slm
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
    x, y = _grids(grid)
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
    mask = PolynomialMask(x, y, terms, mono, x_scale, y_scale, mode, squeeze=True)
    return mask if lazy else mask.raster(out=out, get=get)


def zernike(grid, index, weight=1, **kwargs):
    """One Zernike polynomial: ``zernike_sum`` with a single term (phase.py:783-814)."""
    return zernike_sum(grid, (int(index),), (float(weight),), **kwargs)
