"""
The recorded cases of tests/golden/phase_*.npz (tools/make_golden_phase.py) and how a test repeats the recorded call on
``slmsuite_amd.holography.toolbox.phase``.  Shared by tests/test_phase_cpu.py and tests/test_phase_gpu.py.
"""
import functools
import json
import os

import numpy as np

from conftest import GOLDEN

FILES = ("phase_prod_true", "phase_prod_false", "phase_prod_nan", "phase_stack", "phase_rot", "phase_deriv", "phase_poly",
         "phase_order10", "phase_tiny")


@functools.lru_cache(maxsize=None)
def load_file(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    cases = {}
    for key in z.files:
        case, _, arr = key.partition("/")
        cases.setdefault(case, {})[arr] = z[key]
    for c in cases.values():
        c["call"] = json.loads(str(c["call"]))
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)          # shared among the tests: nobody edits a reference
    return cases


def case_ids():
    return [f"{f[6:]}/{c}" for f in FILES for c in load_file(f)]


def get_case(case_id):
    f, c = case_id.split("/")
    return load_file("phase_" + f)[c]


class SlmGrid:
    """aperture=None on an SLM: its grids and the scaling it reports."""

    def __init__(self, x, y, scaling):
        self.grid = (x, y)
        self._scaling = scaling

    def get_source_zernike_scaling(self):
        return self._scaling


def grids(case, dtype):
    return np.ascontiguousarray(case["x"], dtype=dtype), np.ascontiguousarray(case["y"], dtype=dtype)


def call(phase, case, dtype, use_mask=None, **kw):
    """The recorded call on ``phase`` for a ``dtype`` grid (float32: the weights cast too, as the tool did); ``use_mask``
    overrides the recorded one ("return"); ``kw`` goes on (out, get, lazy)."""
    x, y = grids(case, dtype)
    w = np.asarray(case["weights"], dtype=dtype)
    c = case["call"]
    if c["kind"] == "polynomial":
        return phase.polynomial((x, y), w, case["terms"], **kw)
    ap = c["aperture"]
    grid = SlmGrid(x, y, float(case["slm_scaling"])) if ap == "slm" else (x, y)
    ap = None if ap == "slm" else tuple(ap) if isinstance(ap, list) else ap
    um = {"True": True, "False": False, "nan": np.nan}[c["use_mask"]] if use_mask is None else use_mask
    return phase.zernike_sum(grid, c["indices"], w, ap, um, tuple(c["derivative"]), **kw)


def table_eval(mask):
    """A PolynomialMask's triangle summed with NumPy in float64 over its own coordinates, unmasked: ``(N,) + grid shape``.
    The vortex plate is added where its weight is positive."""
    if mask.axes is not None:
        x, y = np.meshgrid(mask.axes[0].astype(np.float64), mask.axes[1].astype(np.float64))
    else:
        x, y = (g.astype(np.float64) for g in mask.grids)
    xs, ys = x * mask.x_scale, y * mask.y_scale
    out = np.zeros((mask.stack,) + x.shape)
    row = 0
    for b in range(mask.degree + 1):
        for a in range(mask.degree - b + 1):
            out += mask.table[:, row + a].reshape(-1, 1, 1) * (xs ** a * ys ** b)
        row += mask.degree - b + 1
    if mask.vortex is not None:
        out += mask.vortex.reshape(-1, 1, 1) * np.arctan2(ys, xs)
    return out
