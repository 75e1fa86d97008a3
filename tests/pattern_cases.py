"""
The recorded cases of tests/golden/pattern_*.npz (tools/make_golden_patterns.py) and how a test repeats the recorded call on
``slmsuite_amd.holography.toolbox.phase``.  Shared by tests/test_patterns_cpu.py and tests/test_patterns_gpu.py.
"""
import functools
import json
import os

import numpy as np

from conftest import GOLDEN

FUNCTIONS = ("blaze", "sinusoid", "binary", "lens", "axicon", "laguerre_gaussian", "hermite_gaussian", "quadrants", "bahtinov")
GRIDS = ("slm", "odd", "rot", "tiny35", "tiny11")
PRODUCT = {"slm": True, "odd": True, "rot": False, "tiny35": True, "tiny11": True}
POLYNOMIAL = ("blaze", "lens")
MODE = {"sinusoid": 1, "binary": 2, "axicon": 3, "laguerre_gaussian": 4, "hermite_gaussian": 5}      # (_lib.PATTERN_*)


@functools.lru_cache(maxsize=None)
def _grids():
    z = np.load(os.path.join(GOLDEN, "pattern_grids.npz"), allow_pickle=False)
    return {g: (z[f"{g}/x"], z[f"{g}/y"]) for g in GRIDS}


def grid(name, dtype):
    x, y = _grids()[name]
    return np.ascontiguousarray(x, dtype=dtype), np.ascontiguousarray(y, dtype=dtype)


@functools.lru_cache(maxsize=None)
def load_file(fn):
    z = np.load(os.path.join(GOLDEN, f"pattern_{fn}.npz"), allow_pickle=False)
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


def case_ids(fn=None, grid_name=None):
    """``<function>/<case>@<grid>`` of every recorded case, of one function, on one grid."""
    out = [f"{f}/{c}" for f in FUNCTIONS if fn in (None, f) for c in load_file(f)]
    return [c for c in out if grid_name is None or c.endswith("@" + grid_name)]


def get_case(case_id):
    fn, c = case_id.split("/")
    return load_file(fn)[c]


def kwargs_of(phase, case):
    kw = dict(case["call"]["kwargs"])
    if isinstance(kw.get("f"), list):
        kw["f"] = tuple(np.inf if v == "inf" else v for v in kw["f"])
    if "grating" in kw:
        kw["grating"] = getattr(phase, kw["grating"])
    for k in ("vector", "center"):
        if k in kw:
            kw[k] = tuple(kw[k])
    return kw


def call(phase, case, dtype, prepare=False, **kw):
    """The recorded call on ``phase`` for a ``dtype`` grid; ``prepare``: through ``prepare_grid``; ``kw`` goes on."""
    g = grid(case["call"]["grid"], dtype)
    return getattr(phase, case["call"]["fn"])(phase.prepare_grid(g) if prepare else g, **kwargs_of(phase, case), **kw)


def reference(case, dtype):
    return case["ref64" if np.dtype(dtype) == np.float64 else "ref32"]


def result_dtype(case, dtype):
    """The type the call returns for a ``dtype`` grid: the fixture's, but the grid's for the polynomials."""
    return np.dtype(dtype) if case["call"]["fn"] in POLYNOMIAL else reference(case, dtype).dtype


def is_threshold(case):
    """A step decides the value (array equality outside the marginal set); else the values are continuous (relative L2)."""
    fn, kw = case["call"]["fn"], case["call"]["kwargs"]
    return (fn in ("binary", "hermite_gaussian") or (fn == "laguerre_gaussian" and kw["p"] != 0)
            or (fn == "bahtinov" and kw["grating"] == "binary"))


def marginal(case):
    """The pixels no test compares: 0 < |q| <= 1e-9 max|q|; for binary | |d| - 1e-8 | <= 1e-9, the edge of isclose(d, 0)."""
    q = case.get("q")
    if q is None:
        return np.zeros(case["ref64"].shape, dtype=bool)
    if case["call"]["fn"] in ("binary", "bahtinov"):
        return np.abs(np.abs(q) - 1e-8) <= 1e-9
    return (q != 0) & (np.abs(q) <= 1e-9 * np.abs(q).max())


def expected_launch(case, dtype):
    """(kernel family, template arguments as the dispatch record spells them, flags) of the recorded call."""
    fn = case["call"]["fn"]
    g = np.dtype(dtype)
    args = {"R": {4: "float", 8: "double"}[g.itemsize], "PROD": "true" if PRODUCT[case["call"]["grid"]] else "false"}
    out = result_dtype(case, dtype)
    args["OUT_BYTES"] = str(out.itemsize if out.kind == "f" else 8)          # (integers are converted on the host from double)
    if fn in POLYNOMIAL:
        return "poly_kernel", args, set()
    if fn in ("quadrants", "bahtinov"):
        grating = case["call"]["kwargs"].get("grating", "blaze")
        args["MODE"] = str({"blaze": 0, "sinusoid": 1, "binary": 2}[grating])
        return "pattern_kernel", args, {"quad"}
    args["MODE"] = str(MODE[fn])
    return "pattern_kernel", args, set()
