#!/usr/bin/env python
"""
Record tests/golden/pattern_*.npz: what the REAL reference's ``toolbox.phase`` returns on the CPU for its gratings, lenses
and Gaussian-mode masks (toolbox/phase.py:37-498, :1800-1935) on the grids built here.  Runs where the reference checkout is
(see tools/make_golden.py); the fixtures hold inputs and recorded outputs only.

    python tools/make_golden_patterns.py

pattern_grids.npz holds ``<grid>/x`` and ``<grid>/y`` (float64; the float32 grids are these, cast):
    slm      the 48 x 64 grid of a simulated SLM (a product grid)
    odd      37 x 53, centred axes that hold 0 exactly (odd quadrants, exact zeros of odd Hermite orders), an SLM's units
    rot      the 33 x 50 rotated grid of the phase fixtures: no product grid
    tiny35   3 x 5
    tiny11   1 x 1, off the origin
pattern_<function>.npz holds cases as ``<case>@<grid>/<array>``:
    call     JSON: fn, grid, kwargs (infinite focal lengths as the string "inf", ``grating`` by name)
    ref64    the call on the float64 grid
    ref32    the call on the float32 grid
    q        threshold cases: the float64 decision quantity -- binary's d (after the duty-cycle shift), the Laguerre value,
             the Hermite product; for bahtinov with binary the d of each window, 0 outside the windows
Every case runs on ``slm``; the first case of a function runs on every grid; a few more are placed where their point is
(the odd grid for quadrants, bahtinov and H_1).  The coordinates of rot and the tiny grids span a fraction of a unit, where
the recorded vectors would leave a grating flat: there the vectors are 250 times and the radii 150 times the recorded ones
(``call`` holds what was passed).  The marginal set of a threshold case -- 0 < |q| <= 1e-9 max|q|, for binary
| |d| - 1e-8 | <= 1e-9, the edge of its isclose(d, 0) -- must hold at most 0.1 % of its pixels: asserted here.  (A pixel
period puts a quarter of the pixels at |d| ~ 1e-16, where the last bit of a product decides the sign of d and isclose decides
the pixel: those are no marginal pixels, the tests compare them.)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import GOLD, import_reference  # noqa: E402
from make_golden_phase import meshgrid  # noqa: E402

INF = "inf"
# function -> [(case, kwargs, extra grids)]; the first case of each also runs on every grid
CASES = {
    "blaze": [("v2", dict(vector=(0.003, -0.002)), ()), ("v3", dict(vector=(0.003, -0.002, 0.0004)), ()),
              ("zero", dict(vector=(0, 0)), ())],
    "sinusoid": [("shifted", dict(vector=(0.004, 0.001), shift=0.7, a=2.5, b=-0.5), ()), ("zero", dict(vector=(0, 0), shift=0.3), ()),
                 ("plain", dict(vector=(-0.002, 0.005)), ())],
    "binary": [("kspace", dict(vector=(0.0031, 0.0017), shift=0.4, duty_cycle=0.3), ()),
               ("pixel_4_0", dict(vector=(4, 0)), ("odd",)),
               ("pixel_4_6", dict(vector=(4, 6), a=1.0, b=-1.0, duty_cycle=.25), ("odd", "rot")),
               ("zero_shift", dict(vector=(0, 0), shift=4.0), ()),
               ("ints", dict(vector=(0.0031, 0.0017), a=3, b=1), ())],
    "lens": [("scalar", dict(f=40.0), ()), ("pair", dict(f=(30.0, -55.0)), ()), ("inf_fy", dict(f=(INF, 25.0)), ())],
    "axicon": [("pair", dict(f=(3.0, 5.0)), ()), ("scalar_w", dict(f=4.0, w=0.9), ()), ("inf_fy", dict(f=(INF, -2.0)), ())],
    "laguerre_gaussian": [("l2_p0", dict(l=2, p=0), ()), ("lm3_p2", dict(l=-3, p=2), ("rot", "odd")), ("l0_p3", dict(l=0, p=3), ("rot",))],
    "hermite_gaussian": [("n3_m2", dict(n=3, m=2), ()), ("n0_m0", dict(n=0, m=0), ()), ("n1_m0", dict(n=1, m=0), ("odd",))],
    "quadrants": [("center", dict(radius=0.004, center=(0.001, -0.0005)), ())],
    "bahtinov": [("binary", dict(radius=0.006, grating="binary"), ()), ("blaze", dict(radius=0.006, grating="blaze"), ("odd", "rot")),
                 ("sinusoid", dict(radius=0.006, angle=0.3, grating="sinusoid"), ("odd", "rot"))],
}
ALL_GRIDS = ("slm", "odd", "rot", "tiny35", "tiny11")


def adapt(kwargs, gname):
    """The kwargs for the grid: gratings that vary over the small coordinates of rot and the tiny grids."""
    kw = dict(kwargs)
    if gname in ("rot", "tiny35", "tiny11"):
        v = kw.get("vector")
        if v is not None and 0 < max(abs(c) for c in v) <= 1:
            kw["vector"] = tuple(250 * c for c in v[:2]) + tuple(v[2:])
        if "radius" in kw:
            kw["radius"] = 150 * kw["radius"]
            if "center" in kw:
                kw["center"] = tuple(150 * c for c in kw["center"])
    return kw


def decode(rp, kwargs):
    """The recorded kwargs as the call takes them."""
    kw = dict(kwargs)
    if "f" in kw and isinstance(kw["f"], (list, tuple)):
        kw["f"] = tuple(np.inf if v == INF else v for v in kw["f"])
    if "grating" in kw:
        kw["grating"] = getattr(rp, kw["grating"])
    for k in ("vector", "center"):
        if k in kw:
            kw[k] = tuple(kw[k])
    return kw


def binary_d(rp, grid, vector=(0, 0), shift=0, a=np.pi, b=0, duty_cycle=.5):
    """binary()'s decision quantity on a float64 grid (phase.py:211-248), None for a zero vector."""
    x, y = grid
    duty = np.clip(float(duty_cycle), 0, 1)
    if np.any(np.abs(vector) > 1):
        grid = np.meshgrid(np.arange(x.shape[1]).astype(float), np.arange(x.shape[0]).astype(float))
        vector = (0 if vector[0] == 0 else 1. / vector[0], 0 if vector[1] == 0 else 1. / vector[1])
    if vector[0] == 0 and vector[1] == 0:
        return None
    d = np.mod(rp.blaze(grid, vector) + shift, 2 * np.pi)
    d[np.isclose(d, 2 * np.pi)] = 0
    d -= 2 * np.pi * (1 - duty)
    return d


def decision(rp, fn, grid, kw):
    from scipy import special
    x, y = grid
    if fn == "binary":
        return binary_d(rp, grid, **kw)
    if fn == "laguerre_gaussian" and kw["p"] != 0:
        w = rp._determine_source_radius(grid, kw.get("w"))
        return special.genlaguerre(kw["p"], abs(kw["l"]))(16 * (y * y + x * x) / w / w)
    if fn == "hermite_gaussian":
        w = rp._determine_source_radius(grid, kw.get("w"))
        return special.hermite(kw["n"])(4 / w * x) * special.hermite(kw["m"])(4 / w * y)
    if fn == "bahtinov" and kw["grating"] is rp.binary:
        s, c = np.sin(kw.get("angle", 10 * np.pi / 180)), np.cos(kw.get("angle", 10 * np.pi / 180))
        q = np.zeros_like(x)
        hh, hw = x.shape[0] // 2, x.shape[1] // 2
        for i, v in enumerate(kw["radius"] * np.array([(s, c), (s, -c), (0, 1), (0, 1)])):
            y0, x0 = hh * (i % 2), hw * ((3 - i) // 2)
            win = (slice(y0, min(y0 + hh, x.shape[0] - 1)), slice(x0, min(x0 + hw, x.shape[1] - 1)))       # (window_slice clips the ends)
            if q[win].size:
                q[win] = binary_d(rp, (x[win], y[win]), vector=v)
        return q
    return None


def marginal(fn, q):
    if fn in ("binary", "bahtinov"):
        return np.abs(np.abs(q) - 1e-8) <= 1e-9
    return (q != 0) & (np.abs(q) <= 1e-9 * np.abs(q).max())


def main():
    import_reference()
    from slmsuite.hardware.slms.simulated import SimulatedSLM
    from slmsuite.holography.toolbox import phase as rp
    limit = max(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD) if f.startswith("phase_"))

    slm = SimulatedSLM((64, 48), pitch_um=(8, 8), wav_um=0.78)
    grids = {"slm": tuple(np.array(g, dtype=np.float64) for g in slm.grid), "odd": tuple(meshgrid(37, 53, pitch=10.0))}
    xr, yr = meshgrid(33, 50)
    c, s = np.cos(0.1), np.sin(0.1)
    grids["rot"] = (np.ascontiguousarray(c * xr - s * yr), np.ascontiguousarray(s * xr + c * yr))
    grids["tiny35"] = tuple(meshgrid(3, 5))
    xt, yt = meshgrid(1, 1)
    grids["tiny11"] = (xt + 0.003, yt - 0.002)
    assert grids["slm"][0].shape == (48, 64) and 0.0 in grids["odd"][0][0] and 0.0 in grids["odd"][1][:, 0]

    files = {"pattern_grids": {f"{g}/{n}": a for g, (x, y) in grids.items() for n, a in (("x", x), ("y", y))}}
    for fn, cases in CASES.items():
        arrays = files.setdefault("pattern_" + fn, {})
        for index, (case, kwargs, extra) in enumerate(cases):
            for gname in ALL_GRIDS if index == 0 else ("slm",) + tuple(extra):
                x, y = grids[gname]
                used = adapt(kwargs, gname)
                kw = decode(rp, used)
                rec = {"call": np.array(json.dumps(dict(fn=fn, grid=gname, kwargs=used)))}
                rec["ref64"] = np.array(getattr(rp, fn)((x, y), **kw))
                rec["ref32"] = np.array(getattr(rp, fn)((x.astype(np.float32), y.astype(np.float32)), **kw))
                assert rec["ref64"].shape == x.shape and rec["ref32"].shape == x.shape, (fn, case, gname)
                q = decision(rp, fn, (x, y), kw)
                if q is not None:
                    rec["q"] = np.array(q, dtype=np.float64)
                    share = float(np.mean(marginal(fn, rec["q"])))
                    assert share <= 1e-3, f"{fn}/{case}@{gname}: {share:.2%} of the pixels are marginal"
                    if share:
                        print(f"  {fn}/{case}@{gname}: {share:.4%} marginal")
                arrays.update({f"{case}@{gname}/{k}": v for k, v in rec.items()})
    for file, arrays in files.items():
        path = os.path.join(GOLD, file + ".npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print(f"{path}: {len({k.split('/')[0] for k in arrays})} entries, {size} bytes")
        assert size <= limit, f"{path} is larger than the largest phase fixture ({limit} bytes)"


if __name__ == "__main__":
    main()
