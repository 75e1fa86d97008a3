"""
NumPy restatement of the gray-level conversion ``hgs_get_display`` performs (include/hgs.h), for the tests: what the
reference's ``slm.set_phase(hologram)`` displays, at shapes the recorded fixtures (tests/golden/display_*.npz) do not hold.
``test_display_cpu.py`` pins it against those fixtures first, pixel for pixel.

Not the product path (that is HIP) and not the host route of ``slmsuite_amd.hardware.DisplaySLM`` either: written
out-of-place and step by step so that the three can disagree.
"""
import glob
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def mask_of(phase, kernel=None, correction=None):
    """float64 mask of an engine-precision phase: ``+ pi`` in that precision (or ``+ kernel``), widened, plus the correction."""
    phase = np.asarray(phase)
    assert phase.dtype in (np.float32, np.float64)
    p = phase + (phase.dtype.type(np.pi) if kernel is None else np.asarray(kernel, dtype=phase.dtype))
    assert p.dtype == phase.dtype
    x = p.astype(np.float64)
    if correction is not None:
        x = x + np.asarray(correction, dtype=np.float64)
    return x


def numpy_mod(y, b):
    """``np.mod`` for floats spelled out: C ``fmod`` (exact), then the divisor's sign."""
    r = np.fmod(y, b)
    return np.where((r != 0) & (r < 0), r + b, r)


def branch_of(mask, bitdepth, s):
    """Which way the extremes send a mask: "plain" / "shift" (s == 1), "inbounds" / "mod" (s != 1)."""
    R = 2 ** bitdepth
    if s == 1:
        return "shift" if np.max(mask * -(R / 2 / np.pi)) >= 0 else "plain"
    y = mask * -(R * s / 2 / np.pi)
    return "mod" if (np.min(y) <= -R or np.max(y) > 0) else "inbounds"


def levels_of(mask, bitdepth=8, s=1.0):
    """Gray levels of a float64 mask (one hologram)."""
    R = 2 ** bitdepth
    x = np.asarray(mask, dtype=np.float64)
    if s == 1:
        y = x * -(R / 2 / np.pi)
        m = np.max(y)
        if m >= 0:
            y = y - R * 2 * np.ceil(m / R)
        out = (np.rint(y).astype(np.int64) - 1) & (R - 1)
    else:
        y = x * -(R * s / 2 / np.pi)
        if np.min(y) <= -R or np.max(y) > 0:
            y = numpy_mod(y - 1, R * s) + R * (1 - s)
            if s > 1:
                y = np.where(y < 0, float(R - 1), y)
        else:
            y = y + (R - 1)
        out = np.trunc(y).astype(np.int64)
    assert out.min() >= 0 and out.max() < R
    return out.astype(np.uint8 if bitdepth <= 8 else np.uint16)


def display_of(phase, bitdepth=8, s=1.0, correction=None, kernel=None):
    """What ``Engine.get_display`` must return for one hologram's raw phase."""
    return levels_of(mask_of(phase, kernel, correction), bitdepth, s)


def fixtures():
    """Every recorded case: ``[(name, dict of arrays)]``, sorted by name.  Keys: ``phase`` (the raw engine phase, float32 or
    float64), optional ``kernel`` and ``correction``, ``bitdepth``, ``scaling``, ``display`` and ``slm_phase`` (the
    reference's ``slm.display`` / ``slm.phase`` after ``set_phase``), ``mask`` (what ``set_phase`` was given)."""
    out = []
    for path in sorted(glob.glob(os.path.join(GOLD, "display_*.npz"))):
        with np.load(path) as z:
            names = sorted({k.split("/", 1)[0] for k in z.files})
            for n in names:
                out.append((os.path.basename(path)[:-4] + ":" + n,
                            {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")}))
    return out


def case_args(c):
    """(bitdepth, scaling, correction or None, kernel or None) of a fixture case."""
    return int(c["bitdepth"]), float(c["scaling"]), c.get("correction"), c.get("kernel")


def near_tie_x(k, bitdepth=8):
    """
    A float64 mask value x with fl(x * f) == -(k + 0.5) + 2**-46 for s == 1 (f = -(R / 2 / pi)): ``rint`` of the product
    gives -k, but subtracting a shift of 512 or more rounds it onto the tie -(k + 0.5) - shift, which rounds to even --
    one level less for odd k.  Found among the float64 neighbours of want / f; None when no neighbour's product hits it.
    """
    f = -(2 ** bitdepth / 2 / np.pi)
    want = -(k + 0.5) + 2.0 ** -46
    x = want / f
    for direction in (-np.inf, np.inf):
        c = x
        for _ in range(64):
            if c * f == want:
                return float(c)
            c = np.nextafter(c, direction)
    return None


def split_mask(x, dtype):
    """
    (raw phase v of ``dtype``, float64 correction c) whose mask is exactly the float64 array x: fl64(fl_dtype(v + pi)) + c == x.
    c = x - p is exact where p is within a factor of two of x (Sterbenz), and so is the sum that undoes it.
    """
    x = np.asarray(x, dtype=np.float64)
    v = (x - np.pi).astype(dtype)
    p = (v + np.dtype(dtype).type(np.pi)).astype(np.float64)
    c = x - p
    assert np.array_equal(p + c, x)
    return v, c
