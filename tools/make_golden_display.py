#!/usr/bin/env python
"""
Record tests/golden/display_*.npz: what the REAL reference displays -- ``SimulatedSLM(...).set_phase(mask)`` on the CPU
(hardware/slms/slm.py:472-783) -- for the masks ``Hologram.get_phase()`` hands it (_hologram.py:786-811).  Runs where the
reference checkout is (see tools/make_golden.py); the fixtures hold inputs and recorded outputs only.

    python tools/make_golden_display.py

A file holds cases as ``<case>/<array>``:
    phase        the RAW engine phase (float32 or float64) -- the mask is phase + pi in that precision, or phase + kernel
    kernel       optional: the propagation kernel (include_propagation)
    correction   optional: slm.source["phase"], float64
    given        optional: the array set_phase was handed where that is not the mask itself (a padded mask, integer levels)
    bitdepth, scaling (wav_um / wav_design_um as the reference formed it)
    display, slm_phase   slm.display and slm.phase afterwards
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden import GOLD, import_reference  # noqa: E402

WAV_UM = 0.78
DESIGN_UM = {"unit": None, "short": 0.9, "long": 0.7}       # phase_scaling 1, 0.8667 (in bounds without a correction), 1.1143


def x_for(want, bitdepth=8):
    """float64 x with fl(x * f) == want, f = -(2^bitdepth / 2 / pi), among the neighbours of want / f."""
    f = -(2 ** bitdepth / 2 / np.pi)
    for direction in (-np.inf, np.inf):
        c = want / f
        for _ in range(64):
            if c * f == want:
                return float(c)
            c = np.nextafter(c, direction)
    raise RuntimeError(f"no float64 neighbour of {want / f} scales to {want}")


def split(x, dtype):
    """raw phase v (dtype) and float64 correction c with fl64(fl_dtype(v + pi)) + c == x exactly"""
    x = np.asarray(x, dtype=np.float64)
    v = (x - np.pi).astype(dtype)
    p = (v + np.dtype(dtype).type(np.pi)).astype(np.float64)
    c = x - p
    assert np.array_equal(p + c, x)
    return v, c


class Recorder:
    def __init__(self, SimulatedSLM):
        self.SimulatedSLM = SimulatedSLM
        self.files = {}

    def slm(self, shape, bitdepth, design):
        return self.SimulatedSLM((shape[1], shape[0]), bitdepth=bitdepth, wav_um=WAV_UM, wav_design_um=DESIGN_UM[design])

    def case(self, file, name, phase, bitdepth=8, design="unit", correction=None, kernel=None, pad=None):
        phase = np.ascontiguousarray(phase)
        slm = self.slm(phase.shape, bitdepth, design)
        mask = phase + (phase.dtype.type(np.pi) if kernel is None else kernel)
        assert mask.dtype == phase.dtype
        rec = dict(phase=phase, bitdepth=np.int32(bitdepth), scaling=np.float64(slm.phase_scaling))
        if kernel is not None:
            rec["kernel"] = kernel
        if correction is not None:
            slm.source["phase"] = np.array(correction, dtype=np.float64)
            rec["correction"] = slm.source["phase"].copy()
        given = mask.copy()
        if pad is not None:                     # a larger array around the mask: set_phase crops it (toolbox.unpad)
            rng = np.random.default_rng(99)
            big = rng.uniform(0, 6, size=(phase.shape[0] + pad[0], phase.shape[1] + pad[1])).astype(phase.dtype)
            t, l = pad[0] // 2, pad[1] // 2
            big[t:t + phase.shape[0], l:l + phase.shape[1]] = mask
            rec["given"] = given = big
        out = slm.set_phase(given.copy())
        assert out is slm.display
        rec["display"] = np.array(slm.display)
        rec["slm_phase"] = np.array(slm.phase, dtype=np.float64)
        self.files.setdefault(file, {}).update({f"{name}/{k}": v for k, v in rec.items()})
        return rec["display"]

    def int_case(self, file, name, shape, bitdepth, design, pad=None):
        slm = self.slm(shape, bitdepth, design)
        rng = np.random.default_rng(bitdepth)
        big = (shape[0] + (pad or (0, 0))[0], shape[1] + (pad or (0, 0))[1])
        given = rng.integers(0, 2 ** bitdepth, size=big).astype(slm.dtype)
        slm.set_phase(given.copy())
        rec = dict(given=given, bitdepth=np.int32(bitdepth), scaling=np.float64(slm.phase_scaling),
                   display=np.array(slm.display), slm_phase=np.array(slm.phase, dtype=np.float64))
        self.files.setdefault(file, {}).update({f"{name}/{k}": v for k, v in rec.items()})

    def save(self):
        for file, arrays in self.files.items():
            path = os.path.join(GOLD, file + ".npz")
            np.savez_compressed(path, **arrays)
            print(f"{path}: {len({k.split('/')[0] for k in arrays})} cases, {os.path.getsize(path)} bytes")


def main():
    import_reference()
    from slmsuite.hardware.slms.simulated import SimulatedSLM
    r = Recorder(SimulatedSLM)
    rng = np.random.default_rng(20)

    # ---- the grid: 4 bit depths x 3 scalings x with / without a correction of +-20 rad, float32
    shape = (17, 23)
    phase = rng.uniform(-np.pi, np.pi, size=shape).astype(np.float32)
    corr = rng.uniform(-20, 20, size=shape)
    for bits in (1, 8, 10, 16):
        for design in DESIGN_UM:
            for c in (None, corr):
                r.case("display_grid", f"b{bits}_{design}_{'corr' if c is not None else 'plain'}", phase, bits, design, c)

    # ---- s == 1, the situations of the data-dependent shift
    shape = (33, 47)
    phase = rng.uniform(-3.1, np.pi, size=shape).astype(np.float32)
    r.case("display_unit", "plain_f32", phase)                                   # every y < 0: no shift
    r.case("display_unit", "plain_f64", rng.uniform(-3.1, np.pi, size=shape), 10)
    r.case("display_unit", "padded_f32", phase, pad=(4, 4))
    r.case("display_unit", "padded_odd_f32", phase[:30, :35], 16, "short", pad=(3, 5))
    zero = phase.copy()
    zero[17, 5] = np.float32(-np.pi)                                              # fl32(-pi) + fl32(pi) = 0: max y = 0, shift 0
    assert zero[17, 5] + np.float32(np.pi) == 0
    r.case("display_unit", "zero_f32", zero)
    kern = rng.uniform(-40, 0, size=shape).astype(np.float32)                     # phase + kernel, no pi: negative masks
    r.case("display_unit", "kernel_f32", phase, kernel=kern)
    r.case("display_unit", "kernel_b10_f32", phase, 10, kernel=kern)
    for dtype, tag in ((np.float32, "f32"), (np.float64, "f64")):                 # unwrapped CG-like phases
        wide = (rng.uniform(-1e4, 1e4, size=shape)).astype(dtype)
        r.case("display_unit", f"unwrapped_{tag}", wide)
        r.case("display_unit", f"unwrapped_b16_{tag}", wide, 16)
        r.case("display_unit", f"unwrapped_corr_{tag}", wide, 8, correction=rng.uniform(-20, 20, size=shape))
    r.case("display_unit", "unwrapped_b1_f32", rng.uniform(-1e4, 1e4, size=shape).astype(np.float32), 1)

    # ---- near ties: y = -(k + 0.5) + 2^-46 rounds to -k alone, onto the tie once a shift of 512 is subtracted; and exact ties
    ks = (101, 37, 7, 200)
    for dtype, tag in ((np.float32, "f32"), (np.float64, "f64")):
        x = rng.uniform(0.05, 6.2, size=(5, 7))
        x.flat[:4] = [x_for(-(k + 0.5) + 2.0 ** -46) for k in ks]
        x.flat[4:8] = [x_for(-(n + 0.5)) for n in (12, 13, 100, 255)]             # y exactly a half-integer
        v, c = split(x, dtype)
        alone = r.case("display_ties", f"alone_{tag}", v, correction=c)
        x2 = x.copy()
        x2.flat[20] = -3.0                                                         # one negative mask value: y > 0, shift 512
        v2, c2 = split(x2, dtype)
        shifted = r.case("display_ties", f"shifted_{tag}", v2, correction=c2)
        print(tag, "near ties alone", alone.flat[:4], "next to a negative phase", shifted.flat[:4])
        assert list(alone.flat[:4]) == [154, 218, 248, 55] and list(shifted.flat[:4]) == [153, 217, 247, 55]

    # ---- integer levels handed in (slm.py:637-663)
    r.int_case("display_int", "b8_unit", (9, 14), 8, "unit")
    r.int_case("display_int", "b8_short_padded", (9, 14), 8, "short", pad=(2, 4))
    r.int_case("display_int", "b10_long", (9, 14), 10, "long")
    r.int_case("display_int", "b16_unit_padded", (9, 14), 16, "unit", pad=(3, 1))
    r.save()


if __name__ == "__main__":
    main()
