"""
Timing of Hologram.remove_vortices() on the engine (hgs_remove_vortices) at the cfg 2 geometry (4096 x 4096 pad,
1152 x 1920 SLM, float32): a dense image target, 20 GS iterations, then the removal on the stored phase_ff.  Reports the
number of vortices K, the HIP-event time of the call's kernels (search passes + removal; the search alone from a second
call against an all-zero target, where the removal does not run) and the atan2 evaluations per second of the removal
against the fp32 vector peak.  --cpu times the NumPy statement of the same operation at 512 x 512 instead (no GPU).

    python tools/vortex_probe.py [--json PATH] [--iters N]
    python tools/vortex_probe.py --cpu
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slmsuite_amd import _lib as L              # noqa: E402
from slmsuite_amd import synth                  # noqa: E402

SHAPE, SLM = (4096, 4096), (1152, 1920)
# MI355X: 256 CUs x 4 SIMDs x 32 lanes per cycle x 2.4 GHz = 78.6e12 fp32 vector operations per second (an FMA counts
# once here: the 157.3 TFLOPS of the data sheet)
PEAK_VALU_OPS = 256 * 4 * 32 * 2.4e9
OPS_PER_ATAN2 = 27                              # vector operations per vortex and pixel in the float32 removal loop (ISA)


def np_vortices(phase, target):
    """The reference's detection (analysis/__init__.py:1207-1267) with the 5 x 5 erosion of target > 0."""
    dd = [np.mod(np.diff(phase, axis=a, prepend=np.nan) - np.pi, 2 * np.pi) for a in range(2)]
    with np.errstate(invalid="ignore"):
        w = -(dd[0] - dd[1] - np.roll(dd[0], 1, axis=1) + np.roll(dd[1], 1, axis=0)) / (2 * np.pi)
    w[np.isnan(w)] = 0
    w = np.rint(w)
    h, wd = phase.shape
    padded = np.zeros((h + 4, wd + 4), dtype=bool)
    padded[2:-2, 2:-2] = target > 0
    keep = np.ones((h, wd), dtype=bool)
    for dy in range(5):
        for dx in range(5):
            keep &= padded[dy:dy + h, dx:dx + wd]
    w[~keep] = 0
    rows, cols = np.nonzero(w)
    return rows, cols, w[rows, cols]


def cpu_probe(n=512, iters=20):
    """The reference's loop (one whole-image arctan2 per vortex) in NumPy on a speckled phase: seconds for K vortices."""
    rng_phase = synth.seed_phase(3, (n, n)).astype(np.float64)
    target = synth.random_target(3, (n, n)).astype(np.float64) + 0.1
    # a band-limited speckle phase like a stored phase_ff: the farfield phase of a random SLM window half the pad wide
    nf = np.zeros((n, n), dtype=complex)
    nf[n // 4:3 * n // 4, n // 4:3 * n // 4] = np.exp(1j * rng_phase[:n // 2, :n // 2])
    phase = np.angle(np.fft.fftshift(np.fft.fft2(np.fft.fftshift(nf))))
    rows, cols, wts = np_vortices(phase, target)
    X, Y = np.meshgrid(np.arange(n, dtype=float), np.arange(n, dtype=float))
    k = min(len(rows), 200)
    t0 = time.perf_counter()
    for x, y, w in zip(cols[:k], rows[:k], wts[:k]):
        phase -= w * np.arctan2(X - x, Y - y)
    dt = time.perf_counter() - t0
    return {"shape": [n, n], "K": int(len(rows)), "timed_vortices": k, "seconds_per_vortex": dt / k,
            "seconds_for_K": dt / k * len(rows)}


def gpu_probe(iters):
    from slmsuite_amd.holography.algorithms import Hologram
    target = synth.random_target(1, SHAPE) + np.float32(0.1)
    h = Hologram(target, phase=synth.seed_phase(1, SLM), slm_shape=SLM)
    h.optimize("GS", maxiter=iters, verbose=False)
    h._flush_populate()                           # phase_ff of the final phase, on the device
    e = h._get_engine()
    e.sync()
    e.profile_enable(True)
    e.profile_read()
    t0 = time.perf_counter()
    k = h.remove_vortices()
    e.sync()
    wall = time.perf_counter() - t0
    ms_all = e.profile_read()["elementwise"]["ms"]
    # the search alone: nothing lies inside an all-zero target's mask, so the scatter pass and the removal do not run
    e.set(L.TARGET, np.zeros(SHAPE, dtype=np.float32))
    h.remove_vortices()
    ms_find = e.profile_read()["elementwise"]["ms"]
    e.profile_enable(False)
    h._release_engine()
    ms_remove = ms_all - 2 * ms_find               # (count pass + scan, scatter pass)
    evals = float(k) * SHAPE[0] * SHAPE[1]
    rate = evals / (ms_remove * 1e-3) if ms_remove > 0 else 0.0
    return {"shape": list(SHAPE), "slm_shape": list(SLM), "dtype": "float32", "gs_iterations": iters, "K": int(k),
            "wall_ms": round(wall * 1e3, 2), "event_ms_call": round(ms_all, 3), "event_ms_search_pass": round(ms_find, 3),
            "event_ms_removal": round(ms_remove, 3), "atan2_per_s": rate,
            "fraction_of_fp32_vector_peak": round(rate * OPS_PER_ATAN2 / PEAK_VALU_OPS, 3),
            "peak_valu_ops_per_s": PEAK_VALU_OPS, "ops_per_atan2": OPS_PER_ATAN2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the result to this file")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu", action="store_true", help="time the NumPy statement at 512 x 512 instead")
    args = ap.parse_args()
    out = {"cpu_numpy_512": cpu_probe()} if args.cpu else {"cfg2": gpu_probe(args.iters)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
