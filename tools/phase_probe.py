"""
What an aberration sweep costs per setting: the two routes from fifteen Zernike weights to the gray levels of a frame with
that wavefront correction, at 1152 x 1920 (2048 x 2048 pad), for float32 and float64 grids, one setting (N = 1) and a
sweep of eight (N = 8).

    (a) the masks as a NumPy monomial sum on the host (written here: powers by repeated multiplication, one array pass per
        monomial, the pupil cut at the end), then get_display(phase_correction=array) per mask -- the 17.7 MB upload
    (b) zernike_sum(..., lazy=True) per setting, then get_display(phase_correction=mask): the descriptor goes to the engine
        and poly_kernel forms the correction on the device

Both routes include their parsing.  They alternate in one process for ROUNDS rounds on fresh weights (so neither is served
from a fingerprint); recorded are both medians, every round's pair and in how many rounds (b) won.  Next to it the time of
poly_kernel alone between HIP events (the engine's elementwise profile row around hgs_set_array_poly's launch), against
the bytes it writes over 8 TB/s: the display correction (8 bytes per pixel) and the propagation kernel in the engine's type.

    python tools/phase_probe.py [--json profiles/phase_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slmsuite_amd import _lib as L                                  # noqa: E402
from slmsuite_amd import synth                                      # noqa: E402
from slmsuite_amd.hardware import SimpleSLM                         # noqa: E402
from slmsuite_amd.holography import toolbox                         # noqa: E402
from slmsuite_amd.holography.algorithms import Hologram             # noqa: E402
from slmsuite_amd.holography.toolbox import phase                   # noqa: E402

SHAPE, SLM_SHAPE = (2048, 2048), (1152, 1920)
INDICES = list(range(1, 16))                # ANSI 1 .. 15: fifteen terms (degree 5)
ROUNDS = 15
HBM_BYTES_PER_S = 8e12


def numpy_masks(x, y, scale, weights):
    """sum_k weights[k, n] Z_k on the host: monomials x^a y^b by repeated multiplication, cut to the unit pupil"""
    terms, mono = toolbox.zernike_monomial_weights(INDICES, weights)
    xs, ys = x * x.dtype.type(scale), y * x.dtype.type(scale)
    out = np.zeros((weights.shape[1],) + x.shape, dtype=x.dtype)
    mono = mono.astype(x.dtype)
    for (a, b), w in zip(terms, mono):
        m = np.ones_like(xs)
        for _ in range(a):
            m *= xs
        for _ in range(b):
            m *= ys
        for n in range(out.shape[0]):
            if w[n] != 0:
                out[n] += w[n] * m
    out[:, np.square(xs) + np.square(ys) > 1] = 0
    return out


def probe(dtype, n_masks):
    slm = SimpleSLM(SLM_SHAPE)
    x, y = (np.ascontiguousarray(g, dtype=dtype) for g in slm.grid)
    scale = float(slm.get_source_zernike_scaling())
    h = Hologram(synth.random_target(1, SHAPE), slm_shape=SLM_SHAPE, phase=synth.seed_phase(7, SLM_SHAPE), dtype=np.float32)
    e = h._get_engine()

    def weights(seed):
        return (synth.uniform01(seed, (len(INDICES), n_masks)) * 2 - 1).astype(dtype)

    def route_a(w):
        masks = numpy_masks(x, y, scale, w)
        return [h.get_display(phase_correction=masks[n]) for n in range(n_masks)]

    def route_b(w):
        return [h.get_display(phase_correction=phase.zernike_sum((x, y), INDICES, w[:, n], aperture=scale, lazy=True))
                for n in range(n_masks)]

    w0 = weights(100)
    a0, b0 = route_a(w0), route_b(w0)                                  # warm both routes
    differing = max(float(np.mean(p != q)) for p, q in zip(a0, b0))     # (float32 host arithmetic moves a few levels by one)
    rounds = []
    for r in range(ROUNDS):
        pair = {}
        for route, fn in (("a", route_a), ("b", route_b)):
            w = weights(200 + 2 * r + (route == "b"))
            e.sync()
            t0 = time.perf_counter()
            fn(w)
            pair[route] = (time.perf_counter() - t0) * 1e3
        rounds.append(pair)
    # the kernel alone, between HIP events
    lazy = phase.zernike_sum((x, y), INDICES, w0[:, 0], aperture=scale, lazy=True)
    S = SLM_SHAPE[0] * SLM_SHAPE[1]
    kernel = {}
    e.profile_enable(True)
    for name, which, out_bytes in (("display_correction", L.DISPLAY_CORRECTION, 8), ("propagation_kernel", L.PROP_KERNEL, 4)):
        e.set_array_poly(which, lazy)
        e.profile_read()
        for _ in range(20):
            e.set_array_poly(which, lazy)
        prof = e.profile_read()["elementwise"]
        us = prof["ms"] * 1e3 / max(1, prof["launches"])
        floor_us = S * out_bytes / HBM_BYTES_PER_S * 1e6
        kernel[name] = {"event_us": round(us, 2), "samples": prof["launches"], "bytes_written": S * out_bytes,
                        "bytes_over_8TBps_us": round(floor_us, 3), "share_of_that_bound": round(floor_us / us, 3) if us > 0 else None}
    e.profile_enable(False)
    e.clear_propagation_kernel()
    res = {"numpy_route_ms_median": round(statistics.median(r["a"] for r in rounds), 3),
           "lazy_route_ms_median": round(statistics.median(r["b"] for r in rounds), 3),
           "rounds_ms": [[round(r["a"], 3), round(r["b"], 3)] for r in rounds],
           "lazy_faster_in_rounds": sum(r["b"] < r["a"] for r in rounds), "rounds": ROUNDS,
           "levels_differing_fraction": differing, "degree": lazy.degree, "poly_kernel": kernel}
    h._release_engine()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the result to this file")
    args = ap.parse_args()
    out = {"shape": list(SHAPE), "slm_shape": list(SLM_SHAPE), "terms": len(INDICES), "engine_dtype": "float32"}
    for dtype in (np.float32, np.float64):
        for n in (1, 8):
            out[f"{np.dtype(dtype).name}_n{n}"] = res = probe(dtype, n)
            print(f"{np.dtype(dtype).name} N={n}: numpy {res['numpy_route_ms_median']} ms, lazy {res['lazy_route_ms_median']} ms",
                  file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
