"""
What a live sweep of a grating or a mode mask costs per setting: the two routes from a handful of parameters to the gray
levels of a frame with that mask as its correction, at 1152 x 1920 (2048 x 2048 pad), for float32 and float64 grids.

    (a) the mask as the NumPy expression on the host (written here, as the reference forms it), then
        get_display(phase_correction=array) -- the 17.7 MB upload
    (b) the function with lazy=True on a grid prepared once (prepare_grid), then get_display(phase_correction=mask): the
        descriptor goes to the engine and pattern_kernel forms the correction on the device

Cases: laguerre_gaussian(l=3, p=2) with the radius swept, and a binary grating with the vector and duty cycle swept.  The
routes alternate in one process for ROUNDS rounds on fresh parameters (so neither is served from a fingerprint); recorded are
both medians, every round's pair and in how many rounds (b) won.  Next to it the time of pattern_kernel alone between HIP
events (the engine's elementwise profile row around hgs_set_array_pattern's launch) against the bytes it writes over 8 TB/s.

The prepared grid by itself: zernike_sum(lazy=True) + get_display per setting with the raw grid (the route before
prepare_grid existed) and with the prepared one, alternating in the same process.

    python tools/pattern_probe.py [--json profiles/pattern_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
from scipy import special

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slmsuite_amd import _lib as L                                  # noqa: E402
from slmsuite_amd import synth                                      # noqa: E402
from slmsuite_amd.hardware import SimpleSLM                         # noqa: E402
from slmsuite_amd.holography.algorithms import Hologram             # noqa: E402
from slmsuite_amd.holography.toolbox import phase                   # noqa: E402

SHAPE, SLM_SHAPE = (2048, 2048), (1152, 1920)
INDICES = list(range(1, 16))
ROUNDS = 15
HBM_BYTES_PER_S = 8e12


def numpy_lg(x, y, l, p, w):
    out = l * np.arctan2(x, y)
    out += np.pi * np.heaviside(-special.genlaguerre(p, abs(l))(16 * (y * y + x * x) / w / w), 0)
    return out


def numpy_binary(x, y, vector, shift, duty):
    d = np.mod((2 * np.pi * vector[0]) * x + (2 * np.pi * vector[1]) * y + shift, 2 * np.pi)
    d[np.isclose(d, 2 * np.pi)] = 0
    d -= 2 * np.pi * (1 - duty)
    return np.where(np.logical_or(d > 0, np.isclose(d, 0)), np.pi, 0)


def probe(dtype):
    slm = SimpleSLM(SLM_SHAPE)
    x, y = (np.ascontiguousarray(g, dtype=dtype) for g in slm.grid)
    prepared = phase.prepare_grid((x, y))
    w0 = float(prepared.radius)
    h = Hologram(synth.random_target(1, SHAPE), slm_shape=SLM_SHAPE, phase=synth.seed_phase(7, SLM_SHAPE), dtype=np.float32)
    e = h._get_engine()

    def setting(seed):
        u = synth.uniform01(seed, (3,))
        return float(u[0]), float(u[1]), float(u[2])

    cases = {
        "laguerre_gaussian_l3_p2": (
            lambda u: numpy_lg(x, y, 3, 2, w0 * (0.5 + u[0])),
            lambda u: phase.laguerre_gaussian(prepared, 3, 2, w=w0 * (0.5 + u[0]), lazy=True)),
        "binary": (
            lambda u: numpy_binary(x, y, (0.002 + 0.002 * u[0], 0.001 * u[1]), 0.4, 0.3 + 0.4 * u[2]),
            lambda u: phase.binary(prepared, (0.002 + 0.002 * u[0], 0.001 * u[1]), 0.4, duty_cycle=0.3 + 0.4 * u[2], lazy=True)),
    }
    S = SLM_SHAPE[0] * SLM_SHAPE[1]
    res = {}
    for name, (host, lazy) in cases.items():
        routes = (("a", lambda u: h.get_display(phase_correction=host(u))), ("b", lambda u: h.get_display(phase_correction=lazy(u))))
        u0 = setting(100)
        a0, b0 = (fn(u0) for _, fn in routes)                           # warm both routes
        rounds = []
        for r in range(ROUNDS):
            pair = {}
            for route, fn in routes:
                u = setting(200 + 2 * r + (route == "b"))
                e.sync()
                t0 = time.perf_counter()
                fn(u)
                pair[route] = (time.perf_counter() - t0) * 1e3
            rounds.append(pair)
        mask = lazy(u0)
        kernel = {}
        e.profile_enable(True)
        for target, which, out_bytes in (("display_correction", L.DISPLAY_CORRECTION, 8), ("propagation_kernel", L.PROP_KERNEL, 4)):
            e.set_array_poly(which, mask)
            e.profile_read()
            for _ in range(20):
                e.set_array_poly(which, mask)
            prof = e.profile_read()["elementwise"]
            us = prof["ms"] * 1e3 / max(1, prof["launches"])
            floor_us = S * out_bytes / HBM_BYTES_PER_S * 1e6
            kernel[target] = {"event_us": round(us, 2), "samples": prof["launches"], "bytes_written": S * out_bytes,
                              "bytes_over_8TBps_us": round(floor_us, 3), "share_of_that_bound": round(floor_us / us, 3) if us > 0 else None}
        e.profile_enable(False)
        e.clear_propagation_kernel()
        res[name] = {"numpy_route_ms_median": round(statistics.median(r["a"] for r in rounds), 3),
                     "lazy_route_ms_median": round(statistics.median(r["b"] for r in rounds), 3),
                     "rounds_ms": [[round(r["a"], 3), round(r["b"], 3)] for r in rounds],
                     "lazy_faster_in_rounds": sum(r["b"] < r["a"] for r in rounds), "rounds": ROUNDS,
                     "levels_differing_fraction": float(np.mean(a0 != b0)), "pattern_kernel": kernel}

    # the prepared grid by itself: the lazy Zernike route with and without it
    scale = float(slm.get_source_zernike_scaling())

    def weights(seed):
        return (synth.uniform01(seed, (len(INDICES),)) * 2 - 1).astype(dtype)

    routes = (("raw", lambda w: h.get_display(phase_correction=phase.zernike_sum((x, y), INDICES, w, aperture=scale, lazy=True))),
              ("prepared", lambda w: h.get_display(phase_correction=phase.zernike_sum(prepared, INDICES, w, aperture=scale, lazy=True))))
    for _, fn in routes:
        fn(weights(300))
    rounds = []
    for r in range(ROUNDS):
        pair = {}
        for route, fn in routes:
            w = weights(400 + 2 * r + (route == "prepared"))
            e.sync()
            t0 = time.perf_counter()
            fn(w)
            pair[route] = (time.perf_counter() - t0) * 1e3
        rounds.append(pair)
    res["zernike_sum_lazy"] = {"raw_grid_ms_median": round(statistics.median(r["raw"] for r in rounds), 3),
                               "prepared_grid_ms_median": round(statistics.median(r["prepared"] for r in rounds), 3),
                               "rounds_ms": [[round(r["raw"], 3), round(r["prepared"], 3)] for r in rounds],
                               "prepared_faster_in_rounds": sum(r["prepared"] < r["raw"] for r in rounds), "rounds": ROUNDS}
    h._release_engine()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the result to this file")
    args = ap.parse_args()
    out = {"shape": list(SHAPE), "slm_shape": list(SLM_SHAPE), "engine_dtype": "float32"}
    for dtype in (np.float32, np.float64):
        out[np.dtype(dtype).name] = res = probe(dtype)
        for name, r in res.items():
            print(f"{np.dtype(dtype).name} {name}: {({k: v for k, v in r.items() if k.endswith('_median')})}", file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
