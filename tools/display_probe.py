"""
What a frame costs after optimize(): the two routes from the device phase to the gray levels an 8-bit SLM takes, at the
cfg 2 geometry (4096 x 4096 pad, 1152 x 1920 SLM, 32 x 32 spots, float32) after optimize("WGS-Leonardo", 50), with and
without a wavefront correction.

    (a) get_phase() -- 4 bytes per pixel to the host -- then the NumPy conversion of DisplaySLM.set_phase
    (b) get_display(slm) -- two launches, 1 byte per pixel to the host

The routes alternate in one process for ROUNDS rounds, each round re-running one optimize() body first so that the phase
is device-fresh (as in a refresh loop) -- route (a) would otherwise be served from the host copy of the round before.
Recorded: both medians, every round's pair, in how many rounds (b) won, the time of the two launches between HIP events
(the elementwise row of the engine's profile) and the bytes each route downloads.

    python tools/display_probe.py [--json profiles/display_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slmsuite_amd import synth                                      # noqa: E402
from slmsuite_amd.hardware import DisplaySLM                        # noqa: E402
from slmsuite_amd.holography.algorithms import SpotHologram         # noqa: E402

SHAPE, SLM_SHAPE, ARRAY, PITCH = (4096, 4096), (1152, 1920), (32, 32), (64, 64)
ROUNDS = 15


def probe(with_correction):
    slm = DisplaySLM(SLM_SHAPE, bitdepth=8)
    if with_correction:
        slm.source["phase"] = np.random.default_rng(1).uniform(-20, 20, size=SLM_SHAPE)
    h = SpotHologram.make_rectangular_array(SHAPE, ARRAY, PITCH, basis="knm", slm_shape=SLM_SHAPE,
                                            phase=synth.seed_phase(7, SLM_SHAPE).copy())
    h.optimize("WGS-Leonardo", maxiter=50, verbose=False)
    host = DisplaySLM(SLM_SHAPE, bitdepth=8)
    host.source = slm.source
    same = np.array_equal(h.get_display(slm), host.set_phase(h.get_phase()))          # warm both routes; they must agree
    e = h._get_engine()
    rounds = []
    for _ in range(ROUNDS):
        pair = {}
        for route in ("a", "b"):
            h.optimize("WGS-Leonardo", maxiter=1, verbose=False)       # a fresh device phase, as in a refresh loop
            e.sync()
            t0 = time.perf_counter()
            if route == "a":
                out = host.set_phase(h.get_phase())
            else:
                out = h.get_display(slm)
            pair[route] = (time.perf_counter() - t0) * 1e3
        rounds.append(pair)
    e.profile_enable(True)
    e.profile_read()
    n = 20
    for _ in range(n):
        h.get_display(slm)
    prof = e.profile_read()["elementwise"]
    e.profile_enable(False)
    S = SLM_SHAPE[0] * SLM_SHAPE[1]
    res = {"routes_agree": bool(same),
           "host_route_ms_median": round(statistics.median(r["a"] for r in rounds), 3),
           "get_display_ms_median": round(statistics.median(r["b"] for r in rounds), 3),
           "rounds_ms": [[round(r["a"], 3), round(r["b"], 3)] for r in rounds],
           "get_display_faster_in_rounds": sum(r["b"] < r["a"] for r in rounds), "rounds": ROUNDS,
           "two_launches_event_us": round(prof["ms"] * 1e3 / max(1, prof["launches"]), 1), "event_samples": prof["launches"],
           "bytes_downloaded": {"host_route": 4 * S, "get_display": int(out.nbytes)}}
    h._release_engine()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the result to this file")
    args = ap.parse_args()
    out = {"shape": list(SHAPE), "slm_shape": list(SLM_SHAPE), "dtype": "float32", "bitdepth": 8,
           "without_correction": probe(False), "with_correction": probe(True)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
