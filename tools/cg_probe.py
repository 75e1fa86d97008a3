"""
Timing of optimize(method="CG") on the engine (hgs_cg_iterate): iterations per second of one device-resident call and the
per-kernel HIP-event times of a loop body, at the cfg 1 geometry (512 x 512, SLM = pad) and the cfg 2 geometry
(4096 x 4096 pad, 1152 x 1920 SLM) with a dense image target, float32.  A body is a forward transform (row + col_fwd), the
seed pass over the farfield (cg_seed), the inverse without phase extraction (col_inv + row) and the Adam pass over the SLM
window (cg_adam).  python tools/cg_probe.py [--json PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slmsuite_amd import synth                  # noqa: E402
from slmsuite_amd.holography.algorithms import Hologram   # noqa: E402

GEOMETRIES = {"cfg1": ((512, 512), (512, 512)), "cfg2": ((4096, 4096), (1152, 1920))}
N_ITER, REPEATS = 50, 5


def probe(shape, slm):
    h = Hologram(synth.random_target(1, shape), phase=synth.seed_phase(1, slm), slm_shape=slm)
    h.optimize("CG", maxiter=5, verbose=False)             # allocations, first-use costs
    e = h._get_engine()
    best = 1e9
    for _ in range(REPEATS):
        e.sync()
        t0 = time.perf_counter()
        e.cg_iterate(N_ITER)                               # (returns the losses: ends in a stream sync)
        best = min(best, time.perf_counter() - t0)
    e.profile_enable(True)
    e.cg_iterate(N_ITER)
    prof = e.profile_read()
    e.profile_enable(False)
    per_body = {k: round(v["ms"] * 1e3 / N_ITER, 2) for k, v in prof.items() if v["launches"]}
    loss = e.cg_iterate(1)
    h._release_engine()
    return {"iterations_per_s": round(N_ITER / best, 1), "us_per_iteration": round(best / N_ITER * 1e6, 1),
            "event_us_per_body": per_body, "loss_after": float(loss[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the result to this file")
    args = ap.parse_args()
    out = {name: dict(shape=list(shape), slm_shape=list(slm), dtype="float32", n_iter=N_ITER, **probe(shape, slm))
           for name, (shape, slm) in GEOMETRIES.items()}
    text = json.dumps(out, indent=1)
    print(text)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
