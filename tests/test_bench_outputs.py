"""
``bench.py --dump-outputs`` on the device (``-m gpu``): a plain run writes what its last timed step computed, and that is what
a caller of the same path gets from the same inputs after the warm-up and the timed steps.  (bench.main() runs in this
process, which has the engine loaded already: a second interpreter would only add its start-up to the suite's time.)
"""
import json
import sys

import numpy as np
import pytest

from conftest import ROOT, phase_rel_l2, rel_l2

pytestmark = pytest.mark.gpu


def test_dump_outputs_are_what_the_timed_steps_computed(tmp_path, monkeypatch, capsys):
    from slmsuite_amd import _lib as L
    from slmsuite_amd import synth
    from slmsuite_amd.batch import HologramBatch
    from slmsuite_amd.holography.algorithms import SpotHologram
    sys.path.insert(0, ROOT)
    import bench
    W, K = 3, 5
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--workload", "small", "--steps", str(K), "--warmup", str(W),
                                      "--dump-outputs", str(tmp_path)])
    capsys.readouterr()
    bench.main()
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = lines[0]
    assert d["steps"] == K and d["repetitions"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["event_ms_per_step"] is None
    ph, w = np.load(tmp_path / "phase.npy"), np.load(tmp_path / "weights.npy")
    assert ph.dtype == np.float32 and w.dtype == np.float32

    # the same hologram through the same path here: SpotHologram 16 x 16 on a 1024^2 pad, SLM 288 x 480, dense kernels forced
    shape, slm = (1024, 1024), (288, 480)
    host = SpotHologram.make_rectangular_array(shape, (16, 16), (32, 32), basis="knm", slm_shape=slm,
                                               phase=synth.seed_phase(2, slm), dtype=np.float32)
    hb = HologramBatch(shape, slm, host.target, synth.seed_phase(2, slm)[None], spot_index=host.spot_knm_rounded,
                       spot_amp=host.spot_amp)
    try:
        hb.set_option(L.OPT_SPARSE_COLUMNS, 0)
        hb.optimize("WGS-Leonardo", W)
        hb.optimize("WGS-Leonardo", K)
        want_ph = hb.phases()
        want_w = hb.engine.get(L.WEIGHTS)[:, host.spot_knm_rounded[1], host.spot_knm_rounded[0]]
    finally:
        hb.close()
    assert ph.shape == want_ph.shape == (1,) + slm and w.shape == want_w.shape == (1, 256)
    assert phase_rel_l2(ph, want_ph) < 1e-6
    assert rel_l2(w, want_w) < 1e-6
