"""
CPU tests of the product's host side: the C-ABI library loads and exports what include/hgs.h
declares, the class surface builds the same host state as the reference (checked against the
golden fixtures), flag / history logic, and the loud failure without a GPU.  No compute calls.
"""
import os
import sys
import re

import numpy as np
import pytest

from conftest import ROOT, golden_names, load_golden
from golden_cases import hologram_inputs, spot_null_ctor
from slmsuite_amd import _lib as L
from slmsuite_amd import synth
from slmsuite_amd.engine import make_step
from slmsuite_amd.holography import toolbox
from slmsuite_amd.holography.algorithms import ALGORITHM_DEFAULTS, ALGORITHM_INDEX, Hologram, SpotHologram


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "hgs.h")).read()
    declared = set(re.findall(r"\b(hgs_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"hgs_engine", "hgs_config", "hgs_step", "hgs_status"}
    assert declared, "no declarations parsed"
    lib = L.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/hgs.h but not exported"
    assert set(L.EXPORTS) == declared
    assert lib.hgs_version().startswith(b"hgs ")


def test_struct_layouts_match_header():
    # field order is part of the ABI: keep ctypes and the header in lock-step
    hdr = open(os.path.join(ROOT, "include", "hgs.h")).read()
    cfg = re.search(r"typedef struct \{([^{}]*)\} hgs_config;", hdr, re.S).group(1)
    names = re.findall(r"\b([a-z_]+)\s*[;,]", re.sub(r"/\*.*?\*/", "", cfg, flags=re.S))
    assert [n for n, _ in L.hgs_config._fields_] == names
    st = re.search(r"typedef struct \{([^{}]*)\} hgs_step;", hdr, re.S).group(1)
    names = re.findall(r"\b([a-z_]+)\s*[;,]", re.sub(r"/\*.*?\*/", "", st, flags=re.S))
    assert [n for n, _ in L.hgs_step._fields_] == names


def test_option_constants_match_header():
    """hgs_set_option's enumerators: the ctypes module and the header must not drift apart (HGS_OPT_X = n <-> L.OPT_X)."""
    hdr = open(os.path.join(ROOT, "include", "hgs.h")).read()
    opts = dict(re.findall(r"\bHGS_OPT_([A-Z_]+)\s*=\s*(\d+)", hdr))
    assert len(opts) >= 7
    for name, val in opts.items():
        assert getattr(L, "OPT_" + name) == int(val), name


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    h = Hologram(synth.random_target(1, (64, 64)), phase=synth.seed_phase(1, (64, 64)))
    with pytest.raises(L.HgsError):
        h.optimize("GS", maxiter=1, verbose=False)


def test_product_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "slmsuite_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                # no import, no path, no dlopen / subprocess of anything under oracle/
                assert not re.search(r"(from|import)\s+oracle\b|oracle[/.]hgs_oracle|['\"]oracle['\"/]|hgs_oracle", src), f


def test_constants_follow_reference_order():
    assert list(ALGORITHM_INDEX) == ["GS", "WGS-Leonardo", "WGS-Kim", "WGS-Nogrette", "WGS-Wu", "WGS-tanh", "CG"]
    assert ALGORITHM_DEFAULTS["WGS-Kim"]["fix_phase_iteration"] == 10


def test_helpers_match_reference():
    meta, gold = load_golden("helpers")
    for row, out in zip(gold["unpad_in"], gold["unpad_out"]):
        assert toolbox.unpad((int(row[0]), int(row[1])), (int(row[2]), int(row[3]))) == tuple(out)
    for row, out in zip(gold["padshape_in"], gold["padshape_out"]):
        assert Hologram.get_padded_shape((int(row[0]), int(row[1])), int(row[2]), bool(row[3])) == tuple(out)
    m = np.arange(12.0).reshape(3, 4)
    p = toolbox.pad(m, (8, 9))
    assert p.shape == (8, 9) and np.array_equal(toolbox.unpad(p, (3, 4)), m)


@pytest.mark.parametrize("name", golden_names("holo_")[:4] + golden_names("mraf_")[:1])
def test_constructor_state_matches_reference(name):
    """target normalisation, weights = target (NaN -> 0), scalar/array amp: compare with weights_0-like data."""
    meta, gold = load_golden(name)
    kw = hologram_inputs(meta)
    h = Hologram(**kw)
    assert h.shape == tuple(meta["shape"]) and h.slm_shape == tuple(meta["slm_shape"])
    t = np.array(kw["target"], dtype=h.dtype)
    t = np.abs(t)
    t *= 1 / np.sqrt(np.nansum(np.square(t)))
    np.testing.assert_array_equal(np.nan_to_num(h.target, nan=-1), np.nan_to_num(t, nan=-1))
    np.testing.assert_array_equal(h.weights, np.nan_to_num(t, nan=0))
    if kw["amp"] is None:
        assert np.isscalar(h.amp) and abs(h.amp - 1 / np.sqrt(np.prod(h.slm_shape))) < 1e-15
    else:
        assert abs(float(np.sum(h.amp.astype(float) ** 2)) - 1) < 1e-5
    assert h.iter == 0 and h.stats == {"method": [], "flags": {}, "stats": {}}
    assert h.amp_ff is None and h.phase_ff is None
    np.testing.assert_allclose(h.get_phase(), kw["phase"] + np.pi)


def test_spot_hologram_host_state_matches_reference():
    meta, gold = load_golden("spot_WGSLeonardo_computational_spot")
    shape, slm = tuple(meta["shape"]), tuple(meta["slm_shape"])
    h = SpotHologram.make_rectangular_array(shape, tuple(meta["array_shape"]), tuple(meta["array_pitch"]),
                                            basis="knm", slm_shape=slm, phase=synth.seed_phase(meta["seed"], slm))
    np.testing.assert_array_equal(h.spot_knm, gold["spot_knm"])
    np.testing.assert_array_equal(h.spot_knm_rounded, gold["spot_knm_rounded"])
    np.testing.assert_allclose(h.spot_amp, gold["spot_amp"])
    assert h.spot_integration_width_knm == meta["width"] and len(h) == 64
    ky, kx = h.spot_knm_rounded[1], h.spot_knm_rounded[0]
    np.testing.assert_allclose(h.target[ky, kx], gold["target_spots"], rtol=1e-6)
    assert np.count_nonzero(h.target) == 64
    with pytest.raises(ValueError):
        SpotHologram((64, 64), [[70], [10]], basis="knm", slm_shape=(64, 64))


@pytest.mark.parametrize("name", golden_names("spotnull_"))
def test_spot_hologram_null_target_matches_reference(name):
    """null_vectors / null_radius / null_region / null_region_radius_frac (_spots.py:1300-1373, 1514-1538): the target
    raster the reference built -- NaN background, zero region, zero disks (edge rule included), spots -- bit for bit."""
    meta, gold = load_golden(name)
    shape, slm = tuple(meta["shape"]), tuple(meta["slm_shape"])
    h = SpotHologram.make_rectangular_array(shape, tuple(meta["array_shape"]), tuple(meta["array_pitch"]),
                                            basis="knm", slm_shape=slm, phase=synth.seed_phase(meta["seed"], slm),
                                            **spot_null_ctor(meta, gold))
    assert h.null_radius_knm == int(gold["null_radius_knm"])
    np.testing.assert_array_equal(np.isnan(h.target), np.isnan(gold["target"]))
    np.testing.assert_array_equal(np.nan_to_num(h.target, nan=-1), np.nan_to_num(gold["target"], nan=-1))
    assert h._mraf_enabled()
    np.testing.assert_array_equal(h.weights, np.nan_to_num(gold["target"], nan=0))


def test_spot_hologram_null_region_alone_is_ignored():
    """Without null points the reference never consults the null region (_spots.py:1514-1515): plain zero background."""
    region = np.ones((64, 64), dtype=bool)
    h = SpotHologram((64, 64), [[20, 40], [30, 30]], basis="knm", slm_shape=(64, 64), null_region=region)
    assert not np.isnan(h.target).any() and np.count_nonzero(h.target) == 2


def test_flag_parsing_and_errors():
    h = Hologram(synth.random_target(1, (64, 64)), phase=synth.seed_phase(1, (64, 64)), my_flag=3)
    with pytest.raises(ValueError):
        h._update_flags("nope", False, None, [])
    with pytest.raises(ValueError):
        h._update_flags("GS", False, "bogus", [])
    with pytest.raises(ValueError):
        h._update_flags("GS", False, None, ["bogus"])
    h._update_flags("WGS-Kim", False, None, [], feedback_exponent=0.7)
    assert h.flags["feedback_exponent"] == 0.7 and h.flags["fix_phase_iteration"] == 10
    assert h.flags["fixed_phase"] is False and h.flags["my_flag"] == 3 and h.flags["feedback"] == "computational"
    st = make_step(h.flags, 4, false_run=2)
    assert (st.method, st.feedback, st.iter, st.false_run, st.fix_phase_iteration) == (2, 0, 4, 2, 10)
    assert abs(st.feedback_exponent - 0.7) < 1e-15 and st.mraf_enabled == 0
    h.flags["feedback"] = "experimental"
    with pytest.raises(NotImplementedError):
        make_step(h.flags, 0)
    with pytest.raises(ValueError):
        Hologram(synth.random_target(1, (64, 64)), phase=np.zeros((32, 32)), amp=np.ones((16, 16)))
    with pytest.raises(ValueError):
        Hologram(synth.random_target(1, (64, 64)), phase=np.zeros((64, 64)), dtype=np.float16)


def test_false_run_history():
    h = Hologram(synth.random_target(1, (64, 64)), phase=synth.seed_phase(1, (64, 64)))
    h.stats["flags"]["fixed_phase"] = [np.nan, False, False, False]
    assert h._false_run() == 3 and h._false_run(skip_last=True) == 2
    h.stats["flags"]["fixed_phase"] = [False, True, False]
    assert h._false_run() == 1
    h.stats["flags"]["fixed_phase"] = []
    assert h._false_run() == 0


def test_stats_dictionary_bookkeeping():
    h = Hologram(synth.random_target(1, (64, 64)), phase=synth.seed_phase(1, (64, 64)))
    h._update_flags("WGS-Leonardo", False, None, [])
    h._update_stats_dictionary({})
    h.iter = 2
    h.flags["new_flag"] = 5
    h._update_stats_dictionary({"computational": {"efficiency": 0.5}})
    assert h.stats["method"] == ["WGS-Leonardo", "", "WGS-Leonardo"]
    assert h.stats["flags"]["fixed_phase"][0] is False and np.isnan(h.stats["flags"]["fixed_phase"][1])
    assert np.isnan(h.stats["flags"]["new_flag"][0]) and h.stats["flags"]["new_flag"][2] == 5
    eff = h.stats["stats"]["computational"]["efficiency"]
    assert np.isnan(eff[0]) and eff[2] == 0.5


def test_batched_stats_bookkeeping_equals_the_per_iteration_one():
    """
    The device-resident loop writes n iterations of flag / statistics history at once (_update_stats_batch) and the
    stepwise loop one at a time (_update_stats_dictionary, a range of one).  The yardstick for both is the ORACLE's
    per-iteration writer (oracle/hgs_oracle.py update_stats, the restatement of _stats.py:130-190 that the recorded
    reference histories pin in test_oracle_golden.py): fresh history, an existing one, histories with holes (iterations
    recorded before a flag / group existed), new groups, stale groups, and an ``iter`` that lags the lists -- also by
    more than the range, where a list created now must cover the whole history.
    """
    import copy
    from oracle import hgs_oracle as orc
    rng = np.random.default_rng(5)

    def scenario(prep, n=7):
        a = Hologram(synth.random_target(1, (64, 64)), phase=np.zeros((64, 64), np.float32))
        a._update_flags("WGS-Kim", False, None, [])
        prep(a)
        b, c = copy.deepcopy(a), copy.deepcopy(a)
        o = orc.OracleHologram(synth.random_target(1, (64, 64)), phase=np.zeros((64, 64), np.float32))
        o.flags, o.stats, o.iter = copy.deepcopy(a.flags), copy.deepcopy(a.stats), a.iter
        hist = [bool(x) for x in rng.integers(0, 2, n)]
        groups = ["computational"] if "computational" in a.stats["stats"] or rng.integers(0, 2) else []
        per = [{g: dict(efficiency=float(rng.random()), uniformity=float(rng.random())) for g in groups} for _ in range(n)] if groups else None
        for k in range(n):
            o.flags["fixed_phase"] = a.flags["fixed_phase"] = hist[k]
            o.compute_stats = lambda stat_groups, k=k: {} if per is None else per[k]
            o.update_stats([])
            o.iter += 1
            a._update_stats_dictionary({} if per is None else per[k])
            a.iter += 1
        b._update_stats_batch(n, hist, per, groups)
        b.iter += n
        assert a.iter == b.iter == o.iter

        def same(x, y):
            if isinstance(x, dict):
                assert x.keys() == y.keys()
                for k in x:
                    same(x[k], y[k])
            else:
                assert len(x) == len(y), (len(x), len(y))
                for u, v in zip(x, y):
                    assert (u == v) or (isinstance(u, float) and isinstance(v, float) and np.isnan(u) and np.isnan(v)), (u, v)
        same(o.stats, a.stats)
        same(o.stats, b.stats)

    scenario(lambda h: None)                                            # fresh

    def with_history(h):
        for k in range(5):
            h.flags["fixed_phase"] = False
            h._update_stats_dictionary({"computational": dict(efficiency=0.1 * k, uniformity=0.5)} if k >= 2 else {})
            h.iter += 1
    scenario(with_history)

    def stale_and_new(h):
        with_history(h)
        h.stats["flags"]["old_flag"] = [1] * 3                          # a flag that is gone, list shorter than iter
        h.flags["brand_new_flag"] = "x"
        h.stats["stats"]["experimental_ij"] = {"efficiency": [0.3] * 5, "uniformity": [0.2] * 5}
    scenario(stale_and_new)

    def lagging_iter(h):
        with_history(h)
        h.iter = 3                                                      # lists longer than iter: entries are overwritten
    scenario(lagging_iter)

    def far_behind(h):
        with_history(h)
        with_history(h)
        h.iter = 1
        h.flags["brand_new_flag"] = "y"                                 # created now: must be as long as the history
    scenario(far_behind, n=3)


def test_false_run_is_capped_where_only_the_threshold_matters():
    h = Hologram(synth.random_target(1, (64, 64)), phase=np.zeros((64, 64), np.float32))
    h._update_flags("WGS-Kim", False, None, [], fix_phase_iteration=4)
    h.stats["flags"]["fixed_phase"] = [True] + [False] * 3
    assert h._false_run() == 3
    h.stats["flags"]["fixed_phase"] = [False] * 5000
    assert h._false_run() == 5                                          # >= fix_phase_iteration is all the engine asks
    h.stats["flags"]["fixed_phase"] = [False] * 10 + [np.nan, False, False]
    assert h._false_run() == 2 and h._false_run(skip_last=True) == 1


def test_convert_vector_knm_roundtrip():
    class Slm:
        shape = (1152, 1920)
        pitch = (8 / 0.78, 8 / 0.78)
    v = np.array([[0.01, -0.02], [0.005, 0.0]])
    knm = toolbox.convert_vector(v, "kxy", "knm", Slm(), (4096, 4096))
    back = toolbox.convert_vector(knm, "knm", "kxy", Slm(), (4096, 4096))
    np.testing.assert_allclose(back, v, atol=1e-15)
    np.testing.assert_allclose(toolbox.convert_vector((0, 0), "kxy", "knm", Slm(), (4096, 4096)).ravel(), [2048, 2048])


def test_quadratic_initial_phase_matches_reference():
    """reset_phase(quadratic_phase=...) (_hologram.py:480-527, :581-601) against values recorded from the reference."""
    meta, gold = load_golden("quadratic_phase")
    slm = tuple(meta["slm_shape"])
    h = Hologram(gold["target"].copy(), amp=gold["amp"].copy(), phase=synth.seed_phase(31, slm), slm_shape=slm)
    c, sd = h._get_target_moments_knm_norm()
    np.testing.assert_allclose(c, gold["center_knm_norm"], rtol=1e-12)
    np.testing.assert_allclose(sd, gold["std_knm_norm"], rtol=1e-12)
    np.testing.assert_allclose(h._get_quadratic_initial_phase(1), gold["q1"], rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(h._get_quadratic_initial_phase(1.7), gold["q17"], rtol=2e-6, atol=1e-6)
    h.reset_phase(quadratic_phase=True, random_phase=0)
    np.testing.assert_allclose(h.phase, gold["phase_quadratic"], rtol=2e-6, atol=1e-6)
    assert h.phase.dtype == np.float32
    # the flag form, added to a scaled random phase
    h.flags["quadratic_phase"] = 1.7
    h.reset_phase(random_phase=0)
    np.testing.assert_allclose(h.phase, gold["q17"], rtol=2e-6, atol=1e-6)
    # the scalar (uniform) amplitude has no image moments -- the reference fails there too
    g = Hologram(gold["target"].copy(), phase=synth.seed_phase(31, slm), slm_shape=slm)
    with pytest.raises(ValueError):
        g.reset_phase(quadratic_phase=True)


class _StubEngine:
    """Stands in for the HIP engine in host-logic tests: holds arrays, counts resets and closes."""

    def __init__(self, arrays):
        self.arrays = dict(arrays)
        self.closed = False
        self.resets = 0

    def get(self, which):
        return [self.arrays[which].copy()]

    def set(self, which, arr):
        self.arrays[which] = np.array(arr, copy=True)

    def reset_weights(self):
        pass

    def reset(self):
        self.resets += 1

    def close(self):
        self.closed = True


def test_reset_keeps_the_optimised_phase():
    """
    Hologram.reset(reset_phase=False) keeps the CURRENT phase (_hologram.py:442-478).  After optimize() the
    current phase lives on the device only; the engine survives the reset (hgs_reset) and keeps serving it.
    A released engine (MultiplaneHologram takes its children's) brings every device-fresh array home first.
    """
    h = Hologram(synth.random_target(1, (64, 64)), phase=np.zeros((64, 64), np.float32))
    stub = _StubEngine({L.PHASE: np.full((64, 64), 7.0, np.float32), L.WEIGHTS: h.weights.copy(),
                        L.AMP_FF: np.full((64, 64), 3.0, np.float32)})
    h._engine = stub
    h._mark_device_fresh(["phase", "weights"])          # what optimize_gs leaves behind
    h.reset(reset_phase=False)
    assert h._engine is stub and stub.resets == 1 and not stub.closed
    assert np.all(h.phase == 7.0) and h.amp_ff is None and h.phase_ff is None and h.iter == 0
    np.testing.assert_array_equal(h.weights, np.nan_to_num(h.target, nan=0))
    # reset_phase=True replaces it
    stub.arrays[L.PHASE][:] = 9.0
    h._mark_device_fresh(["phase"])
    h.reset(reset_phase=True)
    assert h._engine is stub and not np.any(h.phase == 9.0) and "phase" in h._upload
    # releasing the engine: phase, weights AND amp_ff come home; what the engine cannot serve becomes None
    h._mark_device_fresh(["phase", "amp_ff", "phase_ff"])
    stub.arrays[L.PHASE][:] = 5.0

    def get(which, _get=stub.get):
        if which == L.PHASE_FF:
            raise L.HgsError("phase_ff has not been computed")
        return _get(which)

    stub.get = get
    h._release_engine()
    assert stub.closed and h._engine is None
    assert np.all(h.phase == 5.0) and np.all(h.amp_ff == 3.0) and h.phase_ff is None


def test_reset_weights_are_lazy_but_follow_the_reference():
    """reset_weights (:603-614): weights = target with NaN -> 0.  The host copy is only built when read; a later
    set_target(reset_weights=False) must not change what the weights were."""
    t = synth.random_target(2, (32, 32))
    t[3, 4] = np.nan
    h = Hologram(t.copy(), phase=np.zeros((32, 32), np.float32))
    assert h._host["weights"] is None and h._weights_reset
    w0 = h.weights
    np.testing.assert_array_equal(w0, np.nan_to_num(h.target, nan=0))
    h.reset_weights()
    h.set_target(synth.random_target(3, (32, 32)), reset_weights=False)
    np.testing.assert_array_equal(h.weights, w0)                     # still those of the OLD target
    h.set_target(synth.random_target(4, (32, 32)), reset_weights=True)
    np.testing.assert_array_equal(h.weights, h.target)
    h.set_weights(w0)
    assert not h._weights_reset and "weights" in h._upload


def test_batch_targets_are_normalised_like_set_target():
    from slmsuite_amd.batch import normalize_targets
    t = synth.random_target(3, (2, 32, 32), 0.0, 5.0)
    t[0, 3, 4] = -t[0, 3, 4]
    t[1, 5, 6] = np.nan
    n = normalize_targets(t)
    assert n.dtype == np.float32 and np.all(n[~np.isnan(n)] >= 0) and np.isnan(n[1, 5, 6])
    for i in range(2):
        assert abs(float(np.sqrt(np.nansum(n[i].astype(np.float64) ** 2))) - 1) < 1e-6
    h = Hologram(t[0], phase=synth.seed_phase(1, (32, 32)))
    np.testing.assert_allclose(n[0], h.target, rtol=3e-7)
    # unit-norm input passes through bit-identically
    np.testing.assert_array_equal(normalize_targets(h.target), h.target)


ASAN_SCRIPT = r"""
import ctypes as C, sys
sys.path.insert(0, %r)
from slmsuite_amd import _lib as L
lib = L.load()
h = C.c_void_p()
# argument validation happens before any device work: these return status codes on every box
assert lib.hgs_create(None, C.byref(h)) == L.HGS_ERR_ARG
cfg = L.hgs_config(device=0, pad_h=64, pad_w=64, slm_h=32, slm_w=32, real_bytes=3, batch=1, n_spots=0, kind=0, n_monomials=0)
assert lib.hgs_create(C.byref(cfg), C.byref(h)) == L.HGS_ERR_ARG and not h.value
assert b"real_bytes" in lib.hgs_last_error()
cfg.real_bytes = 4
rc = lib.hgs_create(C.byref(cfg), C.byref(h))
if rc == L.HGS_OK:                        # a GPU is present: walk a few more entry points through the sanitizer
    import numpy as np
    bad = np.zeros(7, np.float32)
    assert lib.hgs_set_array(h, L.PHASE, bad.ctypes.data_as(C.c_void_p), bad.nbytes) == L.HGS_ERR_ARG
    assert lib.hgs_set_array(h, 99, bad.ctypes.data_as(C.c_void_p), bad.nbytes) == L.HGS_ERR_ARG
    ph = np.zeros((32, 32), np.float32)
    assert lib.hgs_set_array(h, L.PHASE, ph.ctypes.data_as(C.c_void_p), ph.nbytes) == 0
    assert lib.hgs_nearfield2farfield(h, 1) == 0 and lib.hgs_farfield2nearfield(h) == 0
    assert lib.hgs_farfield2nearfield(h) == L.HGS_ERR_STATE          # farfield consumed
    assert lib.hgs_destroy(h) == 0
else:
    assert rc == L.HGS_ERR_DEVICE and not h.value
for fn in (lib.hgs_sync, lib.hgs_reset_weights, lib.hgs_farfield2nearfield):
    assert fn(None) == L.HGS_ERR_ARG
assert lib.hgs_destroy(None) == 0
print("asan-ok")
"""


def test_asan_build_of_the_shim_is_clean():
    """The C-ABI error paths through the AddressSanitizer build of engine.hip (make -C slmsuite_amd/csrc asan)."""
    import subprocess
    import sys
    asan_lib = os.path.join(ROOT, "slmsuite_amd", "libhgs_asan.so")
    if not os.path.exists(os.path.join(ROOT, "slmsuite_amd", "libhgs.so")):
        pytest.skip("libhgs.so not built")
    # made on demand (a file target: nothing happens when it is up to date; one -O1 compile of engine.hip otherwise)
    mk = subprocess.run(["make", "-C", os.path.join(ROOT, "slmsuite_amd", "csrc"), "-j8", "asan"], capture_output=True, text=True)
    if mk.returncode != 0 or not os.path.exists(asan_lib):
        pytest.skip("ASan build of the shim failed: " + mk.stderr[-300:])
    rt = subprocess.run(["hipcc", "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(rt) or not os.path.exists(rt):
        pytest.skip("ASan runtime not found")
    # devices are hidden: the stock ROCm runtime cannot allocate device memory under the sanitizer's interceptors
    # (it needs the ASan-instrumented ROCm stack), and the host-side argument / state checks do not need a device
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:protect_shadow_gap=0", HGS_LIB=asan_lib,
               ROCR_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", ASAN_SCRIPT % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert "asan-ok" in p.stdout and p.returncode == 0, p.stderr[-2000:]
    assert "AddressSanitizer" not in p.stderr, p.stderr[-2000:]



# ---- bench.py --gpus N: never a line for fewer GPUs than asked for ------------------------------------------------------
def _run_bench(argv, env_extra=None):
    import subprocess
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True, text=True,
                          timeout=300)


def test_bench_gpus_n_fails_loudly_without_n_devices():
    """``bench.py --gpus 2`` on a box without two GPUs: non-zero exit, a reason on stderr, no JSON line on stdout."""
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs here: the launcher would run")
    r = _run_bench(["--gpus", "2", "--steps", "2", "--warmup", "1"])
    assert r.returncode != 0
    assert "--gpus 2" in r.stderr and ("GPU" in r.stderr)
    assert not any(line.startswith("{") for line in r.stdout.splitlines())


def test_bench_gpus_n_rejects_a_mismatched_launch():
    """A launcher that started another number of ranks than --gpus says must not produce a line either."""
    r = _run_bench(["--gpus", "4", "--steps", "2", "--warmup", "1"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr
    assert not any(line.startswith("{") for line in r.stdout.splitlines())


def test_bench_n_ranks_line_is_self_contained():
    """
    The N > 1 line has to carry its own scaling figure (the N = 1 default is another workload in another process) and the
    aggregate SURVEY 8(d) defines for cfg 3, "including the final RCCL gather".  The rank protocol of ``bench.py --gpus 2`` on
    this box -- self-launch under torch.distributed.run, gloo, the two ranks sharing "the device" -- against the stand-in
    engine (``--stub-engine``: a step is a sleep of 0.2 ms per hologram): rank 0 runs its shard alone first
    (``single_rank_same_job``) while rank 1 waits, ``scaling_efficiency`` = value / (N x that), and
    ``value_including_gather`` charges the gather to the K-step region and to the configured 50-iteration job.
    """
    import json
    r = _run_bench(["--gpus", "2", "--backend", "gloo", "--share-devices", "--no-roofline-pass", "--stub-engine",
                    "--steps", "10", "--warmup", "1", "--reps", "5", "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = lines[0]
    assert d["stub_engine"] is True and "STUB" in d["metric"]              # cannot be mistaken for a measurement
    assert d["n_gpus"] == 2 and d["config"]["holograms_per_gpu"] == 8
    solo = d["single_rank_same_job"]
    step = 8 * 2e-4                                                        # the stand-in's seconds per step of a rank
    assert 0.2 / step * 8 < solo["value"] <= 8 / step * 1.001, solo        # one rank: <= 8 holograms per 1.6 ms
    assert abs(d["scaling_efficiency"] - d["value"] / (2 * solo["value"])) < 1e-12
    assert 0.25 < d["scaling_efficiency"] <= 1.25, d["scaling_efficiency"]   # two sleeping ranks do not slow each other down (loaded box: wide)
    g = d["value_including_gather"]
    assert d["gather_ms"] > 0 and g["gather_ms"] == d["gather_ms"]
    wall = d["ms_per_step"] * 1e-3 * d["steps"]
    assert abs(g["value"] - 16 * d["steps"] / (wall + d["gather_ms"] * 1e-3)) < 1e-6 * g["value"]
    assert abs(g["job_of_50_iterations"] - 16 * 50 / (50 * d["ms_per_step"] * 1e-3 + d["gather_ms"] * 1e-3)) < 1e-6 * g["value"]
    assert g["value"] < g["job_of_50_iterations"] < d["value"]             # the gather weighs less on the longer job
    assert d["gathered"]["masks"] == 16 and d["gathered"]["verified_on_every_rank"] is True


def test_bench_stub_engine_is_only_the_rank_self_test():
    """``--stub-engine`` outside the gloo / shared-device self-test form is an argument error: no line, non-zero exit."""
    r = _run_bench(["--stub-engine", "--steps", "2", "--warmup", "1"])
    assert r.returncode != 0 and "self-test" in r.stderr
    assert not any(line.startswith("{") for line in r.stdout.splitlines())


def test_bench_plain_line_times_exactly_k_steps_and_dumps(tmp_path):
    """
    A plain run (no --full) times one region of exactly --steps steps and prints the headline fields, with nothing of the
    --full extras run: no roofline, no CPU baseline, no HIP-event repetitions.  --dump-outputs writes what the last step left
    (the stand-in's phase masks) as float .npy files.  Stand-in engine: a step is a sleep of 0.2 ms per hologram.
    """
    import json
    out = tmp_path / "dump"
    r = _run_bench(["--backend", "gloo", "--share-devices", "--no-roofline-pass", "--stub-engine",
                    "--steps", "25", "--warmup", "1", "--dump-outputs", str(out)])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 25 and d["repetitions"] == 1 and d["unit"] == "iterations/s" and d["higher_is_better"] is True
    assert 0.2 <= d["ms_per_step"] < 20, d["ms_per_step"]                  # 25 sleeps of 0.2 ms in the region, nothing else
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and "engine_default_path" not in d
    ph = np.load(out / "phase.npy")
    assert ph.dtype == np.float32 and ph.shape == (1, 16, 24) and np.all(ph == 0.0)


def test_bench_dump_outputs_caps_the_size_with_a_fixed_sample(tmp_path):
    """Arrays beyond their share of the 64 MB are replaced by the same seeded sample in every run; dtypes stay float32 /
    float64; small arrays are written whole."""
    sys.path.insert(0, ROOT)
    import bench
    big = np.arange(12_000_000, dtype=np.float64)                  # 96 MB
    small = np.linspace(0, 1, 1000).astype(np.float32)
    for d in ("a", "b"):
        bench.dump_outputs({"weights": big, "phase": small, "amp_ff": big.astype(np.float32)}, str(tmp_path / d))
    total = 0
    for name in ("weights", "phase", "amp_ff"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        np.testing.assert_array_equal(a, b)
        total += os.path.getsize(tmp_path / "a" / f"{name}.npy")
    assert total <= 64 * 10 ** 6
    w = np.load(tmp_path / "a" / "weights.npy")
    assert w.dtype == np.float64 and 0 < w.size < big.size and np.all(np.diff(w) > 0)   # sorted, distinct positions
    assert np.load(tmp_path / "a" / "amp_ff.npy").dtype == np.float32
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "phase.npy"), small)


def test_update_flags_precedence_and_verbose_print(capsys):
    """_update_flags (_hologram.py:1370-1424): method defaults only where no value exists yet (flags persist between calls),
    keyword flags over both, stat_groups / feedback checked against FEEDBACK_OPTIONS right before they are stored (a rejected
    name leaves the earlier updates in place); verbose > 1 prints the flags the method reads."""
    h = Hologram(synth.random_target(1, (64, 64)), phase=np.zeros((64, 64), np.float32))
    h._update_flags("WGS-Kim", False, None, [], feedback_exponent=0.5)
    assert h.flags["method"] == "WGS-Kim" and h.flags["feedback_exponent"] == 0.5 and h.flags["fix_phase_iteration"] == 10
    assert h.flags["fixed_phase"] is False and h.flags["stat_groups"] == [] and h.flags["feedback"] == "computational"
    h.flags["fixed_phase"] = True
    h._update_flags("WGS-Leonardo", False, "computational", ["computational"])
    assert h.flags["feedback_exponent"] == 0.5 and h.flags["fixed_phase"] is True            # kept: defaults never override
    assert h.flags["stat_groups"] == ["computational"]
    with pytest.raises(ValueError, match="Statistics group 'nope'"):
        h._update_flags("GS", False, None, ["nope"], some_flag=3)
    assert h.flags["method"] == "GS" and h.flags["some_flag"] == 3 and h.flags["stat_groups"] == ["computational"]
    with pytest.raises(ValueError, match="Feedback 'bad'"):
        h._update_flags("GS", False, "bad", ["computational_spot"])
    assert h.flags["stat_groups"] == ["computational_spot"] and h.flags["feedback"] == "computational"
    with pytest.raises(ValueError, match="Unrecognized method 'XYZ'"):
        h._update_flags("XYZ", False, None, [])
    capsys.readouterr()
    h._update_flags("WGS-Kim", 2, None, [], fix_phase_iteration=7)
    out = capsys.readouterr().out
    assert "Optimizing with 'WGS-Kim' using the following method-specific flags:" in out
    assert "'fix_phase_iteration': 7" in out and "'method'" not in out and "'some_flag'" not in out


def test_smallest_distance_is_exact_without_scipy_spatial():
    """toolbox.smallest_distance (toolbox/__init__.py:1127-1250 in the reference): the sorted sweep against all pairs, for
    the three metrics, on random points, integer points with coincidences, grids and points on one line -- and without
    importing scipy.spatial (180 ms of a process' first SpotHologram)."""
    import subprocess
    from slmsuite_amd.holography.toolbox import smallest_distance
    rng = np.random.default_rng(5)

    def brute(v, metric):
        d = np.abs(v[:, :, None] - v[:, None, :])
        m = {"chebyshev": d.max(axis=0), "euclidean": np.sqrt((d * d).sum(axis=0)), "cityblock": d.sum(axis=0)}[metric]
        m[np.arange(v.shape[1]), np.arange(v.shape[1])] = np.inf
        return float(m.min())

    grid = np.stack(np.meshgrid(np.arange(20) * 64.0, np.arange(20) * 48.0)).reshape(2, -1)
    cases = [rng.random((2, 2)), rng.random((2, 3)) * 10, rng.random((2, 700)) * 1000, rng.integers(0, 40, (2, 500)).astype(float),
             grid, np.stack((np.zeros(300), rng.random(300) * 50)), np.stack((rng.random(300) * 50, np.ones(300)))]
    for v in cases:
        for metric in ("chebyshev", "euclidean", "cityblock"):
            assert abs(smallest_distance(v, metric) - brute(v, metric)) <= 1e-12 * max(1.0, brute(v, metric))
    assert smallest_distance(np.zeros((2, 1))) == np.inf
    with pytest.raises(ValueError):
        smallest_distance(grid, "minkowski")
    code = ("import sys, numpy as np; from slmsuite_amd.holography.toolbox import smallest_distance; "
            "smallest_distance(np.stack(np.meshgrid(np.arange(32.), np.arange(32.))).reshape(2, -1)); "
            "sys.exit(1 if 'scipy.spatial' in sys.modules else 0)")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
