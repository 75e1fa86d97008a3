"""
GPU tests of get_display(): the gray levels the engine forms from its device phase equal the reference's
``SimulatedSLM.set_phase`` (the fixtures of tests/golden/display_*.npz) and, at shapes the fixtures do not hold, the NumPy
restatement tests/display_ref.py that test_display_cpu.py pins to those fixtures.  Every comparison is array equality:
no tolerance, no excluded pixel.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import display_ref as ref
from conftest import ROOT, dispatch_of
from slmsuite_amd import _lib as L
from slmsuite_amd import synth
from slmsuite_amd.batch import HologramBatch
from slmsuite_amd.engine import Engine
from slmsuite_amd.hardware import DisplaySLM, SimpleFourierSLM
from slmsuite_amd.holography.algorithms import CompressedSpotHologram, Hologram, MultiplaneHologram, SpotHologram

pytestmark = pytest.mark.gpu

FLOAT_CASES = [(n, c) for n, c in ref.fixtures() if "phase" in c]
SHORT, LONG = 0.78 / 0.9, 0.78 / 0.7          # phase_scaling below and above one (the fixtures' values)
_ENGINES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def engine_for(slm_shape, dtype, batch=1, pad=(64, 64)):
    """One small padded-grid engine per (SLM shape, precision, batch), kept for the module: get_display reads the phase only."""
    key = (tuple(slm_shape), np.dtype(dtype).str, batch, pad)
    if key not in _ENGINES:
        _ENGINES[key] = Engine(pad, slm_shape, dtype, batch=batch)
    e = _ENGINES[key]
    e.clear_propagation_kernel()
    e.set_display_correction(None)
    return e


def rname(dtype):
    return {4: "float", 8: "double"}[np.dtype(dtype).itemsize]


def run(e, phase, bits=8, s=1.0, correction=None, kernel=None, **kw):
    e.set(L.PHASE, phase)
    if kernel is not None:
        e.set(L.PROP_KERNEL, kernel)
    e.set_display_correction(correction)
    dispatch_of(e)
    out = e.get_display(bitdepth=bits, phase_scaling=s, include_propagation=kernel is not None, **kw)
    rec = dispatch_of(e)
    assert rec.count("phase_display_kernel", R=rname(e.dtype), BITS=16 if bits > 8 else 8) == 1 and len(rec.records) == 1, rec
    assert out.dtype == (np.uint16 if bits > 8 else np.uint8) and out.shape == (e.batch,) + e.slm_shape
    return out


# ---- 1. fixtures ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,c", FLOAT_CASES, ids=[n for n, _ in FLOAT_CASES])
def test_fixture(name, c):
    bits, s, corr, kern = ref.case_args(c)
    e = engine_for(c["phase"].shape, c["phase"].dtype)
    np.testing.assert_array_equal(run(e, c["phase"], bits, s, corr, kern)[0], c["display"])


def test_fixtures_run_in_both_precisions():
    assert {c["phase"].dtype.itemsize for _, c in FLOAT_CASES} == {4, 8}


# ---- 2. tails: every residue of the pixel count modulo the four pixels of a lane ------------------------------------------------
TAIL_SHAPES = [(5, 3), (31, 35), (30, 35), (33, 47), (32, 48)]


@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_tails(shape, dtype):
    src = open(os.path.join(ROOT, "slmsuite_amd", "csrc", "display_kernels.hpp")).read()
    pix = int(re.search(r"constexpr int DISP_PIX = (\d+);", src).group(1))           # pixels per lane, whatever it is
    assert {sh[0] * sh[1] % pix for sh in TAIL_SHAPES} == set(range(pix))
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    e = engine_for(shape, dtype)
    corr = rng.uniform(-20, 20, size=shape)
    for phase in (rng.uniform(-np.pi, np.pi, size=shape).astype(dtype), rng.uniform(-300, 300, size=shape).astype(dtype)):
        # the last pixel decides the branch: it alone holds the extreme
        phase.flat[-1] = -40
        for bits in (8, 16):
            for c in (None, corr):
                for s in (1.0, SHORT, LONG):
                    np.testing.assert_array_equal(run(e, phase, bits, s, c)[0], ref.display_of(phase, bits, s, c),
                                                  err_msg=f"bits {bits} s {s} corr {c is not None}")


# ---- 3. the extremes across blocks, at the cfg 2 SLM size ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    shape = (1152, 1920)
    rng = np.random.default_rng(3)
    x = rng.uniform(0.01, 6.2, size=shape)                       # every y < 0
    ks = (101, 37, 7, 200)
    x.flat[5:9] = [ref.near_tie_x(k) for k in ks]                # near ties in the first block
    e = Engine((2048, 2048), shape, np.float32)
    yield e, x
    e.close()


@pytest.mark.parametrize("where", ["last", "middle", "first", "none"])
def test_extremes_across_blocks(big, where):
    e, x = big
    x = x.copy()
    S = x.size
    at = {"last": S - 1, "middle": S // 2 + 1, "first": 0, "none": None}[where]
    if at is not None:
        x.flat[at] = -3.0                                        # the only positive y: shift 512
    phase, corr = ref.split_mask(x, np.float32)
    want = ref.levels_of(x, 8, 1.0)
    assert list(want.flat[5:9]) == ([154, 218, 248, 55] if at is None else [153, 217, 247, 55])
    np.testing.assert_array_equal(run(e, phase, 8, 1.0, corr)[0], want)
    if where in ("last", "none"):                                # the other branch pair, decided by the same pixel
        want = ref.levels_of(x, 10, SHORT)
        assert ref.branch_of(x, 10, SHORT) == ("mod" if at is not None else "inbounds")
        np.testing.assert_array_equal(run(e, phase, 10, SHORT, corr)[0], want)


# ---- 4. batch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_batch_members_keep_their_own_extremes(dtype):
    shape = (33, 47)                                             # 1551 pixels: members 1 and 2 start off a quad boundary
    rng = np.random.default_rng(11)
    phases = np.stack([rng.uniform(-3.1, 3.1, size=shape), rng.uniform(-50, 50, size=shape),
                       rng.uniform(-3.1, 3.1, size=shape)]).astype(dtype)
    phases[2, -1, -1] = -3.5                                     # one pixel below -pi
    kern = rng.uniform(-1, 1, size=shape).astype(dtype)
    corr = rng.uniform(-1e-3, 1e-3, size=shape)
    eb, e1 = engine_for(shape, dtype, batch=3), engine_for(shape, dtype)
    for bits, s in ((8, 1.0), (16, 1.0), (8, SHORT), (10, LONG)):
        branches = {ref.branch_of(ref.mask_of(p), bits, s) for p in phases}
        assert branches == ({"plain", "shift"} if s == 1 else {"inbounds", "mod"} if s < 1 else {"mod"})
        got = run(eb, phases, bits, s)
        for b in range(3):
            np.testing.assert_array_equal(got[b], run(e1, phases[b], bits, s)[0])
            np.testing.assert_array_equal(got[b], ref.display_of(phases[b], bits, s))
    got = run(eb, phases, 8, 1.0, corr, kern)                    # kernel and correction are shared, indexed per hologram
    for b in range(3):
        np.testing.assert_array_equal(got[b], ref.display_of(phases[b], 8, 1.0, corr, kern))


def test_hologram_batch_displays():
    shape, slm_shape = (64, 64), (30, 35)
    phases = np.stack([synth.seed_phase(k, slm_shape) for k in range(3)])
    hb = HologramBatch(shape, slm_shape, synth.random_target(2, shape), phases, streams=2)
    hb.optimize("WGS-Leonardo", maxiter=2)
    corr = np.random.default_rng(5).uniform(-20, 20, size=slm_shape)
    got = hb.displays(bitdepth=10, phase_scaling=LONG, phase_correction=corr)
    assert got.shape == (3,) + slm_shape and got.dtype == np.uint16
    for b, p in enumerate(hb.phases()):
        np.testing.assert_array_equal(got[b], ref.display_of(p, 10, LONG, corr))
    sent = []
    for e in hb.engines:                                         # an unchanged correction is not uploaded again, a new one is
        e.set_display_correction = (lambda arr, up=e.set_display_correction: (sent.append(arr), up(arr))[1])
    np.testing.assert_array_equal(hb.displays(bitdepth=10, phase_scaling=LONG, phase_correction=corr), got)
    assert sent == []
    plain = hb.displays(bitdepth=10, phase_scaling=LONG)
    assert len(sent) == len(hb.engines) and all(a is None for a in sent)
    for b, p in enumerate(hb.phases()):
        np.testing.assert_array_equal(plain[b], ref.display_of(p, 10, LONG))
    hb.close()


# ---- 5. kind 1 ---------------------------------------------------------------------------------------------------------------------
def test_compressed_hologram():
    slm = DisplaySLM((70, 93), bitdepth=10, wav_design_um=0.7)
    slm.source["phase"] = np.random.default_rng(8).uniform(-5, 5, size=slm.shape)
    v = np.vstack([0.03 * (synth.uniform01(51, (21,), k) - 0.5) for k in range(2)])
    h = CompressedSpotHologram(v, basis="kxy", cameraslm=SimpleFourierSLM(slm))
    h.optimize("WGS-Leonardo", maxiter=3, verbose=False)
    assert h._engine.kind == 1
    got = h.get_display(slm)
    np.testing.assert_array_equal(got, ref.display_of(h.phase, 10, slm.phase_scaling, slm.source["phase"]))
    np.testing.assert_array_equal(got, DisplaySLM.set_phase(slm, h.get_phase()))


# ---- 6. class level ----------------------------------------------------------------------------------------------------------------
def check_routes(h, slm, include_propagation=False):
    corr = slm.source.get("phase")
    got = h.get_display(slm, include_propagation=include_propagation)
    mask = h.get_phase(include_propagation=include_propagation)
    assert mask.dtype == h.dtype
    want = ref.levels_of(mask.astype(np.float64) + (0 if corr is None else corr), slm.bitdepth, slm.phase_scaling)
    np.testing.assert_array_equal(got, want)
    host = DisplaySLM(slm.shape, bitdepth=slm.bitdepth, wav_design_um=slm.wav_design_um)
    host.source = slm.source
    np.testing.assert_array_equal(got, host.set_phase(mask))
    if not include_propagation:
        out = slm.set_phase(h)
        assert out is slm.display
        np.testing.assert_array_equal(got, out)
        assert slm.phase.dtype == np.float64
        np.testing.assert_array_equal(slm.phase, host.phase)
    return got


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("bits,design", [(8, None), (10, 0.9), (16, 0.7)])
def test_class_level_routes(dtype, bits, design):
    shape, slm_shape = (128, 128), (33, 47)
    slm = DisplaySLM(slm_shape, bitdepth=bits, wav_design_um=design)
    kern = (0.3 * synth.seed_phase(9, slm_shape)).astype(dtype)
    h = SpotHologram.make_rectangular_array(shape, (4, 4), (12, 12), basis="knm", slm_shape=slm_shape, dtype=dtype,
                                            phase=synth.seed_phase(7, slm_shape).copy(), propagation_kernel=kern)
    h.optimize("WGS-Leonardo", maxiter=5, verbose=False)
    h.get_display(slm)
    assert "phase" in h._stale                                   # the device route downloads no phase
    plain = check_routes(h, slm)
    slm.source["phase"] = np.random.default_rng(1).uniform(-20, 20, size=slm_shape)
    with_corr = check_routes(h, slm)
    assert not np.array_equal(plain, with_corr)
    np.testing.assert_array_equal(h.get_display(slm, phase_correct=False), plain)
    check_routes(h, slm, include_propagation=True)
    h.optimize("CG", maxiter=3, verbose=False)
    check_routes(h, slm)
    check_routes(h, slm, include_propagation=True)
    # keyword form, without an SLM object
    np.testing.assert_array_equal(h.get_display(bitdepth=bits, phase_scaling=slm.phase_scaling, phase_correction=slm.source["phase"]),
                                  h.get_display(slm))


def test_host_phase_and_correction_bookkeeping():
    slm_shape = (31, 35)
    slm = DisplaySLM(slm_shape, bitdepth=8)
    h = Hologram(synth.random_target(1, (64, 64)), slm_shape=slm_shape, phase=synth.seed_phase(1, slm_shape))
    h.optimize("GS", maxiter=2, verbose=False)
    e = h._engine
    sent = []
    upload = e.set_display_correction
    e.set_display_correction = lambda arr: (sent.append(arr), upload(arr))[1]
    first = h.get_display(slm)
    assert len(sent) == 1 and sent[0] is None                    # (no correction yet: cleared once)
    # a phase assigned on the host and not yet uploaded is honoured
    new = np.random.default_rng(2).uniform(-9, 9, size=slm_shape).astype(np.float32)
    h.phase = new
    assert "phase" in h._upload
    np.testing.assert_array_equal(h.get_display(slm), ref.display_of(new))
    assert "phase" not in h._upload and "phase" not in h._stale and len(sent) == 1
    # a correction is sent when it appears and when it changes, not when it stays
    slm.source["phase"] = np.random.default_rng(3).uniform(-20, 20, size=slm_shape)
    a = h.get_display(slm)
    np.testing.assert_array_equal(a, ref.display_of(new, correction=slm.source["phase"]))
    np.testing.assert_array_equal(h.get_display(slm), a)
    assert len(sent) == 2
    slm.source["phase"] = slm.source["phase"] + 1.0
    np.testing.assert_array_equal(h.get_display(slm), ref.display_of(new, correction=slm.source["phase"]))
    assert len(sent) == 3
    slm.source["phase"][:] = 0.25                                # in place
    np.testing.assert_array_equal(h.get_display(slm), ref.display_of(new, correction=np.full(slm_shape, 0.25)))
    assert len(sent) == 4
    del slm.source["phase"]
    np.testing.assert_array_equal(h.get_display(slm), ref.display_of(new))
    assert len(sent) == 5 and sent[-1] is None
    assert not np.array_equal(first, a)


def test_a_new_engine_is_sent_the_correction_again():
    """The record of what was uploaded lives with the engine: after the engine is released and rebuilt -- whatever address
    the new object gets -- an unchanged correction goes up again."""
    slm_shape = (31, 35)
    slm = DisplaySLM(slm_shape, bitdepth=8)
    slm.source["phase"] = np.random.default_rng(4).uniform(-20, 20, size=slm_shape)
    h = Hologram(synth.random_target(1, (64, 64)), slm_shape=slm_shape, phase=synth.seed_phase(1, slm_shape))
    h.optimize("GS", maxiter=2, verbose=False)
    first = h.get_display(slm)
    assert not np.array_equal(first, h.get_display(slm, phase_correct=False))
    for _ in range(8):                                           # (several rebuilds: some land on the old object's address)
        old = h._engine
        h._release_engine()
        assert h._engine is None
        np.testing.assert_array_equal(h.get_display(slm), first)
        assert h._engine is not old
    mp = MultiplaneHologram([h])                                 # releases the child's engine (a new amplitude)
    np.testing.assert_array_equal(mp.get_display(slm), first)


def test_refresh_forces_an_unseen_edit_up():
    slm_shape = (31, 35)
    slm = DisplaySLM(slm_shape, bitdepth=8)
    corr = slm.source["phase"] = np.random.default_rng(5).uniform(-20, 20, size=slm_shape)
    h = Hologram(synth.random_target(1, (64, 64)), slm_shape=slm_shape, phase=synth.seed_phase(2, slm_shape))
    phase = np.array(h.phase)
    np.testing.assert_array_equal(h.get_display(slm), ref.display_of(phase, correction=corr))
    before = corr.copy()
    corr[7, 3] += 9.0                                            # in place, in a row the fingerprint does not sample
    np.testing.assert_array_equal(h.get_display(slm), ref.display_of(phase, correction=before))
    h.refresh_farfield_inputs()
    np.testing.assert_array_equal(h.get_display(slm), ref.display_of(phase, correction=corr))


def test_multiplane_asks_its_first_child():
    slm_shape = (30, 35)
    kids = [SpotHologram.make_rectangular_array((64, 64), (3, 3), (8, 8), basis="knm", slm_shape=slm_shape,
                                                phase=synth.seed_phase(4, slm_shape).copy()) for _ in range(2)]
    mp = MultiplaneHologram(kids)
    mp.optimize("GS", maxiter=2, verbose=False)
    slm = DisplaySLM(slm_shape, bitdepth=10)
    np.testing.assert_array_equal(mp.get_display(slm), ref.display_of(mp.phase, 10))
    np.testing.assert_array_equal(mp.get_display(slm), slm.set_phase(mp.get_phase()))


# ---- 7. get=False ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 12])
def test_device_tensor(bits):
    import torch
    shape = (33, 47)
    phase = np.random.default_rng(6).uniform(-30, 30, size=(2,) + shape).astype(np.float32)
    e = engine_for(shape, np.float32, batch=2)
    host = run(e, phase, bits, LONG)
    dev = e.get_display(bitdepth=bits, phase_scaling=LONG, get=False)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == (torch.uint16 if bits > 8 else torch.uint8)
    np.testing.assert_array_equal(dev.cpu().numpy(), host)
    h = Hologram(synth.random_target(1, (64, 64)), slm_shape=shape, phase=phase[0])
    t = h.get_display(bitdepth=bits, phase_scaling=LONG, get=False)
    assert isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == shape
    np.testing.assert_array_equal(t.cpu().numpy(), host[0])


# ---- 8. loud errors ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    shape = (30, 35)
    e = engine_for(shape, np.float32)
    phase = np.random.default_rng(7).uniform(-3, 3, size=shape).astype(np.float32)
    e.set(L.PHASE, phase)
    for bits in (0, 17, -1):
        with pytest.raises(ValueError, match="bitdepth"):
            e.get_display(bitdepth=bits)
    for s in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="phase_scaling"):
            e.get_display(phase_scaling=s)
    prm = L.hgs_display_params(phase_scaling=1.0, bitdepth=8, include_propagation=0, phase_correct=1, reserved=0)
    buf = np.zeros(2 * phase.size + 8, dtype=np.uint8)
    for nbytes in (phase.size - 1, phase.size + 1, 2 * phase.size, 0):
        assert e.lib.hgs_get_display(e._h, C.byref(prm), buf.ctypes.data_as(C.c_void_p), nbytes) == L.HGS_ERR_ARG
        assert b"bad size" in e.lib.hgs_last_error()
    prm.bitdepth = 9                                             # 16-bit levels: twice the bytes
    assert e.lib.hgs_get_display(e._h, C.byref(prm), buf.ctypes.data_as(C.c_void_p), phase.size) == L.HGS_ERR_ARG
    assert e.lib.hgs_get_display(e._h, C.byref(prm), buf.ctypes.data_as(C.c_void_p), 2 * phase.size) == L.HGS_OK
    assert e.lib.hgs_get_display(e._h, None, buf.ctypes.data_as(C.c_void_p), phase.size) == L.HGS_ERR_ARG
    assert e.lib.hgs_get_display(e._h, C.byref(prm), None, 2 * phase.size) == L.HGS_ERR_ARG
    assert not buf[2 * phase.size:].any()                        # nothing past the levels was written
    # a correction of the wrong size, at both layers
    with pytest.raises(ValueError):
        e.set_display_correction(np.zeros((30, 36)))
    bad = np.zeros(phase.size + 1)
    for nbytes in (bad.nbytes, 4 * phase.size, 8):
        assert e.lib.hgs_set_array(e._h, L.DISPLAY_CORRECTION, bad.ctypes.data_as(C.c_void_p), nbytes) == L.HGS_ERR_ARG
        assert b"display correction" in e.lib.hgs_last_error()
    assert e.lib.hgs_get_array(e._h, L.DISPLAY_CORRECTION, bad.ctypes.data_as(C.c_void_p), 8 * phase.size) == L.HGS_ERR_ARG
    # a refused correction leaves none behind; include_propagation without a kernel is the plain phase plus pi, as in the reference
    np.testing.assert_array_equal(e.get_display(include_propagation=True)[0], ref.display_of(phase))
    np.testing.assert_array_equal(e.get_display()[0], ref.display_of(phase))
