"""
CPU tests of get_display()'s host side: the NumPy restatement the GPU tests compare against (tests/display_ref.py) and the
host route of ``DisplaySLM.set_phase`` reproduce every fixture recorded from the reference's ``SimulatedSLM.set_phase``
(tests/golden/display_*.npz, tools/make_golden_display.py) exactly; the ctypes image of ``hgs_display_params`` follows the
header; and without a GPU the call fails loudly.  No compute calls.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import display_ref as ref
from conftest import ROOT
from slmsuite_amd import _lib as L
from slmsuite_amd import synth
from slmsuite_amd.hardware import DisplaySLM, SimpleSLM
from slmsuite_amd.holography.algorithms import Hologram

CASES = ref.fixtures()
FLOAT_CASES = [(n, c) for n, c in CASES if "phase" in c]
INT_CASES = [(n, c) for n, c in CASES if "phase" not in c]
ids = lambda cases: [n for n, _ in cases]       # noqa: E731


def slm_for(c):
    """A DisplaySLM with the case's bit depth, scaling and correction (wav_um / wav_design_um reproduces the recorded scaling)."""
    bits, s, corr, _ = ref.case_args(c)
    shape = c["display"].shape
    slm = DisplaySLM(shape, wav_um=0.78, bitdepth=bits, wav_design_um=None if s == 1 else {0.78 / 0.9: 0.9, 0.78 / 0.7: 0.7}[s])
    assert slm.phase_scaling == s
    if corr is not None:
        slm.source["phase"] = corr
    return slm


def test_fixtures_cover_the_issue():
    """Bit depths, scalings and branches the fixtures must hold -- read off the data, not the case names."""
    seen = set()
    for _, c in FLOAT_CASES:
        bits, s, corr, kern = ref.case_args(c)
        mask = ref.mask_of(c["phase"], kern, corr)
        seen.add((bits, round(s, 3), corr is not None, ref.branch_of(mask, bits, s)))
        assert c["display"].shape[0] <= 33 and c["display"].shape[1] <= 47
    for bits in (1, 8, 10, 16):
        assert (bits, 1.0, False, "plain") in seen and (bits, 1.0, True, "shift") in seen
        assert (bits, 0.867, False, "inbounds") in seen and (bits, 0.867, True, "mod") in seen
        assert (bits, 1.114, False, "mod") in seen and (bits, 1.114, True, "mod") in seen
    assert {str(c["phase"].dtype) for _, c in FLOAT_CASES} == {"float32", "float64"}
    # the shift is observable: the same four near-tie pixels, alone and next to one negative mask value
    by = dict(FLOAT_CASES)
    for tag in ("f32", "f64"):
        assert list(by[f"display_ties:alone_{tag}"]["display"].flat[:4]) == [154, 218, 248, 55]
        assert list(by[f"display_ties:shifted_{tag}"]["display"].flat[:4]) == [153, 217, 247, 55]
    zero = by["display_unit:zero_f32"]
    assert np.max(ref.mask_of(zero["phase"]) * -(256 / 2 / np.pi)) == 0          # one pixel exactly 0: max 0, shift 0
    y = ref.mask_of(by["display_ties:alone_f64"]["phase"], None, by["display_ties:alone_f64"]["correction"]) * -(256 / 2 / np.pi)
    assert np.sum(y * 2 == np.rint(y * 2)) >= 4 and np.sum(y == np.rint(y)) == 0  # exact half-integers


@pytest.mark.parametrize("name,c", FLOAT_CASES, ids=ids(FLOAT_CASES))
def test_restatement_reproduces_fixture(name, c):
    bits, s, corr, kern = ref.case_args(c)
    got = ref.display_of(c["phase"], bits, s, corr, kern)
    assert got.dtype == c["display"].dtype
    np.testing.assert_array_equal(got, c["display"])
    if "given" in c:             # a padded mask: its centred crop is the mask of `phase`
        given = c["given"]
        assert given.shape != c["phase"].shape
        from slmsuite_amd.holography import toolbox
        np.testing.assert_array_equal(toolbox.unpad(given, c["phase"].shape), c["phase"] + c["phase"].dtype.type(np.pi))


@pytest.mark.parametrize("name,c", FLOAT_CASES, ids=ids(FLOAT_CASES))
def test_display_slm_float_route(name, c):
    _, _, _, kern = ref.case_args(c)
    slm = slm_for(c)
    given = c["given"] if "given" in c else c["phase"] + (c["phase"].dtype.type(np.pi) if kern is None else kern)
    before = given.copy()
    out = slm.set_phase(given)
    assert out is slm.display and out.dtype == slm.dtype == c["display"].dtype
    np.testing.assert_array_equal(out, c["display"])
    assert slm.phase.dtype == np.float64
    np.testing.assert_array_equal(slm.phase, c["slm_phase"])
    np.testing.assert_array_equal(given, before)           # the caller's array is not scaled in place
    if "correction" in c:                                   # phase_correct=False leaves the correction out
        plain = slm.set_phase(given, phase_correct=False)
        np.testing.assert_array_equal(plain, ref.levels_of(np.asarray(before, dtype=np.float64), *ref.case_args(c)[:2]))


@pytest.mark.parametrize("name,c", INT_CASES, ids=ids(INT_CASES))
def test_display_slm_integer_route(name, c):
    slm = slm_for(c)
    out = slm.set_phase(c["given"])
    assert c["given"].shape != c["display"].shape or "padded" not in name
    np.testing.assert_array_equal(out, c["display"])
    np.testing.assert_array_equal(slm.phase, c["slm_phase"])
    assert out.dtype == c["display"].dtype


def test_display_slm_integer_errors():
    slm = DisplaySLM((9, 14), bitdepth=10)
    assert slm.dtype == np.uint16 and slm.bitresolution == 1024 and slm.phase_correct is True and slm.phase_scaling == 1
    with pytest.raises(TypeError, match="Unexpected integer type"):
        slm.set_phase(np.zeros((9, 14), dtype=np.uint8))
    with pytest.raises(TypeError, match="Unexpected integer type"):
        slm.set_phase(np.zeros((9, 14), dtype=np.int64))
    levels = np.zeros((9, 14), dtype=np.uint16)
    levels[3, 3] = 1024
    with pytest.raises(TypeError, match="within the bitdepth"):
        slm.set_phase(levels)
    levels[3, 3] = 1023
    assert slm.set_phase(levels)[3, 3] == 1023
    with pytest.raises(ValueError, match="too small"):
        slm.set_phase(np.zeros((8, 14)))
    assert isinstance(slm, SimpleSLM) and not hasattr(SimpleSLM((4, 4)), "set_phase")      # SimpleSLM itself is unchanged


def test_display_params_match_header():
    hdr = open(os.path.join(ROOT, "include", "hgs.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\} hgs_display_params;", hdr, re.S).group(1)
    fields = re.findall(r"\b(double|int32_t)\s+([a-z_]+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    ctype = {"double": C.c_double, "int32_t": C.c_int32}
    assert [(n, ctype[t]) for t, n in fields] == list(L.hgs_display_params._fields_)
    assert C.sizeof(L.hgs_display_params) == 24
    assert int(re.search(r"HGS_DISPLAY_CORRECTION\s*=\s*(\d+)", hdr).group(1)) == L.DISPLAY_CORRECTION == 20
    assert {"hgs_get_display", "hgs_get_display_device"} <= set(L.EXPORTS)
    assert re.search(r"HGS_K_COUNT = 7\b", hdr) and 'v = "hgs 0.2 gfx950"' in open(
        os.path.join(ROOT, "slmsuite_amd", "csrc", "engine.hip")).read()


def test_get_display_has_no_cpu_route():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    h = Hologram(synth.random_target(1, (64, 64)), phase=synth.seed_phase(1, (64, 64)))
    with pytest.raises(L.HgsError):
        h.get_display(DisplaySLM((64, 64)))
    with pytest.raises(L.HgsError):
        DisplaySLM((64, 64)).set_phase(h)
