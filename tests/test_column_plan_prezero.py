"""
``prezero_ok`` of ``slmsuite_amd/csrc/column_plan.hpp`` without a GPU: the pure predicate that says whether the row launch ahead
of a body may store the zero H of the empty columns instead of their G (``RowArgs::zero_mask``) and the body's column launch may
walk past empty half tiles (``ColArgs::h_prezeroed``).  ``tests/column_plan_prezero_host.cpp`` forms the facts of a body, plans
it with ``plan_column_pass`` and prints the predicate; the table below names every fact that must turn it off.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS, LEONARDO, KIM, NOGRETTE = range(4)


def _compiler():
    for cxx in ("c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/bin/amdclang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ / clang++) on this machine")
    exe = str(tmp_path_factory.mktemp("column_plan_prezero") / "column_plan_prezero_host")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "slmsuite_amd", "csrc"),
                        os.path.join(ROOT, "tests", "column_plan_prezero_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _ask(exe, **facts):
    line = " ".join(f"{k}={int(v)}" for k, v in facts.items())
    r = subprocess.run([exe], input=line + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ok, family, col_flags, phase_mode = r.stdout.split()
    return dict(ok=int(ok), family=family, col_flags=int(col_flags), phase_mode=int(phase_mode))


def test_true_for_the_headline_and_the_batch(host):
    """cfg 2 (one hologram, 32 active columns of 4096, column lists off) and cfg 3 (a batch of eight): bodies with and without a
    weight update, GS as well."""
    for batch in (1, 8):
        for method, upd in ((LEONARDO, 1), (LEONARDO, 0), (GS, 0), (KIM, 0)):
            got = _ask(host, B=batch, method=method, do_update=upd)
            assert got == dict(ok=1, family="tile2", col_flags=1, phase_mode=0), (batch, method, upd, got)
    # (a quarter of the columns active is the most the flags go with)
    assert _ask(host, n_active=1024)["ok"] == 1
    assert _ask(host, n_active=1025)["ok"] == 0


FALSE_CASES = {
    "loads off": dict(HGS_OPT_EMPTY_COL_LOADS=0),
    "inverse off": dict(HGS_OPT_EMPTY_COL_INVERSE=0),
    "forward off": dict(HGS_OPT_EMPTY_COL_FORWARD=0),
    "prezero off": dict(HGS_OPT_EMPTY_COL_PREZERO=0),
    "PHASE 1 (WGS-Kim stores the farfield phase)": dict(method=KIM, store_phase=1),
    "PHASE 2 (WGS-Kim reads it)": dict(method=KIM, use_fixed=1),
    "2048 rows": dict(Ph=2048, Sh=520),
    "six slots": dict(Sh=1500),
    "a weight written outside the scan": dict(w_outside_scan=1),
    "a dirty scan": dict(sparse_dirty=1),
    "a dirty scan that counted nothing": dict(sparse_dirty=1, n_active=0),
    "MRAF": dict(mraf=1),
    "MRAF, normalised weights (pre-sum form)": dict(mraf=1, w_unit=1),
    "MRAF without an update": dict(mraf=1, do_update=0),
    "statistics": dict(stat_groups=1),
    "spot statistics": dict(stat_groups=2),
    "Nogrette": dict(method=NOGRETTE),
    "fp64": dict(elem=8),
    "column lists": dict(sparse_enabled=1, HGS_OPT_SPARSE_COLUMNS=1),
    "half-width kernel off": dict(HGS_TILE2=0),
    "8192 rows": dict(Ph=8192, Pw=8192, Sh=2304),
}


@pytest.mark.parametrize("why", sorted(FALSE_CASES))
def test_false(host, why):
    for batch in (1, 8):
        got = _ask(host, B=batch, **FALSE_CASES[why])
        assert got["ok"] == 0, (why, batch, got)


def test_the_switch_alone_changes_no_plan(host):
    """HGS_OPT_EMPTY_COL_PREZERO off: the same main launch, only the predicate turns."""
    on, off = _ask(host), _ask(host, HGS_OPT_EMPTY_COL_PREZERO=0)
    assert on["ok"] == 1 and off["ok"] == 0
    assert {k: v for k, v in on.items() if k != "ok"} == {k: v for k, v in off.items() if k != "ok"}
