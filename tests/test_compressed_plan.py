"""
What the host decides about a compressed (CompressedSpotHologram) problem, without a GPU:
``slmsuite_amd/csrc/compressed_plan.hpp`` is plain C++ (no HIP), so the classification of the term list, the product-grid
and regular-axis tests, the spot chunks of the run kernels and the choice of kernel form are checked here on the plan itself,
at the points tests/test_dispatch.py::test_compressed_forms observes on the device and at the ones no GPU test reaches (a grid
that is no product grid, an irregular axis, a single column, a cross term, the vortex plate, an unrecognised term, the
spot-count threshold).  This file asserts what the plan SAYS; the GPU dispatch test keeps asserting what was LAUNCHED.
"""
import itertools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slmsuite_amd", "csrc")
SEP_MAXDEG, C_MTAB = 8, 16              # compressed_sep.hpp, compressed_kernels.hpp (test_constants_match_the_kernels)

# term lists (px, py) as toolbox.zernike_monomial_weights orders them (ascending Cantor order, pseudo-terms last)
KXY2 = [(1, 0), (0, 1)]                                             # ANSI 2, 1
KXY3 = [(0, 0), (1, 0), (0, 1), (2, 0), (0, 2)]                     # ANSI 2, 1, 4: Z4 = 2 x^2 + 2 y^2 - 1
ANSI5 = [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2)]            # ANSI 2, 1, 4, 3, 5: Z3 = 2 x y
DEG3 = ANSI5 + [(3, 0), (2, 1), (1, 2), (0, 3)]                     # ANSI 1 .. 9
VORTEX = KXY2 + [(-1, 0)]


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
    exe = str(tmp_path_factory.mktemp("compressed_plan") / "compressed_plan_host")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                        os.path.join(ROOT, "tests", "compressed_plan_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _ask(exe, lines):
    """one process for all the cases: a line each in, a JSON object each out"""
    r = subprocess.run([exe, "cases"], input="".join(line + "\n" for line in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(lines), r.stdout[-2000:]
    return out


def _num(v):
    return float(v).hex()


def _terms(terms, maxdeg=SEP_MAXDEG):
    return f"terms {maxdeg} " + " ".join(f"{px} {py}" for px, py in terms)


def _form(**kw):
    f = dict(elem=4, sep_valid=1, run_valid=1, opt_separable=1, opt_sep_min=96, opt_run=1, n_spots=120, n_monomials=2, degree=1,
             mono_tab=1, c_mtab=C_MTAB)
    assert set(kw) <= set(f), kw
    f.update(kw)
    return "form " + " ".join(str(int(v)) for v in f.values())


def test_header_includes_no_hip():
    src = open(os.path.join(CSRC, "compressed_plan.hpp")).read()
    assert "hip/" not in src and "__global__" not in src and "hipLaunch" not in src
    assert '#include "' not in src.replace('#include "../../include/hgs.h"', "")


def test_constants_match_the_kernels():
    assert f"constexpr int SEP_MAXDEG = {SEP_MAXDEG};" in open(os.path.join(CSRC, "compressed_sep.hpp")).read()
    assert f"constexpr int C_MTAB = {C_MTAB};" in open(os.path.join(CSRC, "compressed_kernels.hpp")).read()


def test_both_directions_take_one_choice():
    """the engine asks the plan in one place, and n2f and f2n both go through it"""
    src = open(os.path.join(CSRC, "compressed_backend.hpp")).read()
    assert src.count("choose_form(") == 1
    for head in ("int n2f(const View& v) {", "int f2n(const View& v, Cx<R>* nf_out) {"):
        body = src[src.index(head):]
        assert body[len(head):].lstrip().startswith("const CFormChoice c = form();"), head


def test_term_lists(host):
    got = _ask(host, [_terms(KXY2), _terms(KXY3), _terms(ANSI5), _terms(DEG3), _terms(VORTEX),
                      _terms(KXY2 + [(-2, 0)]), _terms([(0, -1)] + KXY2), _terms(VORTEX + [(-1, 1)]),
                      _terms([(9, 0), (0, 1)]), _terms([(8, 0), (0, 8)]), _terms([(3, 0), (0, 1)], maxdeg=2)])
    assert got[0] == dict(degree=1, bad=-1, separable=1, dx=1, dy=1)
    assert got[1] == dict(degree=2, bad=-1, separable=1, dx=2, dy=2)
    assert got[2]["degree"] == 2 and got[2]["bad"] == -1 and not got[2]["separable"]        # the xy term
    assert got[3]["degree"] == 3 and got[3]["bad"] == -1 and not got[3]["separable"]
    assert got[4]["degree"] == 3 and got[4]["bad"] == -1 and not got[4]["separable"]        # vortex plate: the general kernels
    assert got[5]["bad"] == 2 and got[6]["bad"] == 0                                        # rejected, with the offending index
    assert got[7]["bad"] == 3 and got[7]["degree"] == 3                                     # (the plate before it was seen)
    assert not got[8]["separable"] and got[8]["degree"] == 9                                # beyond SEP_MAXDEG
    assert got[9] == dict(degree=8, bad=-1, separable=1, dx=8, dy=8)
    assert not got[10]["separable"]
    # ... and the kernels these lists get where nothing but the per-pixel form applies
    px = dict(sep_valid=0, run_valid=0)
    forms = _ask(host, [_form(degree=got[0]["degree"], **px), _form(degree=got[1]["degree"], n_monomials=5, **px),
                        _form(degree=3, n_monomials=len(DEG3), **px), _form(degree=3, n_monomials=len(DEG3), mono_tab=0, **px),
                        _form(degree=3, n_monomials=C_MTAB, **px), _form(degree=3, n_monomials=C_MTAB + 1, **px),
                        _form(degree=got[4]["degree"], n_monomials=len(VORTEX), **px)])
    assert [(f["form"], f["deg"]) for f in forms] == [("pixel", 1), ("pixel", 2), ("pixel", 3), ("pixel", 0), ("pixel", 3), ("pixel", 0),
                                                      ("pixel", 3)]


def test_canonical_slots(host):
    """[1, x, y, x2, xy, y2]; the weights of repeated terms accumulate in their slot"""
    order = [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2)]
    w = [1.0, 2.0, 4.0, 8.0, 16.0, 32.0]
    shuffled = [5, 2, 0, 3, 1, 4]
    lines = ["slots 6 " + " ".join(f"{order[k][0]} {order[k][1]}" for k in shuffled) + " " + " ".join(_num(w[k]) for k in shuffled),
             "slots 4 1 0 0 2 1 0 0 2 " + " ".join(_num(v) for v in (0.5, 3.0, 0.25, -1.0)),
             "slots 1 0 1 " + _num(7.0)]
    got = _ask(host, lines)
    assert got[0]["c"] == w
    assert got[1]["c"] == [0, 0.75, 0, 0, 0, 2.0]
    assert got[2]["c"] == [0, 0, 7.0, 0, 0, 0]


def _grid(kind, axis, a):
    return f"grid {kind} {axis} {a.shape[0]} {a.shape[1]} " + " ".join(_num(v) for v in a.ravel())


def test_product_grid(host):
    H, W = 5, 7
    xs = np.linspace(-0.7, 0.9, W).astype(np.float32)
    ys = np.linspace(-0.3, 0.4, H).astype(np.float32)
    xg, yg = np.meshgrid(xs, ys)
    assert xg.shape == (H, W)
    bad_x, bad_y = xg.copy(), yg.copy()
    bad_x[3, 4] = np.nextafter(bad_x[3, 4], np.float32(2))        # one ulp, in a later row
    bad_y[4, 6] = np.nextafter(bad_y[4, 6], np.float32(-2))
    x64, y64 = np.meshgrid(np.linspace(-1, 1, W), np.linspace(-1, 1, H))
    bad64 = x64.copy()
    bad64[H - 1, 0] = np.nextafter(bad64[H - 1, 0], 2.0)
    got = _ask(host, [_grid("f32", 0, xg), _grid("f32", 1, yg), _grid("f32", 0, bad_x), _grid("f32", 1, bad_y),
                      _grid("f32", 0, yg), _grid("f32", 1, xg),
                      _grid("f32", 0, xg[:1]), _grid("f32", 1, xg[:1]), _grid("f32", 1, yg[:1]),
                      _grid("f32", 0, xg[:, :1]), _grid("f32", 1, yg[:, :1]), _grid("f32", 0, yg[:, :1]),
                      _grid("f64", 0, x64), _grid("f64", 1, y64), _grid("f64", 0, bad64)])
    assert got[0] == dict(sep=1, axis=[float(v) for v in xs]) and got[1] == dict(sep=1, axis=[float(v) for v in ys])
    assert got[2]["sep"] == 0 and got[3]["sep"] == 0
    assert got[2]["axis"] == got[0]["axis"] and got[3]["axis"] == got[1]["axis"]      # row 0 / column 0 either way
    assert got[4]["sep"] == 0 and got[5]["sep"] == 0                                  # the grids swapped
    # H = 1: any x grid is a product grid, a y grid only when its one row is constant
    assert got[6] == dict(sep=1, axis=[float(v) for v in xs]) and got[7]["sep"] == 0 and got[8] == dict(sep=1, axis=[float(ys[0])])
    # W = 1: any y grid is, an x grid only when its one column is constant
    assert got[9] == dict(sep=1, axis=[float(xs[0])]) and got[10] == dict(sep=1, axis=[float(v) for v in ys]) and got[11]["sep"] == 0
    assert got[12] == dict(sep=1, axis=list(np.linspace(-1, 1, W))) and got[13]["sep"] == 1 and got[14]["sep"] == 0


def _axis(xs):
    return f"axis {len(xs)} " + " ".join(_num(v) for v in xs)


def test_regular_axis(host):
    W = 93
    xs = np.linspace(-0.37, 0.41, W).astype(np.float32).astype(float)          # what the engine sees: fp32 roundings
    moved = xs.copy()
    moved[W // 3] += 4e-7 * np.abs(xs).max()
    down = xs[::-1].copy()
    quad = xs + 1e-3 * xs ** 2
    got = _ask(host, [_axis(xs), _axis(moved), _axis(xs[:1]), _axis(down), _axis(xs[:2]), _axis(quad), _axis(np.zeros(4))])
    assert got[0]["ok"] == 1 and got[0]["x0"] == xs[0] and got[0]["hx"] == (xs[-1] - xs[0]) / (W - 1)
    assert got[1]["ok"] == 0
    assert got[2]["ok"] == 0                                                   # W = 1: no step
    assert got[3]["ok"] == 1 and got[3]["x0"] == xs[-1] and got[3]["hx"] == -got[0]["hx"]     # descending: a negative step
    assert got[4]["ok"] == 1 and got[5]["ok"] == 0
    assert got[6] == dict(ok=1, x0=0, hx=0)                                    # (a constant axis: the 1e-30 of the tolerance)


def test_form_choice_at_the_points_of_the_dispatch_test(host):
    """tests/test_dispatch.py::test_compressed_forms: a 96 x 128 SLM, kxy basis (product grid, regular x axis)"""
    got = _ask(host, [_form(n_spots=120), _form(n_spots=40), _form(n_spots=40, n_monomials=5, degree=2),
                      _form(n_spots=120, opt_sep_min=200), _form(n_spots=120, elem=8, sep_valid=0, run_valid=0),
                      _form(n_spots=120, elem=8), _form(n_spots=40, opt_run=0), _form(n_spots=96), _form(n_spots=95),
                      _form(n_spots=120, opt_separable=0), _form(n_spots=120, sep_valid=0, run_valid=0, opt_run=1)])
    assert [(f["form"], f["deg"]) for f in got] == [
        ("sep_gemm", 0), ("run", 1), ("run", 2), ("run", 1), ("pixel", 1), ("pixel", 1), ("pixel", 1), ("sep_gemm", 0), ("run", 1),
        ("run", 1), ("pixel", 1)]


def test_form_choice_invariants_over_the_product_of_the_facts(host):
    """fp64 never gets the separable or the run form; separable needs valid tables, the option and n_spots >= the minimum; run
    needs valid records, the option and degree <= 2; otherwise per-pixel, DEG 3 only within C_MTAB terms and with the table
    switched on; both directions equal."""
    r = subprocess.run([host, "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tail = r.stdout.strip().splitlines()
    assert tail and tail[-1].startswith("checked "), r.stdout[-2000:]
    n_checked, n_bad = int(tail[-1].split()[1]), int(tail[-1].split()[3])
    assert n_bad == 0, "\n".join(tail[:40])
    assert n_checked == 2 * 2 * 2 * 2 * 3 * 2 * 8 * 8 * 6 * 2, tail[-1]


def test_run_chunking(host):
    cases = list(itertools.product((1, 63, 64, 65, 137, 10000), (1, 256), (1, 6, 96, 768, 4096, 100000)))
    got = _ask(host, [f"chunks {n} {cu} {rb}" for n, cu, rb in cases])
    for (n, cu, rb), c in zip(cases, got):
        assert c["nper"] % 64 == 0 and c["nper"] >= 64, (n, cu, rb, c)
        assert c["chunks"] * c["nper"] >= n and (c["chunks"] - 1) * c["nper"] < n and 1 <= c["chunks"] <= 8, (n, cu, rb, c)
    # cfg4: 10000 spots on 256 CUs; few workgroups -> eight chunks of 1280, many -> fewer, larger ones
    by = {k: v for k, v in zip(cases, got)}
    assert by[(10000, 256, 768)] == dict(nper=1280, chunks=8)
    assert by[(10000, 256, 4096)] == dict(nper=5056, chunks=2)
    assert by[(10000, 256, 100000)] == dict(nper=10048, chunks=1)
