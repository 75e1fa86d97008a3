"""
The stream-K schedule of the separable path's complex GEMMs, without a GPU: ``slmsuite_amd/csrc/streamk_schedule.hpp`` is
plain C++ (no HIP), shared by the kernel (``cgemm_streamk``: sk_begin), the engine's tables (``sk_fill``: first workgroup and
number of partial planes per output tile, and the sizes of the plane buffers) and the consumers that add ``nseg[tile]``
planes.  ``tests/streamk_schedule_host.cpp`` replays the kernel's control flow for one (tiles_m, tiles_n, KT, G) -- the
lo / hi range, the (tile, kt) advance, the store condition ``nkt == 0 || !more``, ``seg = w - first_wg[tile]`` and the EPI 1
``slot`` -- and counts violations of:

  a. every workgroup has lo < hi whenever G <= total;
  b. every k-step of every tile is accumulated exactly once (into accumulators that hold no other tile, nothing left unstored);
  c. every (tile, seg) is stored exactly once, 0 <= seg < nseg[tile] <= planes;
  d. the segs of a tile are exactly 0 .. nseg - 1, no hole (the consumers add a prefix), and hold KT steps between them;
  e. planes == max nseg;
  f. slot < tiles_n * 2 * planes, and every store lies inside the buffer sizes the header gives for ``planes``;
  g. first_wg[t] + nseg[t] - 1 == sk_owner(last step of t).

This file asserts what the schedule SAYS; tests/test_streamk_gemm.py asserts what the kernels COMPUTE under it.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (tiles_m, tiles_n, KT) of the n2f and f2n GEMMs of the shapes tests/test_streamk_gemm.py runs, and its caps
# n2f: spots x SLM rows over SLM columns / 16; f2n: SLM rows x SLM columns over spots / 16 (tiles of 128)
SMALL = dict(n2f=(3, 2, 13), f2n=(2, 2, 19))          # SLM (150, 200), 300 spots
EXACT = dict(n2f=(2, 1, 16), f2n=(1, 2, 16))          # SLM (128, 256), 256 spots
NATURAL = dict(n2f=(4, 6, 64), f2n=(6, 8, 25))        # SLM (768, 1024), 400 spots
SMALL_CAPS = (1, 2, 3, 5, 7, 16, 0)
EXACT_CAPS = (1, 3, 0)
DEVICE_G = 512                                         # 2 x 256 CUs; a CPX partition shows 32 CUs: 64


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
    exe = str(tmp_path_factory.mktemp("streamk_schedule") / "streamk_schedule_host")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "slmsuite_amd", "csrc"),
                        os.path.join(ROOT, "tests", "streamk_schedule_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _case(exe, shape, cap, device_g=DEVICE_G):
    """The schedule the engine launches for HGS_OPT_SEP_WORKGROUPS = cap: G = min(cap or 2 #CU, 2 #CU, total)."""
    g = min(cap, device_g) if cap > 0 else device_g
    r = subprocess.run([exe, "case", *[str(v) for v in shape], str(g)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    d = json.loads(lines[-1])
    assert d["bad"] == 0, "\n".join(lines[:20])
    return d


def test_header_includes_no_hip():
    src = open(os.path.join(ROOT, "slmsuite_amd", "csrc", "streamk_schedule.hpp")).read()
    assert "hip/" not in src and "__global__" not in src and "hipLaunch" not in src and "#include \"" not in src


def test_invariants_over_a_swept_grid_of_schedules(host):
    """tiles_m, tiles_n in 1..6, KT in 1..40, G in 1..min(total, 64): invariants a - g of this file's docstring."""
    r = subprocess.run([host, "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tail = r.stdout.strip().splitlines()
    assert tail and tail[-1].startswith("checked "), r.stdout[-2000:]
    n_checked, n_bad = int(tail[-1].split()[1]), int(tail[-1].split()[3])
    assert n_bad == 0, "\n".join(tail[:40])
    assert n_checked == sum(min(64, tm * tn * kt) for tm in range(1, 7) for tn in range(1, 7) for kt in range(1, 41)), tail[-1]


def test_shapes_the_product_meets(host):
    """cfg 4 (1e4 spots on 1152 x 1920): n2f 79 x 9 tiles of 120 steps, f2n 9 x 15 tiles of 625, on 256 and on 32 CUs."""
    for shape in ((79, 9, 120), (9, 15, 625)):
        for g in (512, 64):
            d = _case(host, shape, 0, device_g=g)
            assert d["G"] == g and d["maxlen"] > 2 and d["prefetch"] > 0, d
    # 64 workgroups: ranges of 1333 and 1318 steps, longer than KT in both GEMMs -- every workgroup holds whole tiles
    assert _case(host, (79, 9, 120), 0, device_g=64)["whole"] == 64
    assert _case(host, (9, 15, 625), 0, device_g=64)["whole"] == 64


def test_gpu_test_shapes_reach_the_regimes_they_claim(host):
    """What tests/test_streamk_gemm.py says each cap exercises, from the replay of the schedule itself."""
    for shapes, caps in ((SMALL, SMALL_CAPS), (EXACT, EXACT_CAPS), (NATURAL, (0,))):
        for shape in shapes.values():
            for cap in caps:
                _case(host, shape, cap)                        # (no violation)
    n, f = SMALL["n2f"], SMALL["f2n"]
    # cap 1: one workgroup walks all 6 (4) tiles, every one whole: 5 (3) stores with cleared accumulators inside the range
    for shape, tiles in ((n, 6), (f, 4)):
        d = _case(host, shape, 1)
        assert (d["G"], d["planes"], d["whole"], d["mid"], d["aligned"]) == (1, 1, 1, tiles - 1, 1), d
        assert d["maxlen"] == tiles * shape[2]
    # cap 2: ranges of 3 and 2 whole tiles
    assert _case(host, n, 2)["maxlen"] == 3 * 13 and _case(host, f, 2)["maxlen"] == 2 * 19
    for shape in (n, f):
        d = _case(host, shape, 2)
        assert (d["planes"], d["whole"], d["aligned"]) == (1, 2, 2), d
    # cap 3 on n2f: 26 steps = exactly two tiles each: every range ends on a boundary (nkt == 0 and !more at once)
    d = _case(host, n, 3)
    assert (d["planes"], d["maxlen"], d["aligned"], d["whole"]) == (1, 26, 3, 3), d
    # cap 3 on f2n, cap 5 on n2f: ranges that cross a boundary and hold a whole tile too; two planes
    for shape, cap in ((f, 3), (n, 5)):
        d = _case(host, shape, cap)
        assert d["planes"] == 2 and d["whole"] >= 2 and d["cross"] >= 3 and d["mid"] >= 3, d
    # cap 7: crossings without a whole tile, 2 and 3 planes
    dn, df = _case(host, n, 7), _case(host, f, 7)
    assert (dn["planes"], df["planes"]) == (2, 3) and dn["whole"] == df["whole"] == 0 and dn["cross"] == 5 and df["cross"] == 3
    # cap 16: several workgroups per tile, multi-step ranges (the prefetch runs), four planes
    for shape in (n, f):
        d = _case(host, shape, 16)
        assert d["planes"] == 4 and d["whole"] == 0 and d["maxlen"] == 5 and d["prefetch"] > 0, d
    # cap 0 on 256 CUs: one step per workgroup, a plane per k-step, no prefetch
    for shape in (n, f):
        d = _case(host, shape, 0)
        assert (d["G"], d["planes"], d["maxlen"], d["prefetch"]) == (shape[0] * shape[1] * shape[2], shape[2], 1, 0), d
    # the exact-multiple shape: whole tiles at cap 1, a crossing at cap 3, one step per workgroup at cap 0
    for shape in EXACT.values():
        assert _case(host, shape, 1)["mid"] == 1 and _case(host, shape, 3)["cross"] == 1 and _case(host, shape, 0)["maxlen"] == 1
    # the natural schedule of the larger shape on 256 CUs: 3.0 and 2.34 steps per workgroup, 22 and 11 planes, 16 crossings each
    dn, df = _case(host, NATURAL["n2f"], 0), _case(host, NATURAL["f2n"], 0)
    assert (dn["G"], dn["planes"], dn["maxlen"], dn["cross"]) == (512, 22, 3, 16), dn
    assert (df["G"], df["planes"], df["maxlen"], df["cross"]) == (512, 11, 3, 16), df
    # ... and what a 32-CU partition would launch for it (64 workgroups) holds up as well
    for shape in NATURAL.values():
        assert _case(host, shape, 0, device_g=64)["G"] == 64
