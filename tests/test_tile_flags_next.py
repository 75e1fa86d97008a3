"""
The walk to the next non-empty half tile, without a GPU: ``tile2_next_nonempty`` of ``slmsuite_amd/csrc/tile_flags.hpp`` is plain
C++ that ``col_tile2_kernel`` instantiates with a scalar load of the scan's flag words (``ColArgs::h_prezeroed``).
``tests/tile_flags_next_host.cpp`` instantiates it with a bounds-checked loader over a 64-tile row and compares every walk with
a brute-force one (strides 1, 8 and 32, both halves, "none left", the last byte of the last word); it is built as the
stand-alone program it is, with AddressSanitizer and UndefinedBehaviorSanitizer.  Nothing is loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slmsuite_amd", "csrc")


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
    exe = str(tmp_path_factory.mktemp("tile_flags_next") / "tile_flags_next_host")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, os.path.join(ROOT, "tests", "tile_flags_next_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_walk_matches_brute_force(host):
    r = subprocess.run([host], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[0] == "checked" and int(tail[3]) == 0, r.stdout[-2000:]
    assert int(tail[1]) > 1_000_000, r.stdout[-200:]


def test_kernel_walks_through_the_helper_only():
    """col_tile2_kernel finds its next half tile through the helper, fed by the scalar load: no second spelling of the walk."""
    src = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert src.count("tile2_next_nonempty(flag_word") == 2
    assert "auto flag_word = [&](int i) { return uniform_load_i32(cflag4 + i); };" in src
    hdr = open(os.path.join(CSRC, "tile_flags.hpp")).read()
    assert "hip/" not in hdr and "__global__" not in hdr
