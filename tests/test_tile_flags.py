"""
The flag word of a four-column tile, without a GPU: ``slmsuite_amd/csrc/tile_flags.hpp`` is plain C++ that the kernel and host
code share.  ``tests/tile_flags_host.cpp`` checks its decoders (column active, half tile empty) over all 2^16 values of either
half word and for -1 ("every column fetched") against the definition spelled out byte by byte; it is built as the stand-alone
program it is, with AddressSanitizer and UndefinedBehaviorSanitizer (the shifts of a word that may be negative).
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
    exe = str(tmp_path_factory.mktemp("tile_flags") / "tile_flags_host")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, os.path.join(ROOT, "tests", "tile_flags_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_header_includes_no_hip():
    src = open(os.path.join(CSRC, "tile_flags.hpp")).read()
    assert "hip/" not in src and "__global__" not in src


def test_decoders_match_the_definition_over_every_half_word(host):
    r = subprocess.run([host], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[0] == "checked" and int(tail[3]) == 0, r.stdout[-2000:]
    assert int(tail[1]) >= 2 * 8 * 65536 * 6, r.stdout[-200:]


def test_kernel_spells_no_flag_shift_of_its_own():
    """col_tile2_kernel decodes its flag word only through the helpers."""
    src = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert "fw >> (16 * half" not in src and "fwn >> (16 * half" not in src
    assert src.count("tile2_col_active(") >= 4 and src.count("tile2_half_empty(") >= 2
