"""
Shared by the host-side tests of ``slmsuite_amd/csrc/column_plan.hpp`` and ``tile_flags.hpp``: find a host C++ compiler, build a
stand-alone program of ``tests/*.cpp`` against the headers, and ask ``tests/column_plan_host.cpp`` for the plan of one body.
Nothing is loaded into Python.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slmsuite_amd", "csrc")
GS, LEONARDO, KIM, NOGRETTE, WU, TANH = range(6)


_BUILT = {}


def build(tmp_path_factory, name, *flags):
    """tests/<name>.cpp -> executable, built once per session (skips where the machine has no host compiler)"""
    if (name, flags) not in _BUILT:
        _BUILT[name, flags] = _build(tmp_path_factory, name, *flags)
    return _BUILT[name, flags]


def _build(tmp_path_factory, name, *flags):
    for cxx in ("c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/bin/amdclang++"):
        cxx = shutil.which(cxx)
        if cxx:
            break
    else:
        pytest.skip("no host C++ compiler (c++ / clang++) on this machine")
    exe = str(tmp_path_factory.mktemp(name) / name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build(tmp_path_factory, "column_plan_host")


def plan(exe, *, preset=None, next=None, **facts):
    """The plan of one body: facts as key=value; ``preset="cfg2"`` starts from the cfg-2-like body; ``next`` names the facts in which
    the body after it differs (``close_next`` of the result is the row launch between the two)."""
    words = ([f"preset={preset}"] if preset else []) + [f"{k}={int(v)}" for k, v in facts.items()]
    if next is not None:
        words += ["next:"] + [f"{k}={int(v)}" for k, v in next.items()]
    r = subprocess.run([exe, "plan"], input=" ".join(words) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)
