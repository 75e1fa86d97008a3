"""
Register budget of pattern_kernel (csrc/pattern_kernels.hpp): the two translation units that hold its instances are compiled
with -Rpass-analysis=kernel-resource-usage (hipcc cross-compiles gfx950 without a GPU), with the flags of their Makefile
rule, and every instance must come out without scratch and without spilled registers.  The parameters travel by value:
an indexed read of the four quadrant sets would move them to scratch, which this test is there to notice.
"""
import concurrent.futures
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slmsuite_amd", "csrc")
UNITS = ["launch_pattern_f32.hip", "launch_pattern_f64.hip"]


def _usage(unit):
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-fPIC", "-Wno-unused-value",
           "-Wno-unused-function", "-c", unit, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-2000:]
    rows, name, row = [], None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name, row = m.group(1), {}
        for key, tag in (("vgprs", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
                         ("vgpr_spill", r"VGPRs Spill: (\d+)")):
            m = re.search(tag, line)
            if m:
                row[key] = int(m.group(1))
        if name and "vgpr_spill" in row:
            rows.append((name, row))
            name = None
    return rows


@pytest.mark.skipif(shutil.which("hipcc") is None or shutil.which("c++filt") is None, reason="needs hipcc")
def test_pattern_kernels_use_no_scratch():
    with concurrent.futures.ThreadPoolExecutor(max_workers=2) as pool:
        rows = [r for unit in pool.map(_usage, UNITS) for r in unit]
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.splitlines()
    seen, bad = set(), []
    for (_, row), text in zip(rows, names):
        m = re.match(r"void hgs::pattern_kernel<(\w+), (\w+), (\w+), (\d+)>\(", text)
        if not m:
            continue
        seen.add(m.groups())
        if row["scratch"] or row["sgpr_spill"] or row["vgpr_spill"] or row["vgprs"] > 128:
            bad.append((m.groups(), row))
    assert not bad, bad
    # grid type x stored type x product / full x the six modes
    assert seen == {(g, o, p, str(mode)) for g in ("float", "double") for o in ("float", "double") for p in ("true", "false") for mode in range(6)}
