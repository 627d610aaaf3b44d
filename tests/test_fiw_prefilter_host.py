"""Host: the fused chain's neighbour prefilter (csrc/fiw_box.h box_pre / box_pre_rejects) only ever
rejects what the full test (sup_box_tiles + the box overlap) rejects. tests/host/fiw_prefilter_check.cpp
is built with the host compiler (no FMA contraction, as the device build) and run on the CPU: random
grids, bounds and disks, disks whose reach lies on and a few ulps around every edge of the box's tiles,
huge, tiny, non-finite and negative values."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "maximumareacoverageoptimization.jl_amd", "csrc")


def test_prefilter_passes_a_superset(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (the package's own build needs one)")
    exe = str(tmp_path / "fiw_prefilter_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "host", "fiw_prefilter_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "counterexamples 0" in r.stdout
