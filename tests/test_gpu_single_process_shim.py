"""SparseOptimizer::setDevices of the g2o-named shim (include/sim3opt_g2o.hpp) against sim3opt_set_devices of the C-ABI:
tests/cxx/single_process_conformance.cpp, four ranks on device 0, the suite's 300-vertex graph handed over as text."""
import os
import subprocess

import pytest

from sim3opt_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_single_process_shim_gpu_part(tmp_path):
    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan(300, 2500, dims=(7, 7, 4), per_cell=4)
    path = str(tmp_path / "graph.txt")
    with open(path, "w") as f:
        f.write(f"{len(g['states'])} {len(g['v0'])}\n")
        for s, fx in zip(g["states"], g["fixed"]):
            f.write(f"{int(fx)} " + " ".join(f"{x:.17g}" for x in s) + "\n")
        for a, b, m in zip(g["v0"], g["v1"], g["meas"]):
            f.write(f"{int(a)} {int(b)} " + " ".join(f"{x:.17g}" for x in m) + "\n")
    exe = str(tmp_path / "single_process_conformance")
    libdir = os.path.join(ROOT, "sim3opt_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-DSIM3OPT_G2O_NAMES",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_eigen"),
                           os.path.join(ROOT, "tests", "cxx", "single_process_conformance.cpp"), "-L" + libdir,
                           "-lsim3opt", "-Wl,-rpath," + libdir, "-o", exe])
    r = subprocess.run([exe, "gpu", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
