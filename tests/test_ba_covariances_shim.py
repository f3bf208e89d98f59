"""The covariance part of the g2o-named bundle-adjustment shim (include/sim3opt_g2o_ba.hpp): Vertex::hessianIndex, the
header's SparseBlockMatrix and SparseOptimizer::computeMarginals, through tests/cxx/ba_covariances_conformance.cpp,
compiled against the tests-only Eigen mock the other conformance programs use."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_program(tmp_path):
    exe = str(tmp_path / "ba_covariances_conformance")
    libdir = os.path.join(ROOT, "sim3opt_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-DSIM3OPT_G2O_BA_NAMES",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_eigen"),
                           os.path.join(ROOT, "tests", "cxx", "ba_covariances_conformance.cpp"), "-L" + libdir,
                           "-lsim3opt", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_ba_covariances_shim_host_part(tmp_path):
    r = subprocess.run([compile_program(tmp_path), "host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout


@pytest.mark.gpu
def test_ba_covariances_shim_matches_the_c_abi(tmp_path):
    r = subprocess.run([compile_program(tmp_path), "gpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout and "ba covariances: camera 16" in r.stdout
