"""The host logic of the bundle-adjustment covariances (sim3opt_amd/csrc/ba_cov_host.hpp) on the CPU, under
AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program (tests/cxx/ba_cov_host_driver.cpp) builds the tables
of a hand-made map whose factor is a chain and plans requests on it -- empty ones, duplicates, out-of-range indices,
camera pairs outside the factor's pattern, and a point whose observers include a fixed camera."""
import os
import subprocess

from test_devmem_owners import SAN
from test_example_cpp import ROOT


def test_host_logic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ba_cov_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN +
                          [os.path.join(ROOT, "tests", "cxx", "ba_cov_host_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("ba cov host ok"), r.stdout[-2000:]
