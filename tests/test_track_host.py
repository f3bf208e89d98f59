"""The host logic of the loop-track stage (sim3opt_amd/csrc/track_host.hpp, track_math.hpp) on the CPU, under
AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program (tests/cxx/track_host_driver.cpp) checks every
refusal message of the argument checks as an exact string, the frame of an observation across frames that own nothing,
every kind of absent depth, and holds the serial restatement (union-find) against a second one organised as label
propagation on random ragged batches."""
import os
import subprocess

from test_devmem_owners import SAN
from test_example_cpp import ROOT


def test_host_logic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "track_host_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + SAN +
                          [os.path.join(ROOT, "tests", "cxx", "track_host_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("track host ok"), r.stdout[-2000:]
