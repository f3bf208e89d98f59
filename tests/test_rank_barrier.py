"""The host side of the in-process transport (sim3opt_set_devices): the fail-fast barrier of csrc/rank_barrier.hpp and
the two-mailbox parity scheme, as a stand-alone program under ThreadSanitizer (tests/cxx/rank_barrier_driver.cpp).
No GPU and nothing loaded into this interpreter: the program has its own main."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rank_barrier_driver_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "rank_barrier_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "sim3opt_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "rank_barrier_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert "ThreadSanitizer" not in out, out  # a report fails the test, whatever the program printed
    assert r.returncode == 0, out
    assert "9 passed, 0 failed" in r.stdout, out
